// spgg_dwell.h — the per-agent strategy dwell record (spgg_dwell.hip): how often each agent has
// changed strategy since a reference iteration, since when it holds its current one and for how
// long it has cooperated -- persistence, the two-time autocorrelation and the strategy ages.
//
// Nothing in the reference carries state like this from one iteration to the next.  Unlike the
// other records it is not a function of one instant: an accumulator of three words per agent is
// updated by one launch after every step launch, and two read-outs turn it into a row of counts
// or into per-agent fields.  No workgroup waits for another and every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_dw {

// Per agent: (flips, since, coop_closed), interleaved as [n_rep][n][3] uint32 -- one 12-byte load
// and store per flipping agent, none for the others.  Every field is below 2^26 (spgg_create's
// bound on iterations).
constexpr int kWords = 3;
constexpr int kMaxIterLog2 = 26;
constexpr int kAgeBins = kMaxIterLog2 + 1;           // bin floor(log2(age + 1)), age + 1 <= 2^26
constexpr int kSlots = 7 + 2 * kAgeBins;             // SPGG_DWELL_SLOTS
static_assert(kAgeBins == SPGG_DWELL_AGE_BINS && kSlots == SPGG_DWELL_SLOTS, "the row layout of spgg_abi.h");
static_assert(kSlots == 61, "the row width stated in spgg_abi.h");

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// Step launch: a thread owns 16 consecutive agents (four dwords of each S plane), a workgroup 4096.
constexpr int kRun = 16;
constexpr int kStepCells = kThreads * kRun;
// Read-outs and reset: a thread takes 16 agents kThreads apart (coalesced bytes), a workgroup 4096:
// cfg3's 40,000 cells make 10 workgroups per replica, cfg5's 10^6 make 245.
constexpr int kCells = 4096;
// A workgroup's FLIPS / COOP_TIME partials reach kCells * 2^26 = 2^38: they are 64-bit from the
// thread on.  Counts (<= kCells per workgroup) are 32-bit until the atomic.
static_assert((long long)kCells << kMaxIterLog2 > (1ll << 32), "why the two sums are 64-bit");

// ref = S_{t_ref} & 1 and words = (0, t_ref, 0) of every agent, from plane (t_ref - 1) & 1 (an
// absorbed replica: the plane of its absorbing iteration).
void launch_reset(const spgg_obs::Lattices& lat, int t_ref, uint32_t* words, uint8_t* ref, hipStream_t s);

// After the step launch of iteration j (S_j in plane (j - 1) & 1, S_{j+1} in plane j & 1): the
// words of every agent whose strategy changed.  Replicas absorbed at or before j are skipped.
void launch_step(const spgg_obs::Lattices& lat, int j, uint32_t* words, hipStream_t s);

// The kSlots-value row of S_t per replica (a zeroing launch, then one that adds into it).
void launch_record(const spgg_obs::Lattices& lat, int t, int t_ref, const uint32_t* words, const uint8_t* ref,
                   long long* out, int64_t out_stride, hipStream_t s);

// The per-agent fields flips, age, coop of S_t: int32 [3][n] per replica.
void launch_fields(const spgg_obs::Lattices& lat, int t, int t_ref, const uint32_t* words, int32_t* out,
                   int64_t out_stride, hipStream_t s);

}  // namespace spgg_dw
