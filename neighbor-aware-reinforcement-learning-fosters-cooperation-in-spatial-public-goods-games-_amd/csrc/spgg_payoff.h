// spgg_payoff.h — the payoff field's record (spgg_payoff.hip): per replica the census of the agents
// by (strategy, cooperating neighbours, group-cooperator total K), the bonds between right / lower
// neighbours by their difference in K, the one-byte-per-agent plane they are made from, and the
// pair sums of that plane at every distance.
//
// With c = 1 on cooperators (bit 0 of S_t clear), N = sum5(c) and K = sum5(N) in 0 .. 25, an agent's
// normalised payoff is ((r c / 5) K - 5 cost c_i - (r - 5)) / (4 r - (r - 5)) in real arithmetic: the
// integer census of (sigma, K) is the payoff distribution for any parameters.  Nothing in the
// reference computes these (its view of the payoffs: three lattice sums per iteration).  The kernels
// read S_t in place; no workgroup waits for another and every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_pf {

// ---- census --------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// A workgroup observes one tile of kTileW x kTileH agents at a time, one agent per thread.
constexpr int kTileW = 32, kTileH = 8;
static_assert(kTileW * kTileH == kThreads, "one agent per thread");
constexpr int kMaxK = 25;                      // K = sum5(sum5(c)): 25 cells counted with multiplicity
constexpr int kCensus = 2 * 5 * (kMaxK + 1);   // census[sigma][m][K]
constexpr int kBondCD = kCensus;               // bond_cd[K_C - K_D + 25]
constexpr int kBondCC = kBondCD + 2 * kMaxK + 1;
constexpr int kBondDD = kBondCC + kMaxK + 1;
constexpr int kSlots = kBondDD + kMaxK + 1;
static_assert(kSlots == SPGG_PAYOFF_SLOTS && kBondCD == SPGG_PAYOFF_BOND_CD && kBondCC == SPGG_PAYOFF_BOND_CC &&
                  kBondDD == SPGG_PAYOFF_BOND_DD,
              "the row layout of spgg_abi.h");
// Workgroups per replica: every one adds to the replica's row, so few enough that the same-address
// atomics do not queue, enough that a batch of few replicas fills the device (spgg_policy.h's rule,
// one-tile workgroups queued on a replica's row).
constexpr int groups_per_replica(int tiles, int n_rep) {
  int g = (2048 + n_rep - 1) / n_rep;
  g = g < 64 ? 64 : g > 512 ? 512 : g;
  return tiles < g ? tiles : g;
}

// ---- pair sums -----------------------------------------------------------------------------
constexpr int kCellsPerDword = 4;   // one dword holds 4 cells of a row, cell x at byte x & 3
constexpr int kPairThreads = 1024;
constexpr int kPairWaves = kPairThreads / 64;
// LDS instances: a wave owns one (direction, distance) pair, so a workgroup owns this many distances.
constexpr int kDistPerGroup = kPairWaves / 2;
// Rows a wave loads before it stores the first of them to LDS (loads in flight per wave).
constexpr int kStageDepth = 4;

// The staged lattice is all the LDS the LDS instances declare, as in spgg_reputation.h: L rows of
// ceil(L / 4) dwords of the bytes K | c << 5, the bytes beyond a row's cells zero.
constexpr int kSmallDwords = 65536 / 4;           // 64 KiB: sides up to 256
constexpr int kFullDwords = 163840 / 4;           // the 160 KiB one gfx950 workgroup may declare

constexpr int row_dwords(int L) { return (L + kCellsPerDword - 1) / kCellsPerDword; }
constexpr long long lattice_dwords(int L) { return (long long)L * row_dwords(L); }   // non-decreasing in L

// Lane partials are int32.  KK: one dot of four products K K' is at most 4 * 25^2 = 2500.  CK: a
// dword pair adds two dots of four products c K', at most 2 * 4 * 25 = 200.  CC: at most 4.  So a lane
// may add up kMaxLaneDots dword pairs.
constexpr long long kDotMax = 4ll * kMaxK * kMaxK;
static_assert(kDotMax >= 2 * 4ll * kMaxK && kDotMax >= 4, "KK bounds the three sums");
constexpr long long kMaxLaneDots = ((1ll << 31) - 1) / kDotMax;   // 858,993
static_assert(kMaxLaneDots * kDotMax < (1ll << 31) && (kMaxLaneDots + 1) * kDotMax >= (1ll << 31), "the int32 lane bound");

// Dword pairs one lane adds up: the work split of spgg_reputation.h.
constexpr long long lane_dots_lds(int L) {
  const long long W = row_dwords(L), cols = (lattice_dwords(L) + 63) / 64;
  const long long rows = W <= 64 ? (L + 64 / W - 1) / (64 / W) : L * ((W + 63) / 64);
  return rows > cols ? rows : cols;
}
constexpr long long lane_dots_global(int L) {   // non-decreasing in L
  return (long long)((L + kPairWaves - 1) / kPairWaves) * ((row_dwords(L) + 63) / 64);
}

constexpr int max_lds_side() {
  int L = 1;
  while (lattice_dwords(L + 1) <= kFullDwords) ++L;
  return L;
}
// Largest side of the LDS instances: 404 rows of 101 dwords = 163,216 B.
constexpr int kMaxLdsSide = max_lds_side();
static_assert(kMaxLdsSide == 404, "the side stated in spgg_abi.h");
static_assert(lane_dots_lds(kMaxLdsSide) <= kMaxLaneDots, "LDS instances: lane partials fit int32");

// Largest lattice side (spgg_payoff_pairs_max_side): the largest L with L * L < 2^31 (cell indices
// fit int32); the lane partials of the global instance allow more (lane_dots_global(46340) =
// 2897 * 182 = 527,254).
constexpr int kMaxSide = 46340;
static_assert((long long)kMaxSide * kMaxSide < (1ll << 31) && (long long)(kMaxSide + 1) * (kMaxSide + 1) >= (1ll << 31),
              "cell indices fit int32");
static_assert(lane_dots_global(kMaxSide) <= kMaxLaneDots, "global instance: lane partials fit int32");
static_assert(kMaxSide >= 1000, "cfg5 (L = 1000) must be supported");

// int64 values of one pair-sum row: sum K, sum c, then (KK, CK, CC) for d = 0 .. max_d along rows,
// then along columns.
constexpr int pairs_width(int max_d) { return 2 + 6 * (max_d + 1); }

// Enqueue the census of iteration t (absorbed replicas: of their absorbing iteration) on `s`: a
// launch that zeroes each replica's kSlots counts, then one whose workgroups take the replica's
// tiles, write the plane byte (K | sigma << 5 | m << 6) & 0xff (plane may be null) and add census
// and bonds.  out_stride >= kSlots (caller checks).
void launch_census(const spgg_obs::Lattices& lat, int t, uint8_t* plane, int32_t* out, int64_t out_stride, hipStream_t s);

// Enqueue the pair sums of the plane a census launch wrote: replica k's pairs_width(max_d) values at
// out + k*out_stride.  1 <= L <= kMaxSide and 0 <= max_d <= L / 2 (caller checks).
void launch_pairs(const spgg_obs::Lattices& lat, int max_d, const uint8_t* plane, long long* out, int64_t out_stride,
                  hipStream_t s);

}  // namespace spgg_pf
