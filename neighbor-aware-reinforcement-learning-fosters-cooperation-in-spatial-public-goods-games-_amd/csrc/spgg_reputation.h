// spgg_reputation.h — the reputation field's record (spgg_reputation.hip): the joint histogram
// strategy x reputation bin, and the pair sums of the int8 reputation plane at every distance.
//
// Nothing in the reference computes these on the device (its rep_hist_* datasets are host
// np.histogram calls on at most nine snapshots).  Both kernels read R_t and S_t in place; no
// workgroup waits for another and every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_rp {

// ---- histogram ---------------------------------------------------------------------------
constexpr int kMaxBins = 256;
constexpr int kHistThreads = 256;
constexpr int kHistWaves = kHistThreads / 64;
static_assert(kHistThreads == 256, "one thread bins each of the 256 int8 levels");
// Cells one workgroup bins (16 per thread): cfg5's 10^6 cells make 245 workgroups.
constexpr int kHistCells = 4096;

// ---- pair sums ---------------------------------------------------------------------------
constexpr int kCellsPerDword = 4;   // one dword holds 4 cells of a row, cell x at byte x & 3
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// LDS instances: a wave owns one (direction, distance) pair, so a workgroup owns this many distances.
constexpr int kDistPerGroup = kWaves / 2;
// Rows a wave loads before it stores the first of them to LDS (loads in flight per wave).
constexpr int kStageDepth = 4;

// The staged lattice is all the LDS the LDS instances declare: L rows of ceil(L / 4) dwords, the
// bytes beyond a row's cells zero.  Lattices of at most kSmallDwords dwords run the instance that
// declares 64 KiB (two workgroups of 16 waves fill a CU's 32 wave slots), lattices up to
// kFullDwords the one that declares all 160 KiB; larger ones run the instance that declares no
// lattice at all and reads the plane (L2-resident: 1 MB at L = 1000) from global memory.
constexpr int kSmallDwords = 65536 / 4;           // 64 KiB: sides up to 256
constexpr int kFullDwords = 163840 / 4;           // the 160 KiB one gfx950 workgroup may declare

constexpr int row_dwords(int L) { return (L + kCellsPerDword - 1) / kCellsPerDword; }
constexpr long long lattice_dwords(int L) { return (long long)L * row_dwords(L); }   // non-decreasing in L

// Lane partials are int32.  One dot of four int8 products is at most 4 * 128^2 = 2^16 in
// magnitude, so a lane may add up kMaxLaneDots = 2^15 - 1 of them: 32767 * 65536 < 2^31.
constexpr long long kDotMax = 4ll * 128 * 128;
constexpr long long kMaxLaneDots = ((1ll << 31) - 1) / kDotMax;   // 32767
static_assert(kMaxLaneDots * kDotMax < (1ll << 31) && (kMaxLaneDots + 1) * kDotMax >= (1ll << 31), "the int32 lane bound");

// Dots one lane adds up.  LDS instances: a wave sums one pair over all L * W dwords.  Columns:
// lane l the dwords l, l + 64, ..  Rows: with W <= 64 a lane keeps one dword index and takes every
// (64 / W)-th row, else it takes the dwords l, l + 64, .. of every row.
constexpr long long lane_dots_lds(int L) {
  const long long W = row_dwords(L), cols = (lattice_dwords(L) + 63) / 64;
  const long long rows = W <= 64 ? (L + 64 / W - 1) / (64 / W) : L * ((W + 63) / 64);
  return rows > cols ? rows : cols;
}
// Global instance: a workgroup sums one pair, wave v the rows v, v + 16, .., lane l the dwords
// l, l + 64, .. of each.
constexpr long long lane_dots_global(int L) {
  return (long long)((L + kWaves - 1) / kWaves) * ((row_dwords(L) + 63) / 64);
}

constexpr int max_lds_side() {
  int L = 1;
  while (lattice_dwords(L + 1) <= kFullDwords) ++L;
  return L;
}
// Largest side of the LDS instances: 404 rows of 101 dwords = 163,216 B.
constexpr int kMaxLdsSide = max_lds_side();
static_assert(lane_dots_lds(kMaxLdsSide) <= kMaxLaneDots, "LDS instances: lane partials fit int32");

constexpr int max_side() {
  int L = kMaxLdsSide;
  while (lane_dots_global(L + 1) <= kMaxLaneDots) ++L;
  return L;
}
// Largest lattice side (spgg_reputation_max_side): 11520, set by the int32 lane partials of the
// global instance (lane_dots_global(11520) = 720 * 45 = 32,400; (11521) = 721 * 46 = 33,166).
constexpr int kMaxSide = max_side();
static_assert(kMaxSide == 11520, "the side stated above and in spgg_abi.h");
static_assert(kMaxSide >= 1000, "cfg5 (L = 1000) must be supported");
static_assert((long long)kMaxSide * kMaxSide < (1ll << 31), "cell indices fit int32");

// Enqueue the joint histogram of every replica's (S, R) planes of iteration t (absorbed replicas:
// of their absorbing iteration) on `s`: a launch that zeroes each replica's 2 * bins counts, then
// one that adds into them.  rep_int8: R holds int8 multiples of params[rep].rep_unit, else f64.
// 1 <= bins <= kMaxBins, out_stride >= 2 * bins (caller checks).
void launch_hist(const spgg_obs::Lattices& lat, const void* R0, const void* R1, bool rep_int8,
                 const spgg_rep_params* params, int t, int bins, const double* edges, int32_t* out,
                 int64_t out_stride, hipStream_t s);

// Enqueue the pair sums of every replica's int8 R plane of iteration t on `s`: replica k's sum,
// rows[0..max_d], cols[0..max_d] at out + k*out_stride.  1 <= L <= kMaxSide and
// 0 <= max_d <= L / 2 (caller checks).
void launch_pairs(const spgg_obs::Lattices& lat, const int8_t* R0, const int8_t* R1, int t, int max_d, long long* out,
                  int64_t out_stride, hipStream_t s);

}  // namespace spgg_rp
