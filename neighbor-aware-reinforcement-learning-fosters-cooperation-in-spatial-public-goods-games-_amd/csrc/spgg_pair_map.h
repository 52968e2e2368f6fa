// spgg_pair_map.h — the 2-D pair map of two one-bit fields of S_t (spgg_pair_map.hip): for every
// displacement (dx, dy), dy = 0 .. D, dx = -D .. D, the number of cells (y, x) with A[y][x] set and
// B[(y + dy) % L][(x + dx) % L] set.  The fields (spgg_abi.h): the cooperators of S_t, and the agents
// that changed strategy in iteration t - 1 (bit 0 ^ bit 3 of the S byte).  Nothing in the reference
// computes these.  The kernels read S_t in place; no workgroup waits for another and every loop bound
// is known at launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_pm {

constexpr int kFields = 2;
static_assert(SPGG_FIELD_COOP == 0 && SPGG_FIELD_FLIP == 1, "the field table of spgg_abi.h");

constexpr int kWordBits = 32;
// A wave of the count launch owns one dy and kBlock consecutive dx: one int32 accumulator per dx and lane.
constexpr int kBlock = 32;

constexpr int kPackThreads = 256;
constexpr int kPackWaves = kPackThreads / 64;
constexpr int kCountThreads = 512;
constexpr int kCountWaves = kCountThreads / 64;

// ---- the packed planes: the workspace of one replica ---------------------------------------
// Field A as plain bit rows: L rows of row_words(L) words, cell x at bit x & 31 of word x >> 5, the
// bits past L zero.
constexpr int row_words(int L) { return (L + kWordBits - 1) / kWordBits; }
// Field B as extended rows: bit j of row y is B[y][(j - D) mod L] for j = 0 .. L + 2 D - 1, zero up to
// whole words, and one more zero word: the window of word w at displacement dx = -D + 32 b + j is
// the 32 bits from bit 32 (w + b) + j, two adjacent words funnelled by j, and the last block of the
// last word reads word row_words(L) + (2 D) / 32 <= ext_words - 1.
constexpr int ext_words(int L, int D) { return (L + 2 * D + kWordBits - 1) / kWordBits + 1; }
constexpr long long plane_words(int L, int D) { return (long long)L * (row_words(L) + ext_words(L, D)); }
// dx blocks of one dy
constexpr int dx_blocks(int D) { return (2 * D + kBlock) / kBlock; }   // ceil((2 D + 1) / 32)
static_assert(dx_blocks(0) == 1 && dx_blocks(15) == 1 && dx_blocks(16) == 2 && dx_blocks(32) == 3 && dx_blocks(500) == 32, "");
static_assert(row_words(1000) + (2 * 500) / kWordBits <= ext_words(1000, 500) - 1, "the last window's second word");
static_assert(plane_words(1000, 500) * 4 == 384000, "cfg5 at D = 500: 384 KB per replica");

// The count launch stages both packed planes in LDS where they fit: the instance that declares
// 16 KiB (its workgroups share a CU), the one that declares all 160 KiB a gfx950 workgroup may, and
// above that the instance that reads the workspace itself (L2-resident).
constexpr int kSmallWords = 16384 / 4;
constexpr int kFullWords = 163840 / 4;

constexpr int map_width(int D) { return (D + 1) * (2 * D + 1); }

// ---- work and its cap ----------------------------------------------------------------------
// The work of one call, in word blocks: a word block is one word of A against one window block of B,
// kBlock funnel / AND / popcount triples.  Every wave of the count launch walks the L * row_words(L)
// words of A once, and there are n_rep * (D + 1) * dx_blocks(D) waves:
//   work = n_rep * (D + 1) * ceil((2 D + 1) / 32) * L * ceil(L / 32)
// (saturating at INT64_MAX).  cfg3 (105 x L = 200) at D = 32: 14.6e6; cfg5 (1 x L = 1000) at D = 500:
// 513e6.
constexpr int64_t kWorkMax = INT64_MAX;
inline int64_t work(int L, int n_rep, int D) {
  unsigned __int128 w = (unsigned __int128)n_rep * (unsigned)(D + 1) * (unsigned)dx_blocks(D);
  w *= (unsigned __int128)L * (unsigned)row_words(L);
  return w > (unsigned __int128)kWorkMax ? kWorkMax : (int64_t)w;
}
// The cap: a record must not stall a turn for seconds.  One call at cfg5 with D = 500 (both launches;
// the pack is a hundredth of it) was measured at 1.47 ms on a whole MI355X, 3.48e11 word blocks per
// second (the best rate measured; calls of fewer waves run below it, so the cap
// bounds the work, not the time, of a call that does not fill the device); the largest accepted call
// is a quarter of a second at that rate.
constexpr int64_t kMeasuredRate = 348000000000ll;   // word blocks / s
constexpr int64_t kWorkCap = kMeasuredRate / 4;
static_assert(kWorkCap == SPGG_PAIR_MAP_WORK_CAP, "the cap stated in spgg_abi.h");

// Enqueue the pack launch and the count launch of iteration t (absorbed replicas: of their absorbing
// iteration) on `s`: replica k's packed planes at work + k * plane_words(L, max_d), its
// map_width(max_d) counts at out + k * out_stride.  0 <= max_d <= L / 2, the fields in the table,
// out_stride >= map_width(max_d) and work(..) <= kWorkCap (caller checks).
void launch(const spgg_obs::Lattices& lat, int t, int field_a, int field_b, int max_d, uint32_t* work, int32_t* out,
            int64_t out_stride, hipStream_t s);

}  // namespace spgg_pm
