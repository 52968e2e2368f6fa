// spgg_correlations.hip — cooperator pair counts of a strategy plane at every distance up to
// max_d, along rows and along columns (its own object, like spgg_clusters.hip).
//
// Replaces: nothing in the reference.
//
// With c[y][x] = 1 for a cooperator (bit 0 of S clear; bits 1-4 are the step's bookkeeping) on
// the periodic lattice,
//   rows[d] = sum_yx c[y][x] & c[y][(x + d) % L]      cols[d] = sum_yx c[y][x] & c[(y + d) % L][x]
//
// Layout.  A workgroup holds the replica's plane in LDS one bit per cell: row y is W = ceil(L/32)
// words at bits[y*W ..], cell x at bit x & 31 of word x >> 5, the last word's bits >= L zero.
//
// Work split.  Grid (slice of kDistPerGroup distances) x (replica).  Every workgroup packs the
// plane for itself (n bytes that L2 serves), then each of its 16 waves owns one (direction,
// distance) pair: the wave sums popcounts over all L*W words, reduces across its lanes and
// lane 0 stores the count.  No count is shared between waves or workgroups: no atomics, one
// barrier (after the pack), every loop bound fixed by L and max_d.  Lattices of at most
// kSmallWords words run the instance that declares 8 KiB, so their workgroups share a CU; the
// other instance declares all 160 KiB (one workgroup per CU).
//
// Columns: popcount(bits[i] & bits[(i + d*W) mod L*W]).  Rows: popcount(row[w] & rot[w]), where
// rot is the row rotated as an L-bit cyclic string: rot[w] starts at bit s = (32 w + d) mod L,
// takes bits s .. of the row (two words funnelled) and, where the L - s bits left before the
// wrap are fewer than 32, continues with word 0 shifted up.  A word has at most L - 32 w <= L
// valid cells, so its window wraps at most once; bits of rot[w] beyond the valid cells are
// arbitrary and meet the zero padding of row[w].
#include "spgg_correlations.h"

namespace spgg_co {
namespace {

using namespace spgg_obs;

// the value of the lane a DPP control selects (every lane active: the callers' loops are wave-uniform)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, false);
}

template <int kCapWords>
__global__ __launch_bounds__(kThreads) void spgg_correlations_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter,
    int L, int t, int max_d, int32_t* __restrict__ out, long long out_stride) {
  __shared__ uint32_t bits[kCapWords];

  const int W = row_words(L), words = L * W;
  if (L < 1 || words > kCapWords) return;   // (the host refuses these: spgg_correlations)
  const int rep = blockIdx.y;
  const int n = L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // replica planes are n bytes apart: for odd L not 4-byte aligned
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;

  // pack: a wave takes 256 cells of a row at a time, a lane 4 of them (one unaligned 4-byte
  // load, single bytes at the row's end), 8 lanes make a word; kPackDepth rows per trip, their
  // loads issued before the first is packed (a trip is a round trip to L2 or beyond otherwise)
  const int chunks = (L + 255) >> 8;
  for (int y0 = wave; y0 < L; y0 += kWaves * kPackDepth) {   // wave-uniform, like ch and u
    for (int ch = 0; ch < chunks; ++ch) {
      const int x = ch * 256 + 4 * lane;
      uint32_t q[kPackDepth];
#pragma unroll
      for (int u = 0; u < kPackDepth; ++u) {
        q[u] = 0x01010101u;   // cells beyond the row count as defectors: zero bits
        const int y = y0 + u * kWaves;
        if (y >= L) continue;
        const uint8_t* p = plane + (size_t)y * L + x;
        if (x + 4 <= L) {
          __builtin_memcpy(&q[u], p, 4);
        } else {
          for (int j = 0; j < 4; ++j)
            if (x + j < L) q[u] = (q[u] & ~(0xffu << (8 * j))) | ((uint32_t)p[j] << (8 * j));
        }
      }
      const int w = ch * 8 + (lane >> 3);
#pragma unroll
      for (int u = 0; u < kPackDepth; ++u) {
        const int y = y0 + u * kWaves;
        if (y >= L) break;
        const uint32_t c = ~q[u] & 0x01010101u;   // bit 0 only: 0 = cooperator
        // bits 0, 8, 16, 24 -> a nibble: the 16 partial products of this multiplier land on 16
        // different bits (no carry), bit 8 i of c on bit 21 + i
        uint32_t v = (((c * 0x00204081u) >> 21) & 0xfu) << (4 * (lane & 7));
        v |= dpp_lane<0xB1>(v);    // quad_perm [1,0,3,2]: lane ^ 1
        v |= dpp_lane<0x4E>(v);    // quad_perm [2,3,0,1]: lane ^ 2
        v |= dpp_lane<0x141>(v);   // row_half_mirror: the other quad of the 8 lanes (quads are uniform by now)
        if ((lane & 7) == 0 && w < W) bits[y * W + w] = v;
      }
    }
  }
  __syncthreads();

  const int d = blockIdx.x * kDistPerGroup + (wave >> 1);
  if (d > max_d) return;   // wave-uniform; no barrier follows
  uint32_t cnt = 0u;
  if (wave & 1) {   // columns
    const int shift = d * W;   // <= words / 2
#pragma unroll 4   // independent LDS reads in flight: a trip is a read latency otherwise
    for (int i = lane; i < words; i += 64) {
      int j = i + shift;
      if (j >= words) j -= words;
      cnt += (uint32_t)__popc(bits[i] & bits[j]);
    }
  } else {          // rows
    // a lane keeps its word index w over the rows, so the window of rot[w] -- start bit s, the
    // words a and a + 1 it is funnelled from, the k bits before the wrap -- is computed once;
    // 64 / W rows per trip (W <= 36), the lanes beyond them idle
    const int per_trip = 64 / W;
    const int w = lane % W, y0 = lane / W;
    int s = kWordBits * w + d;   // < 2 L
    if (s >= L) s -= L;
    const int a = s >> 5, sh = s & 31;
    const bool two = a + 1 < W;  // (the word after the row's last reads as 0)
    const int k = L - s;         // >= 1
    const bool wraps = k < kWordBits;
    const uint32_t keep = wraps ? (1u << k) - 1u : ~0u;
    if (y0 < per_trip) {
#pragma unroll 4
      for (int y = y0; y < L; y += per_trip) {
        const uint32_t* row = bits + y * W;
        const uint32_t lo = row[a], hi = two ? row[a + 1] : 0u;
        uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & keep;
        if (wraps) v |= row[0] << k;
        cnt += (uint32_t)__popc(row[w] & v);
      }
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0) out[(long long)rep * out_stride + (wave & 1) * (max_d + 1) + d] = (int32_t)cnt;
}

}  // namespace

void launch(const spgg_obs::Lattices& lat, int t, int max_d, int32_t* out, int64_t out_stride, hipStream_t s) {
  const dim3 grid((max_d + kDistPerGroup) / kDistPerGroup, lat.n_rep);
  const auto kernel = lattice_words(lat.L) <= kSmallWords ? spgg_correlations_kernel<kSmallWords>
                                                          : spgg_correlations_kernel<kFullWords>;
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, lat.S0, lat.S1, lat.stop_iter, lat.L, t, max_d, out,
                     (long long)out_stride);
}

}  // namespace spgg_co
