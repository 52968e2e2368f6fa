// spgg_pair_map.hip — the 2-D pair map of two one-bit fields of a strategy plane: for dy = 0 .. D and
// dx = -D .. D the count of cells with A set whose partner (dx, dy) away has B set (its own object,
// like spgg_correlations.hip).
//
// Replaces: nothing in the reference.
//
//   map[dy][dx + D] = sum_yx A[y][x] & B[(y + dy) % L][(x + dx) % L]
//
// Two launches.
//
// Pack.  Grid (band) x (replica); a wave takes 64 consecutive bits of one packed row at a time: a lane
// reads the S byte of its cell (consecutive lanes, consecutive bytes), forms the field's bit and one
// ballot makes the two words, which lanes 0 and 1 store.  Field A goes out as plain bit rows, field B
// as extended rows (spgg_pair_map.h): bit j of row y is B[y][(j - D) mod L], so that the partners of
// the 32 cells of word w at dx = -D + 32 b + j are the 32 bits from bit 32 (w + b) + j of the
// extended row -- no wrap logic is left for the count.
//
// Count.  Grid (slice of kCountWaves waves) x (replica).  A wave owns one dy and one block b of 32
// consecutive dx outright, over every row.  A lane keeps its word index w over the rows (64 / W rows
// per trip for W <= 64, the lanes beyond them idle) and holds 32 int32 accumulators; per (y, w) it
// reads the word of A[y] and the words w + b, w + b + 1 of the extended row (y + dy) % L, then for
// j = 0 .. 31: funnel by j (a constant: v_alignbit_b32), AND, accumulating popcount.  The padding
// bits of A are zero, so whatever the window holds opposite them is not counted.  At the end the
// wave reduces its 32 sums across the lanes and lanes 0 .. 31 store them (the columns beyond 2 D of
// the last block are dropped).  No count is shared between waves: no atomics; the staging barrier is
// the only one; every loop bound is fixed by L and D.  Where both packed planes fit, a workgroup
// copies them to LDS first (the 16 KiB and the 160 KiB instance); above that the lanes read the
// workspace, which L2 holds.
#include "spgg_pair_map.h"

namespace spgg_pm {
namespace {

using namespace spgg_obs;

// the field's bit of an S byte: bits 0 and 3 alone are read; `first`: the observed state is S_1, which
// has no previous iteration
__device__ __forceinline__ bool field_bit(uint32_t s, int field, bool first) {
  if (field == SPGG_FIELD_COOP) return (s & 1u) == 0u;
  return !first && (((s ^ (s >> 3)) & 1u) != 0u);
}

__global__ __launch_bounds__(kPackThreads) void spgg_pair_map_pack_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L, int t,
    int field_a, int field_b, int D, uint32_t* __restrict__ work, long long words_per_rep) {
  const int rep = blockIdx.y;
  const size_t n = (size_t)L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  const bool first = observed_iter(stop_iter, rep, t) == 1;
  const int W = row_words(L), WE = ext_words(L, D);
  const int CA = (W + 1) >> 1, CE = (WE + 1) >> 1;   // 64-bit chunks of a row of A, of an extended row
  uint32_t* pa = work + (size_t)rep * (size_t)words_per_rep;
  uint32_t* pe = pa + (size_t)L * W;
  const int items = L * (CA + CE);
  for (int i = blockIdx.x * kPackWaves + wave; i < items; i += gridDim.x * kPackWaves) {   // wave-uniform
    const int y = i / (CA + CE), r = i - y * (CA + CE);
    const bool ext = r >= CA;
    const int c = ext ? r - CA : r;
    const int j = 64 * c + lane;
    int x = ext ? j - D : j;   // -L / 2 .. < 3 L / 2
    if (x < 0) x += L;
    else if (x >= L) x -= L;
    const bool valid = ext ? j < L + 2 * D : j < L;
    bool bit = false;
    if (valid) bit = field_bit(sp[(size_t)y * L + x], ext ? field_b : field_a, first);
    const unsigned long long m = __ballot(bit);
    const int words = ext ? WE : W, word = 2 * c + lane;
    if (lane < 2 && word < words) (ext ? pe : pa)[(size_t)y * words + word] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
}

template <int kCapWords>
__global__ __launch_bounds__(kCountThreads) void spgg_pair_map_count_kernel(const uint32_t* __restrict__ work,
                                                                            long long words_per_rep, int L, int D,
                                                                            int32_t* __restrict__ out,
                                                                            long long out_stride) {
  __shared__ uint32_t staged[kCapWords ? kCapWords : 1];

  const int W = row_words(L), WE = ext_words(L, D);
  const int rep = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t* ga = work + (size_t)rep * (size_t)words_per_rep;
  const uint32_t *A, *E;
  if constexpr (kCapWords > 0) {
    const int words = L * (W + WE);
    if (words > kCapWords) return;   // (the host picks the instance: launch)
#pragma unroll 4
    for (int i = threadIdx.x; i < words; i += kCountThreads) staged[i] = ga[i];
    __syncthreads();
    A = staged;
    E = staged + L * W;
  } else {
    A = ga;
    E = ga + (size_t)L * W;
  }

  const int nblk = dx_blocks(D);
  const int q = blockIdx.x * kCountWaves + wave;
  if (q >= (D + 1) * nblk) return;   // wave-uniform; no barrier follows
  const int dy = q / nblk, b = q - dy * nblk;

  int acc[kBlock];
#pragma unroll
  for (int j = 0; j < kBlock; ++j) acc[j] = 0;
  const int per_trip = W <= 64 ? 64 / W : 1;
  const int w0 = W <= 64 ? lane % W : lane, y0 = W <= 64 ? lane / W : 0;
  if (y0 < per_trip) {
    for (int w = w0; w < W; w += 64) {
#pragma unroll 4
      for (int y = y0; y < L; y += per_trip) {
        int y2 = y + dy;   // < 2 L
        if (y2 >= L) y2 -= L;
        const uint32_t a = A[(size_t)y * W + w];
        const uint32_t* e = E + (size_t)y2 * WE + (w + b);
        const uint32_t lo = e[0], hi = e[1];
#pragma unroll
        for (int j = 0; j < kBlock; ++j) acc[j] += __builtin_popcount(a & __builtin_amdgcn_alignbit(hi, lo, (uint32_t)j));
      }
    }
  }
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kBlock; ++j) {
    const int total = wave_sum(acc[j]);
    if (lane == j) mine = total;
  }
  const int col = kBlock * b + lane;
  if (lane < kBlock && col <= 2 * D) out[(long long)rep * out_stride + (long long)dy * (2 * D + 1) + col] = mine;
}

}  // namespace

void launch(const spgg_obs::Lattices& lat, int t, int field_a, int field_b, int max_d, uint32_t* work, int32_t* out,
            int64_t out_stride, hipStream_t s) {
  const int L = lat.L, W = row_words(L), WE = ext_words(L, max_d);
  const long long per_rep = plane_words(L, max_d);
  const long long items = (long long)L * ((W + 1) / 2 + (WE + 1) / 2);
  // about four chunks per wave, up to some 8192 workgroups in all: a chunk is one round trip to the S
  // plane, so one lattice alone is spread over many more workgroups than each of a batch's
  long long bands = (items + 4 * kPackWaves - 1) / (4 * kPackWaves), most = 8192 / lat.n_rep;
  most = most < 64 ? 64 : most > 2048 ? 2048 : most;
  bands = bands < 1 ? 1 : bands > most ? most : bands;
  hipLaunchKernelGGL(spgg_pair_map_pack_kernel, dim3((unsigned)bands, lat.n_rep), dim3(kPackThreads), 0, s, lat.S0, lat.S1,
                     lat.stop_iter, L, t, field_a, field_b, max_d, work, per_rep);
  const long long waves = (long long)(max_d + 1) * dx_blocks(max_d);
  const dim3 grid((unsigned)((waves + kCountWaves - 1) / kCountWaves), lat.n_rep);
  auto kernel = spgg_pair_map_count_kernel<0>;
  if (per_rep <= kSmallWords) kernel = spgg_pair_map_count_kernel<kSmallWords>;
  else if (per_rep <= kFullWords) kernel = spgg_pair_map_count_kernel<kFullWords>;
  hipLaunchKernelGGL(kernel, grid, dim3(kCountThreads), 0, s, (const uint32_t*)work, per_rep, L, max_d, out,
                     (long long)out_stride);
}

}  // namespace spgg_pm
