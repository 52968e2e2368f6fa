// spgg_reputation.hip — the reputation field's record: the joint histogram strategy x reputation
// bin of (S_t, R_t), and the pair sums of the int8 reputation plane at every distance up to
// max_d along rows and along columns (its own object, like spgg_correlations.hip).
//
// Replaces: nothing in the reference on the device; with the reference's edges the histogram's
// two strategy rows add up to its rep_hist_* datasets (np.histogram, spgg.py:399).
//
// Histogram.  Grid (chunk of kHistCells cells) x (replica).  A workgroup holds the replica's
// edges in LDS and one histogram per wave; a cell's bin is the i with edges[i] <= x <
// edges[i + 1] (x == edges[bins]: the last bin; outside: none), found by a bisection of fixed
// depth.  On the int8 path x = k * rep_unit takes 256 values, so the workgroup bins the 256 levels
// once and a cell is a table look-up.  The workgroup then adds its non-zero counts to the
// replica's row with int32 atomics (exact, order-free); a launch ahead of it zeroes the rows.
//
// Pair sums.  With k[y][x] the stored byte on the periodic lattice,
//   sum = sum_yx k[y][x]   rows[d] = sum_yx k[y][x] k[y][(x + d) % L]   cols[d] = sum_yx k[y][x] k[(y + d) % L][x]
// by the int8 dot instruction (v_dot4c_i32_i8) on dwords of four cells.
//
// LDS instances (L <= kMaxLdsSide).  Layout: row y is W = ceil(L/4) dwords at lat[y*W ..], cell x
// at byte x & 3 of dword x >> 2, the last dword's bytes >= L zero.  Work split as in
// spgg_correlations: grid (slice of kDistPerGroup distances) x (replica); every workgroup stages
// the plane for itself (n bytes that L2 serves), then each of its 16 waves owns one (direction,
// distance) pair, sums the dots over all L*W dwords in int32 lane partials (bound:
// spgg_reputation.h), reduces them in int64 across its lanes and lane 0 stores.  No atomics, one
// barrier (after the staging).
//   Columns: dot(lat[i], lat[(i + d*W) mod L*W]) -- aligned, the padding of both is zero.
//   Rows: dot(row[w], rot[w]), rot the row rotated as an L-byte cyclic string: rot[w] starts at
//   byte s = (4 w + d) mod L, takes bytes s .. of the row (two aligned dwords through
//   v_alignbyte_b32; the dword after the row's last reads as 0) and, where the k = L - s bytes left
//   before the wrap are fewer than 4, continues with dword 0 shifted up by k bytes.  A dword has at
//   most L - 4 w <= L valid cells, so its window wraps at most once; bytes of rot[w] beyond the
//   valid cells are arbitrary and meet the zero padding of row[w].
//
// Global instance (kMaxLdsSide < L <= kMaxSide).  Grid (2 * (max_d + 1) pairs) x (replica): a
// workgroup owns one pair, wave v the rows v, v + 16, .., and reads both dwords of a dot from the
// plane in global memory by unaligned 4-byte loads (single bytes at a row's end and across the
// wrap); the 16 wave sums meet in LDS and thread 0 stores.
#include "spgg_reputation.h"

namespace spgg_rp {
namespace {

using namespace spgg_obs;

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
}

// ---- histogram ---------------------------------------------------------------------------

__global__ __launch_bounds__(kHistThreads) void spgg_reputation_zero_kernel(int32_t* __restrict__ out,
                                                                            long long out_stride, int count) {
  for (int i = threadIdx.x; i < count; i += kHistThreads) out[(long long)blockIdx.x * out_stride + i] = 0;
}

// the bin of x among e[0 .. bins] (ascending), -1 if none; 9 halvings cover the 258 outcomes
__device__ __forceinline__ int bin_of(const double* e, int bins, double x) {
  int lo = 0, hi = bins + 1;   // lo ends as the number of edges <= x
#pragma unroll
  for (int it = 0; it < 9; ++it) {
    if (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
  }
  if (lo == 0) return -1;
  if (lo == bins + 1) return x == e[bins] ? bins - 1 : -1;
  return lo - 1;
}

template <bool RQ>
__global__ __launch_bounds__(kHistThreads) void spgg_reputation_hist_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const void* __restrict__ R0,
    const void* __restrict__ R1, const spgg_rep_params* __restrict__ params, const int32_t* __restrict__ stop_iter,
    int L, int t, int bins, const double* __restrict__ edges, int32_t* __restrict__ out, long long out_stride) {
  __shared__ double e[kMaxBins + 1];
  __shared__ uint32_t h[kHistWaves][2 * kMaxBins];
  __shared__ int16_t level_bin[256];

  if (bins < 1 || bins > kMaxBins) return;   // (the host refuses these: spgg_reputation_hist)
  const int rep = blockIdx.y;
  const int n = L * L;
  const int tid = threadIdx.x, wave = tid >> 6;
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;   // n bytes apart: unaligned for odd L
  const void* rv = observed_plane(R0, R1, stop_iter, rep, t);                        // R_t lies where S_t does

  for (int i = tid; i <= bins; i += kHistThreads) e[i] = edges[(size_t)rep * (bins + 1) + i];
  for (int i = tid; i < kHistWaves * 2 * kMaxBins; i += kHistThreads) (&h[0][0])[i] = 0u;
  __syncthreads();
  uint32_t* hw = h[wave];
  const int base = blockIdx.x * kHistCells;

  if constexpr (RQ) {
    // x = k * rep_unit is an exact product; kHistThreads == the 256 levels
    level_bin[tid] = (int16_t)bin_of(e, bins, (double)(tid - 128) * params[rep].rep_unit);
    __syncthreads();
    const int8_t* rp = (const int8_t*)rv + (size_t)rep * n;
#pragma unroll
    for (int j = 0; j < kHistCells / (4 * kHistThreads); ++j) {
      const int i = base + (j * kHistThreads + tid) * 4;
      if (i >= n) break;
      uint32_t sq = 0u, rq = 0u;
      const int valid = min(4, n - i);
      if (valid == 4) {
        __builtin_memcpy(&sq, sp + i, 4);
        __builtin_memcpy(&rq, rp + i, 4);
      } else {
        for (int u = 0; u < valid; ++u) {
          sq |= (uint32_t)sp[i + u] << (8 * u);
          rq |= (uint32_t)(uint8_t)rp[i + u] << (8 * u);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u >= valid) break;
        const int k = (int)(int8_t)(rq >> (8 * u));
        const int b = level_bin[k + 128];
        if (b >= 0) atomicAdd(&hw[((sq >> (8 * u)) & 1u) * bins + b], 1u);   // bit 0 only: 0 = cooperator
      }
    }
  } else {
    const double* rp = (const double*)rv + (size_t)rep * n;
#pragma unroll 4
    for (int j = 0; j < kHistCells / kHistThreads; ++j) {
      const int i = base + j * kHistThreads + tid;
      if (i >= n) break;
      const int b = bin_of(e, bins, rp[i]);
      if (b >= 0) atomicAdd(&hw[(sp[i] & 1u) * bins + b], 1u);
    }
  }
  __syncthreads();
  for (int b = tid; b < 2 * bins; b += kHistThreads) {
    uint32_t c = 0u;
#pragma unroll
    for (int w = 0; w < kHistWaves; ++w) c += h[w][b];
    if (c) atomicAdd(out + (long long)rep * out_stride + b, (int32_t)c);
  }
}

// ---- pair sums: LDS instances --------------------------------------------------------------

// the dword of the cells x0 .. x0 + 3 of a row in global memory (row + x0 need not be aligned),
// the bytes beyond the row's L cells zero
__device__ __forceinline__ uint32_t load_cells(const int8_t* row, int x0, int L) {
  uint32_t q = 0u;
  if (x0 + 4 <= L) {
    __builtin_memcpy(&q, row + x0, 4);
  } else {
    for (int j = 0; j < 4; ++j)
      if (x0 + j < L) q |= (uint32_t)(uint8_t)row[x0 + j] << (8 * j);
  }
  return q;
}

template <int kCapDwords>
__global__ __launch_bounds__(kThreads) void spgg_reputation_pairs_lds_kernel(
    const int8_t* __restrict__ R0, const int8_t* __restrict__ R1, const int32_t* __restrict__ stop_iter, int L, int t,
    int max_d, long long* __restrict__ out, long long out_stride) {
  __shared__ uint32_t lat[kCapDwords];

  const int W = row_dwords(L), dwords = L * W;
  if (L < 1 || dwords > kCapDwords) return;   // (the host picks the instance: launch_pairs)
  const int rep = blockIdx.y;
  const int n = L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // replica planes are n bytes apart: for odd L not 4-byte aligned
  const int8_t* plane = observed_plane(R0, R1, stop_iter, rep, t) + (size_t)rep * n;

  // stage: a wave takes 256 cells of a row at a time, a lane 4 of them; kStageDepth rows per
  // trip, their loads issued before the first is stored
  const int chunks = (W + 63) >> 6;
  for (int y0 = wave; y0 < L; y0 += kWaves * kStageDepth) {   // wave-uniform, like ch and u
    for (int ch = 0; ch < chunks; ++ch) {
      const int w = ch * 64 + lane;
      uint32_t q[kStageDepth];
#pragma unroll
      for (int u = 0; u < kStageDepth; ++u) {
        const int y = y0 + u * kWaves;
        q[u] = (y < L && w < W) ? load_cells(plane + (size_t)y * L, 4 * w, L) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kStageDepth; ++u) {
        const int y = y0 + u * kWaves;
        if (y < L && w < W) lat[y * W + w] = q[u];
      }
    }
  }
  __syncthreads();

  const int d = blockIdx.x * kDistPerGroup + (wave >> 1);
  if (d > max_d) return;   // wave-uniform; no barrier follows
  int acc = 0, ones = 0;   // int32 lane partials: at most lane_dots_lds(L) dots each
  if (wave & 1) {   // columns
    const int shift = d * W;   // <= dwords / 2
#pragma unroll 4   // independent LDS reads in flight: a trip is a read latency otherwise
    for (int i = lane; i < dwords; i += 64) {
      int j = i + shift;
      if (j >= dwords) j -= dwords;
      acc = dot4(lat[i], lat[j], acc);
    }
  } else {          // rows
    // W <= 64: a lane keeps its dword index w over the rows, 64 / W rows per trip (the lanes
    // beyond them idle); W > 64: a lane takes the dwords lane, lane + 64, .. of every row.
    // Either way the window of rot[w] is computed once per w, outside the loop over the rows.
    const int per_trip = W <= 64 ? 64 / W : 1;
    const int w0 = W <= 64 ? lane % W : lane, y0 = W <= 64 ? lane / W : 0;
    const bool with_sum = d == 0;   // the wave of rows[0] also sums the plane
    if (y0 < per_trip) {
      for (int w = w0; w < W; w += 64) {
        int s = kCellsPerDword * w + d;   // < 2 L
        if (s >= L) s -= L;
        const int a = s >> 2;
        const uint32_t sh = (uint32_t)(s & 3);
        const int a1 = a + 1 < W ? a + 1 : a;                    // (the dword after the row's last reads as 0:
        const uint32_t two = a + 1 < W ? ~0u : 0u;               //  read a again and mask it)
        const int k = L - s;                                     // >= 1
        const bool wraps = k < kCellsPerDword;
        const uint32_t keep = wraps ? (1u << (8 * k)) - 1u : ~0u;
        const uint32_t up = wraps ? 8u * (uint32_t)k : 0u, wrap_mask = wraps ? ~0u << (8 * k) : 0u;
        // every read of a trip is unconditional, so the four of them (and those of the unrolled
        // trips) are in flight together: a read under a lane-dependent branch waits on its own
#pragma unroll 4
        for (int y = y0; y < L; y += per_trip) {
          const uint32_t* row = lat + y * W;
          const uint32_t lo = row[a], hi = row[a1] & two, first = row[0], own = row[w];
          const uint32_t v = (__builtin_amdgcn_alignbyte(hi, lo, sh) & keep) | ((first << up) & wrap_mask);
          acc = dot4(own, v, acc);
          if (with_sum) ones = dot4(own, 0x01010101u, ones);
        }
      }
    }
  }
  const long long total = wave_sum((long long)acc);
  long long* o = out + (long long)rep * out_stride;
  if (lane == 0) o[1 + (wave & 1) * (max_d + 1) + d] = total;
  if (!(wave & 1) && d == 0) {   // wave-uniform
    const long long sum = wave_sum((long long)ones);
    if (lane == 0) o[0] = sum;
  }
}

// ---- pair sums: global instance ------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void spgg_reputation_pairs_global_kernel(
    const int8_t* __restrict__ R0, const int8_t* __restrict__ R1, const int32_t* __restrict__ stop_iter, int L, int t,
    int max_d, long long* __restrict__ out, long long out_stride) {
  __shared__ long long part[2][kWaves];

  const int W = row_dwords(L);
  const int rep = blockIdx.y;
  const size_t n = (size_t)L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int8_t* plane = observed_plane(R0, R1, stop_iter, rep, t) + (size_t)rep * n;
  const bool cols = (int)blockIdx.x > max_d;               // pairs 0 .. max_d: rows, then columns
  const int d = cols ? (int)blockIdx.x - (max_d + 1) : (int)blockIdx.x;
  const bool with_sum = blockIdx.x == 0;                   // the workgroup of rows[0] also sums the plane

  int acc = 0, ones = 0;   // int32 lane partials: at most lane_dots_global(L) dots each
  for (int w = lane; w < W; w += 64) {
    const int x0 = kCellsPerDword * w;
    const int valid = min(kCellsPerDword, L - x0);
    int s = x0 + d;   // rows: the window's first cell, < 2 L
    if (s >= L) s -= L;
    const bool whole = valid == kCellsPerDword && s + kCellsPerDword <= L;   // no row end, no wrap
#pragma unroll 2
    for (int y = wave; y < L; y += kWaves) {
      const int8_t* row = plane + (size_t)y * L;
      const uint32_t own = load_cells(row, x0, L);
      uint32_t v = 0u;
      if (cols) {
        int y2 = y + d;
        if (y2 >= L) y2 -= L;
        v = load_cells(plane + (size_t)y2 * L, x0, L);
      } else if (whole) {
        __builtin_memcpy(&v, row + s, 4);
      } else {
        for (int j = 0; j < valid; ++j) {   // valid <= L: the window wraps at most once
          int x = s + j;
          if (x >= L) x -= L;
          v |= (uint32_t)(uint8_t)row[x] << (8 * j);
        }
      }
      acc = dot4(own, v, acc);
      if (with_sum) ones = dot4(own, 0x01010101u, ones);
    }
  }
  const long long total = wave_sum((long long)acc), sum = wave_sum((long long)ones);
  if (lane == 0) {
    part[0][wave] = total;
    part[1][wave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long a = 0, b = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      a += part[0][v];
      b += part[1][v];
    }
    long long* o = out + (long long)rep * out_stride;
    o[1 + (int)blockIdx.x] = a;   // rows[d] at 1 + d, cols[d] at 1 + (max_d + 1) + d
    if (with_sum) o[0] = b;
  }
}

}  // namespace

void launch_hist(const spgg_obs::Lattices& lat, const void* R0, const void* R1, bool rep_int8,
                 const spgg_rep_params* params, int t, int bins, const double* edges, int32_t* out,
                 int64_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(spgg_reputation_zero_kernel, dim3(lat.n_rep), dim3(kHistThreads), 0, s, out,
                     (long long)out_stride, 2 * bins);
  const dim3 grid((unsigned)((lat.cells() + kHistCells - 1) / kHistCells), lat.n_rep);
  const auto kernel = rep_int8 ? spgg_reputation_hist_kernel<true> : spgg_reputation_hist_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(kHistThreads), 0, s, lat.S0, lat.S1, R0, R1, params, lat.stop_iter, lat.L, t,
                     bins, edges, out, (long long)out_stride);
}

void launch_pairs(const spgg_obs::Lattices& lat, const int8_t* R0, const int8_t* R1, int t, int max_d, long long* out,
                  int64_t out_stride, hipStream_t s) {
  dim3 grid((max_d + kDistPerGroup) / kDistPerGroup, lat.n_rep);
  auto kernel = spgg_reputation_pairs_lds_kernel<kFullDwords>;
  if (lat.L > kMaxLdsSide) {
    kernel = spgg_reputation_pairs_global_kernel;
    grid.x = 2 * (max_d + 1);
  } else if (lattice_dwords(lat.L) <= kSmallDwords) {
    kernel = spgg_reputation_pairs_lds_kernel<kSmallDwords>;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, R0, R1, lat.stop_iter, lat.L, t, max_d, out,
                     (long long)out_stride);
}

}  // namespace spgg_rp
