// spgg_payoff.hip — the payoff field's record: the census of (strategy, cooperating neighbours,
// group-cooperator total), the bonds by their difference in that total, the plane, and the plane's
// pair sums (its own object, like spgg_reputation.hip and spgg_policy.hip).
//
// Replaces: nothing in the reference on the device; its view of the payoffs are the three lattice
// sums of spgg.py:383-394.
//
// With c = 1 where bit 0 of S_t is clear (bits 1-4 are the step kernel's bookkeeping and are
// masked), on the periodic lattice
//   N = sum5(c)        the cooperators of the group centred on a cell, 0 .. 5
//   K = sum5(N)        the cooperators of an agent's five groups, 0 .. 25
//   m = N - c          the agent's cooperating von-Neumann neighbours, 0 .. 4
//   sigma = 1 - c
//
// Census kernel.  Grid (groups_per_replica workgroups) x (replica); a workgroup takes the tiles of
// kTileW x kTileH agents blockIdx.x, blockIdx.x + gridDim.x, .. of its replica, one agent per
// thread, and adds to the replica's row once, after its last tile (spgg_policy.hip's scheme).  Per
// tile it stages c over tile + 2 cells left / above and 3 right / below in LDS -- the window is a
// view of the periodic plane, so a lattice narrower than the window (L < 5: the stencil wraps onto
// itself) only repeats in it; coordinates outside -L .. 2L take the general modulus --, then N over
// tile + 1 / 2, then K over the tile and one more column and row: an agent's right and lower
// neighbour (np.roll(., -1) on axis 1 and axis 0) have their K there, so the bonds need no second
// pass and no plane.  Each wave counts into its own LDS histogram; the lanes that share the key of
// the wave's first agent are counted by one ballot (a uniform region costs one LDS add per wave), the
// others add singly.  The workgroup adds its non-zero slots to the replica's row with int32 atomics
// (exact, order-free) after a launch that zeroed the rows.
//
// Pair sums.  The plane byte holds K in bits 0-4 and sigma in bit 5.  Staged as s = K | c << 5 (the
// bytes beyond a row's cells zero), a dword of four cells unpacks by masks into the operands
// Kq = s & 0x1f1f1f1f and cq = (s >> 5) & 0x01010101 of the int8 dot instruction (v_dot4c_i32_i8):
//   KK[d] += dot(Kq, Kq')   CK[d] += dot(cq, Kq') + dot(Kq, cq')   CC[d] += dot(cq, cq')
// Layout, work split, rotated row window and the two LDS instances / the global instance are those of
// spgg_reputation.hip's pair sums (one wave per (direction, distance) in LDS up to side 404; above it
// one workgroup per pair reads the L2-resident plane); int32 lane partials (bound: spgg_payoff.h),
// int64 from the wave reduction on.  No atomics.
#include "spgg_payoff.h"

namespace spgg_pf {
namespace {

using namespace spgg_obs;

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
}

// x mod L for any x; one correction covers -L .. 2L
__device__ __forceinline__ int wrap_any(int x, int L) {
  if (x < 0) x += L;
  else if (x >= L) x -= L;
  if (x < 0 || x >= L) {
    x %= L;
    if (x < 0) x += L;
  }
  return x;
}

// ---- census --------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void spgg_payoff_zero_kernel(int32_t* __restrict__ out, long long out_stride) {
  for (int i = threadIdx.x; i < kSlots; i += kThreads) out[(long long)blockIdx.x * out_stride + i] = 0;
}

// the slot of a bond between (c1, K1) and (c2, K2)
__device__ __forceinline__ int bond_slot(int c1, int K1, int c2, int K2) {
  const int d = K1 - K2;
  if (c1 != c2) return kBondCD + kMaxK + (c1 ? d : -d);   // K_C - K_D
  return (c1 ? kBondCC : kBondDD) + (d < 0 ? -d : d);
}

// h[key] += 1 for every lane with valid: the lanes that share the first valid lane's key by one ballot
__device__ __forceinline__ void wave_count(uint32_t* h, int key, bool valid, int lane) {
  const unsigned long long any = __ballot(valid);
  if (any == 0ull) return;   // wave-uniform
  const int leader = __ffsll((long long)any) - 1;
  const int k0 = __shfl(key, leader, 64);
  const unsigned long long same = __ballot(valid && key == k0);
  if (lane == leader) atomicAdd(&h[k0], (uint32_t)__popcll(same));
  else if (valid && key != k0) atomicAdd(&h[key], 1u);
}

__global__ __launch_bounds__(kThreads) void spgg_payoff_census_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L,
    int tiles_x, int tiles, int t, uint8_t* __restrict__ plane, int32_t* __restrict__ out, long long out_stride) {
  constexpr int CW = kTileW + 5, CH = kTileH + 5;   // c: origin (-2, -2)
  constexpr int NW = kTileW + 3, NH = kTileH + 3;   // N: origin (-1, -1)
  constexpr int KW = kTileW + 1, KH = kTileH + 1;   // K: origin (0, 0)
  __shared__ uint8_t sC[CW * CH];
  __shared__ uint8_t sN[NW * NH];
  __shared__ uint8_t sK[KW * KH];
  __shared__ uint32_t h[kWaves][kSlots];

  const int rep = blockIdx.y;
  const size_t n = (size_t)L * L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;   // n bytes apart: unaligned for odd L

  for (int i = tid; i < kWaves * kSlots; i += kThreads) (&h[0][0])[i] = 0u;
  // (the first tile's barriers order these stores before the first count)

  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // workgroup-uniform
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    for (int i = tid; i < CW * CH; i += kThreads) {
      const int wy = i / CW, wx = i - wy * CW;
      sC[i] = (uint8_t)((sp[(size_t)wrap_any(y0 - 2 + wy, L) * L + wrap_any(x0 - 2 + wx, L)] & 1u) ^ 1u);
    }
    __syncthreads();   // c
    for (int i = tid; i < NW * NH; i += kThreads) {
      const int wy = i / NW, wx = i - wy * NW;
      const uint8_t* c = sC + (wy + 1) * CW + (wx + 1);
      sN[i] = (uint8_t)(c[0] + c[-1] + c[1] + c[-CW] + c[CW]);
    }
    __syncthreads();   // N
    for (int i = tid; i < KW * KH; i += kThreads) {
      const int wy = i / KW, wx = i - wy * KW;
      const uint8_t* q = sN + (wy + 1) * NW + (wx + 1);
      sK[i] = (uint8_t)(q[0] + q[-1] + q[1] + q[-NW] + q[NW]);
    }
    __syncthreads();   // K

    const int lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int gx = x0 + lx, gy = y0 + ly;
    const bool owned = gx < L && gy < L;
    const int c = sC[(ly + 2) * CW + lx + 2], K = sK[ly * KW + lx];
    const int m = sN[(ly + 1) * NW + lx + 1] - c;
    const int sigma = 1 - c;
    if (owned && plane) plane[(size_t)rep * n + (size_t)gy * L + gx] = (uint8_t)(K | sigma << 5 | m << 6);
    wave_count(h[wave], (sigma * 5 + m) * (kMaxK + 1) + K, owned, lane);
    wave_count(h[wave], bond_slot(c, K, sC[(ly + 2) * CW + lx + 3], sK[ly * KW + lx + 1]), owned, lane);   // right
    wave_count(h[wave], bond_slot(c, K, sC[(ly + 3) * CW + lx + 2], sK[(ly + 1) * KW + lx]), owned, lane);   // lower
    __syncthreads();   // the next tile overwrites sC, sN, sK; after the last tile: the histograms
  }
  int32_t* o = out + (long long)rep * out_stride;
  for (int i = tid; i < kSlots; i += kThreads) {
    uint32_t v = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += h[w][i];
    if (v) atomicAdd(o + i, (int32_t)v);
  }
}

// ---- pair sums: the staged byte ------------------------------------------------------------

// plane bytes -> K | c << 5 (bit 5 flipped, the m bits dropped)
__device__ __forceinline__ uint32_t staged(uint32_t q) { return (q ^ 0x20202020u) & 0x3f3f3f3fu; }
__device__ __forceinline__ uint32_t k_of(uint32_t s) { return s & 0x1f1f1f1fu; }
__device__ __forceinline__ uint32_t c_of(uint32_t s) { return (s >> 5) & 0x01010101u; }

// the staged dword of the cells x0 .. x0 + 3 of a row in global memory (row + x0 need not be
// aligned), the bytes beyond the row's L cells zero
__device__ __forceinline__ uint32_t load_cells(const uint8_t* row, int x0, int L) {
  uint32_t q = 0u;
  if (x0 + 4 <= L) {
    __builtin_memcpy(&q, row + x0, 4);
    return staged(q);
  }
  for (int j = 0; j < 4; ++j)
    if (x0 + j < L) q |= (((uint32_t)row[x0 + j] ^ 0x20u) & 0x3fu) << (8 * j);
  return q;
}

// the three sums of one dword pair
struct Acc {
  int kk = 0, ck = 0, cc = 0;
  __device__ __forceinline__ void add(uint32_t own, uint32_t v) {
    const uint32_t ko = k_of(own), co = c_of(own), kv = k_of(v), cv = c_of(v);
    kk = dot4(ko, kv, kk);
    ck = dot4(co, kv, dot4(ko, cv, ck));
    cc = dot4(co, cv, cc);
  }
};

// ---- pair sums: LDS instances --------------------------------------------------------------

template <int kCapDwords>
__global__ __launch_bounds__(kPairThreads) void spgg_payoff_pairs_lds_kernel(const uint8_t* __restrict__ planes, int L,
                                                                             int max_d, long long* __restrict__ out,
                                                                             long long out_stride) {
  __shared__ uint32_t lat[kCapDwords];

  const int W = row_dwords(L), dwords = L * W;
  if (L < 1 || dwords > kCapDwords) return;   // (the host picks the instance: launch_pairs)
  const int rep = blockIdx.y;
  const int n = L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint8_t* plane = planes + (size_t)rep * n;   // n bytes apart: for odd L not 4-byte aligned

  // stage: a wave takes 256 cells of a row at a time, a lane 4 of them; kStageDepth rows per
  // trip, their loads issued before the first is stored
  const int chunks = (W + 63) >> 6;
  for (int y0 = wave; y0 < L; y0 += kPairWaves * kStageDepth) {   // wave-uniform, like ch and u
    for (int ch = 0; ch < chunks; ++ch) {
      const int w = ch * 64 + lane;
      uint32_t q[kStageDepth];
#pragma unroll
      for (int u = 0; u < kStageDepth; ++u) {
        const int y = y0 + u * kPairWaves;
        q[u] = (y < L && w < W) ? load_cells(plane + (size_t)y * L, 4 * w, L) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kStageDepth; ++u) {
        const int y = y0 + u * kPairWaves;
        if (y < L && w < W) lat[y * W + w] = q[u];
      }
    }
  }
  __syncthreads();

  const int d = blockIdx.x * kDistPerGroup + (wave >> 1);
  if (d > max_d) return;   // wave-uniform; no barrier follows
  Acc acc;                 // int32 lane partials: at most lane_dots_lds(L) dword pairs each
  int sum_k = 0, sum_c = 0;
  if (wave & 1) {   // columns
    const int shift = d * W;   // <= dwords / 2
#pragma unroll 4
    for (int i = lane; i < dwords; i += 64) {
      int j = i + shift;
      if (j >= dwords) j -= dwords;
      acc.add(lat[i], lat[j]);
    }
  } else {          // rows: the rotated window of spgg_reputation.hip
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
#pragma unroll 4
        for (int y = y0; y < L; y += per_trip) {
          const uint32_t* row = lat + y * W;
          const uint32_t lo = row[a], hi = row[a1] & two, first = row[0], own = row[w];
          const uint32_t v = (__builtin_amdgcn_alignbyte(hi, lo, sh) & keep) | ((first << up) & wrap_mask);
          acc.add(own, v);
          if (with_sum) {
            sum_k = dot4(k_of(own), 0x01010101u, sum_k);
            sum_c = dot4(c_of(own), 0x01010101u, sum_c);
          }
        }
      }
    }
  }
  const long long kk = wave_sum((long long)acc.kk), ck = wave_sum((long long)acc.ck), cc = wave_sum((long long)acc.cc);
  long long* o = out + (long long)rep * out_stride;
  if (lane == 0) {
    long long* p = o + 2 + 3 * ((wave & 1) * (max_d + 1) + d);
    p[0] = kk;
    p[1] = ck;
    p[2] = cc;
  }
  if (!(wave & 1) && d == 0) {   // wave-uniform
    const long long a = wave_sum((long long)sum_k), b = wave_sum((long long)sum_c);
    if (lane == 0) {
      o[0] = a;
      o[1] = b;
    }
  }
}

// ---- pair sums: global instance ------------------------------------------------------------

__global__ __launch_bounds__(kPairThreads) void spgg_payoff_pairs_global_kernel(const uint8_t* __restrict__ planes, int L,
                                                                                int max_d, long long* __restrict__ out,
                                                                                long long out_stride) {
  __shared__ long long part[5][kPairWaves];

  const int W = row_dwords(L);
  const int rep = blockIdx.y;
  const size_t n = (size_t)L * L;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint8_t* plane = planes + (size_t)rep * n;
  const bool cols = (int)blockIdx.x > max_d;               // pairs 0 .. max_d: rows, then columns
  const int d = cols ? (int)blockIdx.x - (max_d + 1) : (int)blockIdx.x;
  const bool with_sum = blockIdx.x == 0;                   // the workgroup of rows[0] also sums the plane

  Acc acc;   // int32 lane partials: at most lane_dots_global(L) dword pairs each
  int sum_k = 0, sum_c = 0;
  for (int w = lane; w < W; w += 64) {
    const int x0 = kCellsPerDword * w;
    const int valid = min(kCellsPerDword, L - x0);
    int s = x0 + d;   // rows: the window's first cell, < 2 L
    if (s >= L) s -= L;
    const bool whole = valid == kCellsPerDword && s + kCellsPerDword <= L;   // no row end, no wrap
#pragma unroll 2
    for (int y = wave; y < L; y += kPairWaves) {
      const uint8_t* row = plane + (size_t)y * L;
      const uint32_t own = load_cells(row, x0, L);
      uint32_t v = 0u;
      if (cols) {
        int y2 = y + d;
        if (y2 >= L) y2 -= L;
        v = load_cells(plane + (size_t)y2 * L, x0, L);
      } else if (whole) {
        __builtin_memcpy(&v, row + s, 4);
        v = staged(v);
      } else {
        for (int j = 0; j < valid; ++j) {   // valid <= L: the window wraps at most once
          int x = s + j;
          if (x >= L) x -= L;
          v |= (((uint32_t)row[x] ^ 0x20u) & 0x3fu) << (8 * j);
        }
      }
      acc.add(own, v);
      if (with_sum) {
        sum_k = dot4(k_of(own), 0x01010101u, sum_k);
        sum_c = dot4(c_of(own), 0x01010101u, sum_c);
      }
    }
  }
  const long long r[5] = {wave_sum((long long)acc.kk), wave_sum((long long)acc.ck), wave_sum((long long)acc.cc),
                          wave_sum((long long)sum_k), wave_sum((long long)sum_c)};
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) part[k][wave] = r[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    long long a = 0;
#pragma unroll
    for (int v = 0; v < kPairWaves; ++v) a += part[threadIdx.x][v];
    long long* o = out + (long long)rep * out_stride;
    if (threadIdx.x < 3) o[2 + 3 * (int)blockIdx.x + threadIdx.x] = a;   // rows[d] at pair d, cols[d] at max_d + 1 + d
    else if (with_sum) o[threadIdx.x - 3] = a;
  }
}

}  // namespace

void launch_census(const spgg_obs::Lattices& lat, int t, uint8_t* plane, int32_t* out, int64_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(spgg_payoff_zero_kernel, dim3(lat.n_rep), dim3(kThreads), 0, s, out, (long long)out_stride);
  const int tiles_x = (lat.L + kTileW - 1) / kTileW, tiles_y = (lat.L + kTileH - 1) / kTileH;
  const int tiles = tiles_x * tiles_y;
  hipLaunchKernelGGL(spgg_payoff_census_kernel, dim3((unsigned)groups_per_replica(tiles, lat.n_rep), lat.n_rep),
                     dim3(kThreads), 0, s, lat.S0, lat.S1, lat.stop_iter, lat.L, tiles_x, tiles, t, plane, out,
                     (long long)out_stride);
}

void launch_pairs(const spgg_obs::Lattices& lat, int max_d, const uint8_t* plane, long long* out, int64_t out_stride,
                  hipStream_t s) {
  dim3 grid((max_d + kDistPerGroup) / kDistPerGroup, lat.n_rep);
  auto kernel = spgg_payoff_pairs_lds_kernel<kFullDwords>;
  if (lat.L > kMaxLdsSide) {
    kernel = spgg_payoff_pairs_global_kernel;
    grid.x = 2 * (max_d + 1);
  } else if (lattice_dwords(lat.L) <= kSmallDwords) {
    kernel = spgg_payoff_pairs_lds_kernel<kSmallDwords>;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(kPairThreads), 0, s, plane, lat.L, max_d, out, (long long)out_stride);
}

}  // namespace spgg_pf
