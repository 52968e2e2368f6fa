// spgg_dwell.hip — the per-agent strategy dwell record (its own object, like spgg_reputation.hip).
//
// Replaces: nothing in the reference; the quantities need every S_t, which a run never copies out.
//
// With tracking started at t_ref (strategy = bit 0 of S, 0 = C; the launch of iteration j turns
// S_j into S_{j+1}), an agent's words hold
//   flips        the number of j in t_ref .. t-1 with S_{j+1} != S_j
//   since        the smallest j >= t_ref with S_j == .. == S_t
//   coop_closed  the length of its cooperator runs that have ended
// and are written only when the agent flips: at launch j, flips += 1, a cooperator adds
// (j + 1) - since to coop_closed, since = j + 1.  The open run is added at read-out:
//   age = t - since        coop(t) = coop_closed + (S_t == C ? t - since + 1 : 0)
//
// Step launch.  Grid (chunk of kStepCells cells) x (replica).  A thread loads the same kRun bytes
// of both planes as four dwords each and XORs bit 0 of every byte; nothing flipped: it is done
// (2 bytes of traffic per agent).  Each flipper costs one 12-byte load and store.  No atomics, no
// LDS: an agent's words belong to one thread.  With n % 4 != 0 (odd L) the replica bases are not
// dword-aligned and the thread gathers its bytes one by one into the same four dwords; the bytes
// of a run beyond the replica's n cells are never read and stay zero in both, so they never flip.
// A replica's stop_iter is read once per workgroup (scalar): an absorbed replica's workgroups return.
//
// Read-outs.  Grid (chunk of kCells cells) x (replica), a thread the cells tid, tid + kThreads, ..
// of the chunk.  An absorbed replica (stop s < t) is read as of t = s from plane (s - 1) & 1.
// Record: per-thread counts (the two sums in 64 bits), age bins in one LDS histogram per wave,
// wave shuffles and an LDS pass across the waves, then one 64-bit integer atomic per non-zero slot
// (exact, order-free); a launch ahead of it zeroes the rows.
#include "spgg_dwell.h"

namespace spgg_dw {
namespace {

struct Words {
  uint32_t flips, since, coop;
};
static_assert(sizeof(Words) == 4 * kWords && alignof(Words) == 4, "[n_rep][n][3] uint32");

using namespace spgg_obs;

// the state index a read-out of t describes: a replica absorbed at s < t stays at S_s (and one
// absorbed before tracking began at S_{t_ref} = S_s)
__device__ __forceinline__ int state_of(const int32_t* stop_iter, int rep, int t, int t_ref) {
  return max(t_ref, observed_iter(stop_iter, rep, t));
}

__global__ __launch_bounds__(kThreads) void spgg_dwell_reset_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int n,
    int t_ref, Words* __restrict__ words, uint8_t* __restrict__ ref) {
  const int rep = blockIdx.y;
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t_ref) + (size_t)rep * n;
  const int base = blockIdx.x * kCells;
#pragma unroll 4
  for (int u = 0; u < kCells / kThreads; ++u) {
    const int i = base + u * kThreads + (int)threadIdx.x;
    if (i >= n) break;
    ref[(size_t)rep * n + i] = sp[i] & 1u;
    words[(size_t)rep * n + i] = Words{0u, (uint32_t)t_ref, 0u};
  }
}

// the words of the agents whose bit is set in x (bit 0 of byte u: agent i0 + u), a the dword of S_j
__device__ __forceinline__ void flip_dword(Words* __restrict__ w, uint32_t x, uint32_t a, uint32_t next) {
  while (x) {
    const int bit = __builtin_ctz(x);   // 0, 8, 16 or 24
    x &= x - 1u;
    Words v = w[bit >> 3];
    v.flips += 1u;
    if (((a >> bit) & 1u) == 0u) v.coop += next - v.since;   // a cooperator's run ends
    v.since = next;
    w[bit >> 3] = v;
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void spgg_dwell_step_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int n, int j,
    Words* __restrict__ words) {
  const int rep = blockIdx.y;
  if (stop_iter[rep] != 0) return;   // absorbed at or before j (uniform): launch j wrote no S_{j+1}
  const int i0 = ((int)blockIdx.x * kThreads + (int)threadIdx.x) * kRun;
  if (i0 >= n) return;
  const uint8_t* pa = ((j & 1) ? S0 : S1) + (size_t)rep * n + i0;   // S_j: plane (j - 1) & 1
  const uint8_t* pb = ((j & 1) ? S1 : S0) + (size_t)rep * n + i0;   // S_{j+1}: plane j & 1
  const int valid = min(kRun, n - i0);
  uint32_t a[kRun / 4] = {0u, 0u, 0u, 0u}, b[kRun / 4] = {0u, 0u, 0u, 0u};
  if (ALIGNED) {   // n % 4 == 0: rep * n + i0 and valid are multiples of 4
    const uint32_t* qa = reinterpret_cast<const uint32_t*>(pa);
    const uint32_t* qb = reinterpret_cast<const uint32_t*>(pb);
    if (valid == kRun) {
#pragma unroll
      for (int d = 0; d < kRun / 4; ++d) {
        a[d] = qa[d];
        b[d] = qb[d];
      }
    } else {
#pragma unroll
      for (int d = 0; d < kRun / 4; ++d) {
        if (4 * d < valid) {
          a[d] = qa[d];
          b[d] = qb[d];
        }
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
      if (u < valid) {
        a[u >> 2] |= (uint32_t)pa[u] << (8 * (u & 3));
        b[u >> 2] |= (uint32_t)pb[u] << (8 * (u & 3));
      }
    }
  }
  uint32_t x[kRun / 4];
  uint32_t any = 0u;
#pragma unroll
  for (int d = 0; d < kRun / 4; ++d) {
    x[d] = (a[d] ^ b[d]) & 0x01010101u;
    any |= x[d];
  }
  if (!any) return;
  Words* w = words + (size_t)rep * n + i0;
#pragma unroll
  for (int d = 0; d < kRun / 4; ++d) flip_dword(w + 4 * d, x[d], a[d], (uint32_t)j + 1u);
}

__global__ __launch_bounds__(kThreads) void spgg_dwell_zero_kernel(long long* __restrict__ out, long long out_stride) {
  for (int i = threadIdx.x; i < kSlots; i += kThreads) out[(long long)blockIdx.x * out_stride + i] = 0;
}

__global__ __launch_bounds__(kThreads) void spgg_dwell_record_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int n, int t,
    int t_ref, const Words* __restrict__ words, const uint8_t* __restrict__ ref, unsigned long long* __restrict__ out,
    long long out_stride) {
  __shared__ uint32_t bins[kWaves][2 * kAgeBins];
  __shared__ unsigned long long part[kWaves][7];

  const int rep = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t te = (uint32_t)state_of(stop_iter, rep, t, t_ref);
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  const uint8_t* rp = ref + (size_t)rep * n;
  const Words* wp = words + (size_t)rep * n;

  for (int i = tid; i < kWaves * 2 * kAgeBins; i += kThreads) (&bins[0][0])[i] = 0u;
  __syncthreads();

  uint32_t never = 0u, never_c = 0u, same = 0u, both_c = 0u, ncoop = 0u;
  unsigned long long flips = 0ull, coop_time = 0ull;
  const int base = blockIdx.x * kCells;
#pragma unroll 4
  for (int u = 0; u < kCells / kThreads; ++u) {
    const int i = base + u * kThreads + tid;
    if (i >= n) break;
    const uint32_t s = sp[i] & 1u, r = rp[i] & 1u;
    const Words v = wp[i];
    const uint32_t age = te - v.since;
    const uint32_t c = s ^ 1u, rc = r ^ 1u, nv = v.flips == 0u;
    never += nv;
    never_c += nv & rc;
    same += s == r;
    both_c += c & rc;
    ncoop += c;
    flips += v.flips;
    coop_time += v.coop + (c ? age + 1u : 0u);
    // age + 1 >= 1; the clamp keeps a t behind the words' own state (a caller's error) inside the row
    atomicAdd(&bins[wave][s * kAgeBins + min(31 - __builtin_clz(age + 1u), kAgeBins - 1)], 1u);
  }
  const unsigned long long sums[7] = {wave_sum(never), wave_sum(never_c), wave_sum(same), wave_sum(both_c),
                                      wave_sum(ncoop), wave_sum(flips),   wave_sum(coop_time)};
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) part[wave][k] = sums[k];
  }
  __syncthreads();
  if (tid < kSlots) {
    unsigned long long c = 0ull;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += tid < 7 ? part[w][tid] : (unsigned long long)bins[w][tid - 7];
    if (c) atomicAdd(out + (long long)rep * out_stride + tid, c);
  }
}

__global__ __launch_bounds__(kThreads) void spgg_dwell_fields_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int n, int t,
    int t_ref, const Words* __restrict__ words, int32_t* __restrict__ out, long long out_stride) {
  const int rep = blockIdx.y;
  const uint32_t te = (uint32_t)state_of(stop_iter, rep, t, t_ref);
  const uint8_t* sp = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  const Words* wp = words + (size_t)rep * n;
  int32_t* o = out + (long long)rep * out_stride;
  const int base = blockIdx.x * kCells;
#pragma unroll 4
  for (int u = 0; u < kCells / kThreads; ++u) {
    const int i = base + u * kThreads + (int)threadIdx.x;
    if (i >= n) break;
    const Words v = wp[i];
    const uint32_t age = te - v.since;
    o[i] = (int32_t)v.flips;
    o[(size_t)n + i] = (int32_t)age;
    o[2 * (size_t)n + i] = (int32_t)(v.coop + ((sp[i] & 1u) ? 0u : age + 1u));
  }
}

inline dim3 readout_grid(const Lattices& lat) { return dim3((unsigned)((lat.cells() + kCells - 1) / kCells), lat.n_rep); }

}  // namespace

void launch_reset(const spgg_obs::Lattices& lat, int t_ref, uint32_t* words, uint8_t* ref, hipStream_t s) {
  hipLaunchKernelGGL(spgg_dwell_reset_kernel, readout_grid(lat), dim3(kThreads), 0, s, lat.S0, lat.S1, lat.stop_iter,
                     (int)lat.cells(), t_ref, reinterpret_cast<Words*>(words), ref);
}

void launch_step(const spgg_obs::Lattices& lat, int j, uint32_t* words, hipStream_t s) {
  const long long n = lat.cells();
  const dim3 grid((unsigned)((n + kStepCells - 1) / kStepCells), lat.n_rep);
  // dword loads need every replica base rep * n (and the caller's planes: spgg_dwell_bind) aligned
  const bool aligned =
      n % 4 == 0 && ((reinterpret_cast<uintptr_t>(lat.S0) | reinterpret_cast<uintptr_t>(lat.S1)) & 3) == 0;
  hipLaunchKernelGGL(aligned ? spgg_dwell_step_kernel<true> : spgg_dwell_step_kernel<false>, grid, dim3(kThreads), 0, s,
                     lat.S0, lat.S1, lat.stop_iter, (int)n, j, reinterpret_cast<Words*>(words));
}

void launch_record(const spgg_obs::Lattices& lat, int t, int t_ref, const uint32_t* words, const uint8_t* ref,
                   long long* out, int64_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(spgg_dwell_zero_kernel, dim3(lat.n_rep), dim3(kThreads), 0, s, out, (long long)out_stride);
  hipLaunchKernelGGL(spgg_dwell_record_kernel, readout_grid(lat), dim3(kThreads), 0, s, lat.S0, lat.S1, lat.stop_iter,
                     (int)lat.cells(), t, t_ref, reinterpret_cast<const Words*>(words), ref,
                     reinterpret_cast<unsigned long long*>(out), (long long)out_stride);
}

void launch_fields(const spgg_obs::Lattices& lat, int t, int t_ref, const uint32_t* words, int32_t* out,
                   int64_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(spgg_dwell_fields_kernel, readout_grid(lat), dim3(kThreads), 0, s, lat.S0, lat.S1, lat.stop_iter,
                     (int)lat.cells(), t, t_ref, reinterpret_cast<const Words*>(words), out, (long long)out_stride);
}

}  // namespace spgg_dw
