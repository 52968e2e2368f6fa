// spgg_clusters.hip — 4-connected cooperator clusters of a strategy plane, one workgroup per
// replica, the whole lattice in LDS (its own object, like spgg_mt.hip).
//
// Replaces: scipy.ndimage.label + the per-label sums of src/model/spgg.py:631-633 (the
// reference labels once per run, on the host); the three-value record has no counterpart there.
//
// Method (label equivalence).  label[g] (16 bit; kDefector for S = 1) starts as the raster index
// y*L + x of the first cell of the cell's row run of cooperators (its own index g for that first
// cell), ref[x] = x.  A pass is
//   scan     every cooperator takes the minimum label m among its cooperator neighbours; if
//            m < its own label `own` it lowers ref[own] to min(ref[own], m)
//   resolve  every representative x (label[x] == x) whose ref was lowered follows ref to its
//            end r (ref[r] == r) and stores label[x] = r
//   relabel  label[g] = label[label[g]] for every cooperator
// until a scan lowers nothing: then equal labels <=> same cluster, and a cluster's label is its
// smallest raster index (labels only ever decrease to labels of the same cluster, and a scan
// that changes nothing means no two neighbouring cooperators differ).
//
// Termination, from the code alone:
//   * ref[x] <= x always (a scan writes m < own into ref[own], or something smaller), so a
//     resolve chase is a strictly decreasing walk of at most n steps (and is capped at n);
//   * barriers separate scan, resolve and relabel.  A scan reads label and writes ref; resolve
//     reads ref and writes label[x] of its own representative only; relabel reads label[l] of
//     a representative l, which a concurrent relabel of l itself can only overwrite with the
//     same value (label[l] is a root r after resolve, and label[r] == r);
//   * the 16-bit minimum is a compare-and-swap of the containing LDS word: a failed swap means
//     another thread strictly lowered one of the word's two halves, at most 2 * 65535 times
//     (the loop is capped there);
//   * the pass loop is capped at kMaxPasses; on the cap (or a capped chase / swap, which cannot
//     happen) the replica's record gets n_clusters = -1 and the host raises;
//   * nothing waits for another workgroup or for global memory.
#include "spgg_clusters.h"

#include "spgg_device.h"

namespace spgg_cl {
namespace {

constexpr uint32_t kDefector = 0xffffu;   // reserved label (cells are numbered 0 .. 39,999)
constexpr int kSwapCap = 2 * 65536;

static_assert(kMaxCells < (int)kDefector, "labels must fit 16 bits beside the reserved value");
static_assert(kMaxCells % 2 == 0, "two labels per LDS word");

// workgroup-shared words beside the two planes
enum { W_CHANGED = 0, W_FAIL, W_NCLU, W_BONDS, W_LARGEST, W_COUNT = 8 };

// the planes are LDS words (the swaps and packed adds) read and written as halves
typedef uint16_t __attribute__((may_alias)) half_t;

__device__ __forceinline__ uint32_t half_of(const uint32_t* words, int i) {
  return reinterpret_cast<const half_t*>(words)[i];
}

__device__ __forceinline__ void set_half(uint32_t* words, int i, uint32_t v) {
  reinterpret_cast<half_t*>(words)[i] = (half_t)v;
}

// ref[x] = min(ref[x], m); true if this call lowered it.  *fail is set if the swap loop runs
// out of its (unreachable) bound.
__device__ __forceinline__ bool lower_ref(uint32_t* ref, int x, uint32_t m, uint32_t* fail) {
  uint32_t* w = ref + (x >> 1);
  const int sh = (x & 1) * 16;
  uint32_t old = *w;
  for (int k = 0; k < kSwapCap; ++k) {
    if (((old >> sh) & 0xffffu) <= m) return false;
    const uint32_t want = (old & ~(0xffffu << sh)) | (m << sh);
    const uint32_t seen = atomicCAS(w, old, want);
    if (seen == old) return true;
    old = seen;
  }
  *fail = 1u;
  return false;
}

__global__ __launch_bounds__(kThreads) void spgg_clusters_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter,
    int L, int t, int periodic, int32_t* __restrict__ sizes, int32_t* __restrict__ rec, long long rec_stride) {
  __shared__ uint32_t label[kMaxCells / 2];   // two 16-bit labels per word
  __shared__ uint32_t ref[kMaxCells / 2];     // two 16-bit refs per word; afterwards the counts
  __shared__ uint32_t sh[W_COUNT];

  const int n = L * L;
  if (L < 1 || n > kMaxCells) return;   // (the host refuses these: spgg_clusters)
  const int rep = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63;
  // the plane holding S_t; a replica absorbed before t keeps its state in S_stop's plane
  const int stop = stop_iter ? stop_iter[rep] : 0;
  const int tt = (stop == 0 || stop >= t) ? t : stop;
  const uint8_t* plane = (((tt - 1) & 1) ? S1 : S0) + (size_t)rep * n;
  int32_t* out_rec = rec + (long long)rep * rec_stride;

  if (tid < W_COUNT) sh[tid] = 0u;
  for (int g = tid; g < n; g += nthr) {
    set_half(label, g, (plane[g] & 1) ? kDefector : (uint32_t)g);   // bit 0 only: 0 = cooperator
    set_half(ref, g, (uint32_t)g);
  }
  __syncthreads();
  // every cooperator starts with the label of the first cell of its row run (one thread per
  // row, L steps): the first resolve then hops from run to run instead of from cell to cell.
  // A run's first cell keeps its own index, so the labels in use are still representatives.
  for (int y = tid; y < L; y += nthr) {
    uint32_t run = kDefector;
    for (int g = y * L; g < (y + 1) * L; ++g) {
      if (half_of(label, g) == kDefector) run = kDefector;
      else if (run == kDefector) run = (uint32_t)g;
      else set_half(label, g, run);
    }
  }
  __syncthreads();

  // C-D bonds, always periodic: sum(S != roll(S,1,0)) + sum(S != roll(S,1,1))
  uint32_t part[2] = {0u, 0u};   // {clusters, bonds} of this thread
  for (int g = tid; g < n; g += nthr) {
    const int y = g / L, x = g - y * L;
    const bool d = half_of(label, g) == kDefector;
    const int up = (y > 0 ? g : g + n) - L, left = x > 0 ? g - 1 : g + L - 1;
    part[1] += (uint32_t)(d != (half_of(label, up) == kDefector)) +
               (uint32_t)(d != (half_of(label, left) == kDefector));
  }

  bool converged = false;
  for (int pass = 0; pass < kMaxPasses; ++pass) {
    // scan (reads label, lowers ref)
    bool lowered = false;
    for (int g = tid; g < n; g += nthr) {
      const uint32_t own = half_of(label, g);
      if (own == kDefector) continue;
      const int y = g / L, x = g - y * L;
      uint32_t m = own;
      if (y > 0) m = min(m, half_of(label, g - L));
      else if (periodic) m = min(m, half_of(label, g + n - L));
      if (y < L - 1) m = min(m, half_of(label, g + L));
      else if (periodic) m = min(m, half_of(label, g - n + L));
      if (x > 0) m = min(m, half_of(label, g - 1));
      else if (periodic) m = min(m, half_of(label, g + L - 1));
      if (x < L - 1) m = min(m, half_of(label, g + 1));
      else if (periodic) m = min(m, half_of(label, g - L + 1));
      if (m < own) lowered |= lower_ref(ref, (int)own, m, &sh[W_FAIL]);
    }
    if (lowered) sh[W_CHANGED] = 1u;
    __syncthreads();
    const bool changed = sh[W_CHANGED] != 0u, failed = sh[W_FAIL] != 0u;   // workgroup-uniform
    if (failed) break;
    if (!changed) {
      converged = true;
      break;
    }
    // resolve (reads ref, writes label[x] of this thread's representatives)
    for (int x = tid; x < n; x += nthr) {
      if (half_of(label, x) != (uint32_t)x) continue;
      uint32_t r = half_of(ref, x);
      if (r == (uint32_t)x) continue;
      int k = 0;
      for (; k < n; ++k) {   // ref[r] < r until the root: at most n steps
        const uint32_t q = half_of(ref, (int)r);
        if (q == r) break;
        r = q;
      }
      if (k == n) sh[W_FAIL] = 1u;
      set_half(label, x, r);
    }
    __syncthreads();
    if (tid == 0) sh[W_CHANGED] = 0u;   // (read above, before the barrier; next written after the next one)
    // relabel
    for (int g = tid; g < n; g += nthr) {
      const uint32_t l = half_of(label, g);
      if (l != kDefector) set_half(label, g, half_of(label, (int)l));
    }
    __syncthreads();
  }
  if (!converged) {   // workgroup-uniform: the pass cap (or an unreachable loop cap)
    if (tid == 0) {
      out_rec[0] = -1;
      out_rec[1] = 0;
      out_rec[2] = 0;
    }
    return;
  }

  // sizes: ref becomes the table of 16-bit counts (a count is at most n < 65,536, so the
  // packed add of a low half never carries into the high one)
  for (int w = tid; w < (n + 1) / 2; w += nthr) ref[w] = 0u;
  __syncthreads();
  for (int base = 0; base < n; base += nthr) {   // wave-uniform trip count
    const int g = base + tid;
    const uint32_t l = g < n ? half_of(label, g) : kDefector;
    const bool c = l != kDefector;
    const unsigned long long any = __ballot(c);
    if (any == 0ull) continue;
    // the lanes that share the first cooperator's label add once (a large cluster is most of a wave)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)any) - 1);
    const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)l, leader);
    const bool same = c && l == first;
    const unsigned long long grp = __ballot(same);
    if (lane == leader) atomicAdd(&ref[first >> 1], (uint32_t)__popcll(grp) << ((first & 1u) * 16));
    if (c && !same) atomicAdd(&ref[l >> 1], 1u << ((l & 1u) * 16));
  }
  __syncthreads();

  uint32_t largest = 0u;
  int32_t* out_sizes = sizes ? sizes + (size_t)rep * n : nullptr;
  for (int g = tid; g < n; g += nthr) {
    uint32_t sz = 0u;
    if (half_of(label, g) == (uint32_t)g) {   // representative: the cluster's smallest raster index
      sz = half_of(ref, g);
      part[0] += 1u;
      largest = max(largest, sz);
    }
    if (out_sizes) out_sizes[g] = (int32_t)sz;
  }
  // wave sums of {clusters, bonds}: afterwards lanes 0..31 hold value 0's, lanes 32..63 value 1's
  spgg::transpose_level<2, 32, 2, uint32_t>(part, lane);
  if ((lane & 31) == 0) atomicAdd(&sh[W_NCLU + (lane >> 5)], part[0]);
  if (largest) atomicMax(&sh[W_LARGEST], largest);
  __syncthreads();
  if (tid == 0) {
    out_rec[0] = (int32_t)sh[W_NCLU];
    out_rec[1] = (int32_t)sh[W_LARGEST];
    out_rec[2] = (int32_t)sh[W_BONDS];
  }
}

}  // namespace

void launch(const uint8_t* S0, const uint8_t* S1, const int32_t* stop_iter, int n_rep, int L, int t,
            int periodic, int32_t* sizes, int32_t* rec, int64_t rec_stride, hipStream_t s) {
  const int n = L * L;
  const int threads = n >= kThreads ? kThreads : ((n + 63) / 64) * 64;   // whole waves
  hipLaunchKernelGGL(spgg_clusters_kernel, dim3(n_rep), dim3(threads), 0, s, S0, S1, stop_iter, L, t,
                     periodic ? 1 : 0, sizes, rec, (long long)rec_stride);
}

}  // namespace spgg_cl
