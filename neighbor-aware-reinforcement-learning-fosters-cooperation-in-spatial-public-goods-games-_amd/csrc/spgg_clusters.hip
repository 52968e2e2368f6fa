// spgg_clusters.hip — 4-connected cooperator clusters of a strategy plane, one workgroup per
// replica, the whole lattice in LDS (its own object, like spgg_mt.hip).
//
// Replaces: scipy.ndimage.label + the per-label sums of src/model/spgg.py:631-633 (the
// reference labels once per run, on the host); the three-value record has no counterpart there.
//
// The labelling pass -- method, termination -- is spgg_label_lds.h's, here on the whole L x L
// lattice.  This object's own: the C-D bonds from the label plane, and the cluster sizes as
// 16-bit counts in the ref plane once the pass is done with it (wave-aggregated packed LDS adds).
// On a pass that did not converge the replica's record gets n_clusters = -1 and the host raises.
#include "spgg_clusters.h"

#include "spgg_device.h"
#include "spgg_label_lds.h"

namespace spgg_cl {
namespace {

using namespace spgg_obs;

static_assert(kMaxCells < (int)kDefector, "labels must fit 16 bits beside the reserved value");
static_assert(kMaxCells % 2 == 0, "two labels per LDS word");

// workgroup-shared words beside the two planes, after the labelling pass's
enum { W_NCLU = W_LABEL_WORDS, W_BONDS, W_LARGEST, W_COUNT = 8 };

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
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  int32_t* out_rec = rec + (long long)rep * rec_stride;

  if (tid < W_COUNT) sh[tid] = 0u;
  for (int g = tid; g < n; g += nthr) {
    set_half(label, g, (plane[g] & 1) ? kDefector : (uint32_t)g);   // bit 0 only: 0 = cooperator
    set_half(ref, g, (uint32_t)g);
  }
  __syncthreads();
  if (!label_region(label, ref, sh, L, L, periodic != 0)) {   // workgroup-uniform
    if (tid == 0) {
      out_rec[0] = -1;
      out_rec[1] = 0;
      out_rec[2] = 0;
    }
    return;
  }

  // C-D bonds, always periodic: sum(S != roll(S,1,0)) + sum(S != roll(S,1,1))
  uint32_t part[2] = {0u, 0u};   // {clusters, bonds} of this thread
  for (int g = tid; g < n; g += nthr) {
    const int y = g / L, x = g - y * L;
    const bool d = half_of(label, g) == kDefector;
    const int up = (y > 0 ? g : g + n) - L, left = x > 0 ? g - 1 : g + L - 1;
    part[1] += (uint32_t)(d != (half_of(label, up) == kDefector)) +
               (uint32_t)(d != (half_of(label, left) == kDefector));
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

void launch(const spgg_obs::Lattices& lat, int t, int periodic, int32_t* sizes, int32_t* rec, int64_t rec_stride,
            hipStream_t s) {
  const int n = lat.L * lat.L;
  const int threads = n >= kThreads ? kThreads : ((n + 63) / 64) * 64;   // whole waves
  hipLaunchKernelGGL(spgg_clusters_kernel, dim3(lat.n_rep), dim3(threads), 0, s, lat.S0, lat.S1,
                     lat.stop_iter, lat.L, t, periodic ? 1 : 0, sizes, rec, (long long)rec_stride);
}

}  // namespace spgg_cl
