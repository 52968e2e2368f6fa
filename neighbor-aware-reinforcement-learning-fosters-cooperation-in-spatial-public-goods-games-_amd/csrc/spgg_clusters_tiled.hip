// spgg_clusters_tiled.hip — 4-connected cooperator clusters of a strategy plane of any side, one
// replica spread over many workgroups (its own object, like spgg_clusters.hip).
//
// Replaces: scipy.ndimage.label + the per-label sums of src/model/spgg.py:631-633 on lattices
// wider than spgg_clusters' 200 (which were copied to the host and labelled there); the
// three-value record has no counterpart in the reference.
//
// Workspace of a replica (int32): parent[n], count[n], flags[kFlagWords].  Five launches:
//   init    rec = {0, 0, 0}, flags = 0
//   tile    one workgroup per tile x tile square (ragged at the right and bottom edge) labels it
//           in LDS with the tile edge as a wall -- the pass of spgg_label_lds.h on 16-bit local
//           labels -- and writes, for every cell of the tile,
//           parent[g] = the global raster index of the first cell of its tile cluster (row-major
//           order in a tile agrees with the raster order, so that is the tile cluster's smallest
//           index; g itself for a defector) and count[g] = 0
//   seam    one thread per pair of cells that face each other across a tile edge (periodic: also
//           across the lattice edge); two cooperators are united in parent
//   count   every cooperator finds its root and adds one to count[root], aggregated per wave
//           and per workgroup before the global atomic
//   record  clusters = cooperators with parent[g] == g, largest = max count, bonds from S;
//           sizes[g] = count[g] at a root, 0 elsewhere
//
// The union.  parent[x] <= x always, and parent[x] is a cell of x's own cluster: the tile pass
// writes it so, and the only later writes are atomic minima with a value v < x that a walk from
// a cell of x's cluster reached (unite: the root of a neighbouring cooperator; find: the
// grandparent, path halving).  So every walk is strictly decreasing (at most n steps; capped at
// n), a cluster's root is its smallest raster index once every pair is united, and a union that
// loses its atomic minimum -- the word at `hi` was lowered first, to `old` -- goes on with
// (old, lo), both below hi: the retries descend too (capped at kMaxRetries).  Whatever the
// minimum left in parent[hi], hi stays linked to a cell of its cluster and the pending pair
// (old, lo) carries the connection the overwritten link held.
//
// Why a stale read is harmless.  Words another workgroup of the same launch may write (parent
// in seam and count; count[] in count) are only read by agent-scope atomic loads or returned
// atomics.  Should a load still return an older value of a word, that value is an earlier
// parent of the same cell: a cell of the same cluster with an index between the current parent
// and the cell.  A walk that follows it ends at a cell of the right cluster that may no longer
// be a root; the atomic minimum on that cell returns the word's true value, sees that it is not
// a root and retries from the value returned.  A stale read costs a retry, never a wrong union.
// The count launch runs after the seam launch ended, so every link is visible to it; its own
// halving writes only shorten paths.
//
// Termination, from the code alone: the LDS pass and its loops are capped (spgg_label_lds.h),
// every walk at n steps, every union at kMaxRetries, and a parent word
// outside 0 .. x ends the walk.  Any cap sets flags[F_FAIL]; the record launch then writes
// n_clusters = -1 (the other two 0) and the host raises.  A tile that fails still writes
// parent[g] = g for its cells, so later walks stay inside the plane.  Nothing waits for another
// workgroup: no flag is polled, no barrier spans workgroups.
#include "spgg_clusters_tiled.h"

#include "spgg_label_lds.h"

namespace spgg_clt {
namespace {

using namespace spgg_obs;

constexpr int kSeamThreads = 256;

static_assert(kMaxTile * kMaxTile < (int)kDefector, "local labels must fit 16 bits beside the reserved value");

enum { F_FAIL = 0 };                   // flag words of a replica
enum { W_COUNT = 8 };                  // workgroup-shared words of the tile pass (the labelling pass's)

__device__ __forceinline__ int32_t aload(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t amin(int32_t* p, int32_t v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void set_fail(int32_t* flags) {
  __hip_atomic_fetch_or(flags + F_FAIL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root a walk from x reaches, halving the path on the way (parent[x] = its grandparent).
// Every step goes to a smaller index; at most n steps.  Always returns an index inside the plane.
__device__ __forceinline__ int find_root(int32_t* parent, int x, int n, int32_t* flags) {
  for (int k = 0; k < n; ++k) {
    const int p = aload(parent + x);
    if ((uint32_t)p > (uint32_t)x) break;   // not a parent word: ends below in the failure
    if (p == x) return x;
    const int gp = aload(parent + p);
    if ((uint32_t)gp > (uint32_t)p) break;
    if (gp == p) return p;
    amin(parent + x, gp);
    x = gp;
  }
  set_fail(flags);
  return x;
}

__global__ void spgg_clusters_tiled_init_kernel(int n_rep, long long words, long long n, int32_t* __restrict__ work,
                                                int32_t* __restrict__ rec, long long rec_stride) {
  const int rep = blockIdx.x * blockDim.x + threadIdx.x;
  if (rep >= n_rep) return;
  int32_t* flags = work + rep * words + 2 * n;
  for (int k = 0; k < kFlagWords; ++k) flags[k] = 0;
  int32_t* out_rec = rec + rep * rec_stride;
  out_rec[0] = out_rec[1] = out_rec[2] = 0;
}

// kSide: the largest tile side this instance holds in LDS (two 16-bit planes of kSide^2 cells).
template <int kSide>
__global__ __launch_bounds__(kThreads) void spgg_clusters_tiled_tile_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L,
    int t, int tile, int ntx, int32_t* __restrict__ work, long long words) {
  constexpr int kCells = kSide * kSide;
  static_assert(kCells % 2 == 0, "two labels per LDS word");
  __shared__ uint32_t label[kCells / 2];
  __shared__ uint32_t ref[kCells / 2];
  __shared__ uint32_t sh[W_COUNT];

  const int n = L * L;
  const int rep = blockIdx.y;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int x0 = tx * tile, y0 = ty * tile;
  if (tile > kSide || x0 >= L || y0 >= L) return;   // (the host launches neither)
  const int tw = min(tile, L - x0), th = min(tile, L - y0);
  const int m = tw * th;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  int32_t* parent = work + rep * words;
  int32_t* count = parent + n;
  int32_t* flags = count + n;

  if (tid < W_COUNT) sh[tid] = 0u;
  for (int l = tid; l < m; l += nthr) {
    const int ly = l / tw, lx = l - ly * tw;
    const int g = (y0 + ly) * L + x0 + lx;
    set_half(label, l, (plane[g] & 1) ? kDefector : (uint32_t)l);   // bit 0 only: 0 = cooperator
    set_half(ref, l, (uint32_t)l);
  }
  __syncthreads();
  const bool converged = label_region(label, ref, sh, tw, th, false);   // the tile edge is a wall
  if (!converged && tid == 0) set_fail(flags);   // the pass cap (or an unreachable loop cap)

  for (int l = tid; l < m; l += nthr) {
    const int ly = l / tw, lx = l - ly * tw;
    const int g = (y0 + ly) * L + x0 + lx;
    const uint32_t lb = half_of(label, l);
    int p = g;
    if (converged && lb != kDefector && lb <= (uint32_t)l) {   // lb <= l < m always; the test keeps p <= g
      const int ry = (int)lb / tw, rx = (int)lb - ry * tw;
      p = (y0 + ry) * L + x0 + rx;
    }
    parent[g] = p;
    count[g] = 0;
  }
}

// Pairs of a replica: seam s = 0 .. nseam-1 between tile columns (s < nseam: cells (y, xa) and
// (y, xb)), then the same between tile rows; the last seam of each direction is the lattice edge
// when periodic.
__global__ __launch_bounds__(kSeamThreads) void spgg_clusters_tiled_seam_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L,
    int t, int tile, int ntx, int periodic, int32_t* work, long long words) {
  const int n = L * L;
  const int rep = blockIdx.y;
  const int nseam = ntx - 1 + periodic;
  const long long pairs = 2LL * nseam * L;
  const long long p = (long long)blockIdx.x * kSeamThreads + threadIdx.x;
  if (p >= pairs) return;
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  int32_t* parent = work + rep * words;
  int32_t* flags = parent + 2LL * n;

  const int dir = p >= (long long)nseam * L;   // 0: between columns, 1: between rows
  const int q = (int)(p - (long long)dir * nseam * L);
  const int s = q / L, along = q - s * L;
  const int ca = s < ntx - 1 ? (s + 1) * tile - 1 : L - 1;   // the coordinate across the seam, before it
  const int cb = s < ntx - 1 ? ca + 1 : 0;                   // and after it
  int a = dir ? ca * L + along : along * L + ca;
  int b = dir ? cb * L + along : along * L + cb;
  if (a == b || (plane[a] & 1) || (plane[b] & 1)) return;

  for (int k = 0; k < kMaxRetries; ++k) {
    const int ra = find_root(parent, a, n, flags), rb = find_root(parent, b, n, flags);
    if (ra == rb) return;
    const int hi = max(ra, rb), lo = min(ra, rb);
    const int old = amin(parent + hi, lo);
    if (old == hi) return;                       // hi was a root: linked
    if ((uint32_t)old > (uint32_t)hi) break;     // not a parent word
    a = old;                                     // hi had been linked to old < hi first: the word now
    b = lo;                                      // holds min(old, lo); old and lo are still to be united
  }
  set_fail(flags);
}

__global__ __launch_bounds__(kThreads) void spgg_clusters_tiled_count_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L,
    int t, int32_t* work, long long words) {
  __shared__ int wave_root[kThreads / 64];
  __shared__ int wave_count[kThreads / 64];
  const int n = L * L;
  const int rep = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long gl = (long long)blockIdx.x * kThreads + tid;
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  int32_t* parent = work + rep * words;
  int32_t* count = parent + n;
  int32_t* flags = count + n;

  const bool c = gl < n && !(plane[gl] & 1);
  const int r = c ? find_root(parent, (int)gl, n, flags) : -1;
  // the lanes that share the first cooperator's root add once (a large cluster is most of a wave)
  const unsigned long long any = __ballot(c);
  int first = -1, shared = 0;
  if (any != 0ull) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)any) - 1);
    first = __builtin_amdgcn_readlane(r, leader);
    const bool same = c && r == first;
    shared = __popcll(__ballot(same));
    if (c && !same) atomicAdd(count + r, 1);
  }
  if (lane == 0) {
    wave_root[wave] = first;
    wave_count[wave] = shared;
  }
  __syncthreads();
  // and the waves that share the first wave root add once per workgroup
  if (tid == 0) {
    const int nw = blockDim.x >> 6;
    int ref_root = -1, sum = 0;
    for (int w = 0; w < nw; ++w) {
      const int wr = wave_root[w];
      if (wr < 0) continue;
      if (ref_root < 0) ref_root = wr;
      if (wr == ref_root) sum += wave_count[w];
      else atomicAdd(count + wr, wave_count[w]);
    }
    if (ref_root >= 0) atomicAdd(count + ref_root, sum);
  }
}

__global__ __launch_bounds__(kThreads) void spgg_clusters_tiled_record_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, int L,
    int t, const int32_t* __restrict__ work, long long words, int32_t* __restrict__ sizes, int32_t* __restrict__ rec,
    long long rec_stride) {
  __shared__ int sh[3];   // {clusters, largest, bonds} of this workgroup
  const int n = L * L;
  const int rep = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const long long gl = (long long)blockIdx.x * kThreads + tid;
  const uint8_t* plane = observed_plane(S0, S1, stop_iter, rep, t) + (size_t)rep * n;
  const int32_t* parent = work + rep * words;
  const int32_t* count = parent + n;
  const int32_t* flags = count + n;
  int32_t* out_rec = rec + rep * rec_stride;

  if (tid < 3) sh[tid] = 0;
  __syncthreads();
  int nclu = 0, largest = 0, bonds = 0;
  if (gl < n) {
    const int g = (int)gl;
    const int y = g / L, x = g - y * L;
    const int d = plane[g] & 1;
    // C-D bonds, always periodic: sum(S != roll(S,1,0)) + sum(S != roll(S,1,1))
    const int up = (y > 0 ? g : g + n) - L, left = x > 0 ? g - 1 : g + L - 1;
    bonds = (d != (plane[up] & 1)) + (d != (plane[left] & 1));
    int sz = 0;
    if (!d && parent[g] == g) {   // a root: the cluster's smallest raster index
      sz = count[g];
      nclu = 1;
      largest = sz;
    }
    if (sizes) sizes[(size_t)rep * n + g] = sz;
  }
  for (int off = 32; off > 0; off >>= 1) {   // lane 0's total only (fewer instructions than wave_sum's butterfly)
    nclu += __shfl_down(nclu, off, 64);
    bonds += __shfl_down(bonds, off, 64);
    largest = max(largest, __shfl_down(largest, off, 64));
  }
  if (lane == 0) {
    if (nclu) atomicAdd(&sh[0], nclu);
    if (largest) atomicMax(&sh[1], largest);
    if (bonds) atomicAdd(&sh[2], bonds);
  }
  __syncthreads();
  if (tid != 0) return;
  if (flags[F_FAIL]) {   // (set in an earlier launch) a cap was reached: the record is an error
    if (blockIdx.x == 0) {
      out_rec[0] = -1;
      out_rec[1] = 0;
      out_rec[2] = 0;
    }
    return;
  }
  if (sh[0]) atomicAdd(out_rec + 0, sh[0]);
  if (sh[1]) atomicMax(out_rec + 1, sh[1]);
  if (sh[2]) atomicAdd(out_rec + 2, sh[2]);
}

template <int kSide>
void launch_tiles(dim3 grid, int threads, hipStream_t s, const Lattices& lat, int t, int tile, int ntx, int32_t* work,
                  long long words) {
  hipLaunchKernelGGL(spgg_clusters_tiled_tile_kernel<kSide>, grid, dim3(threads), 0, s, lat.S0, lat.S1, lat.stop_iter,
                     lat.L, t, tile, ntx, work, words);
}

}  // namespace

void launch(const spgg_obs::Lattices& lat, int t, int periodic, int tile, int32_t* work, int32_t* sizes, int32_t* rec,
            int64_t rec_stride, hipStream_t s) {
  const uint8_t *S0 = lat.S0, *S1 = lat.S1;
  const int32_t* stop_iter = lat.stop_iter;
  const int n_rep = lat.n_rep, L = lat.L;
  const long long n = lat.cells();
  const long long words = workspace_words(n);
  const int ntx = (L + tile - 1) / tile;
  periodic = periodic ? 1 : 0;
  hipLaunchKernelGGL(spgg_clusters_tiled_init_kernel, dim3((n_rep + 63) / 64), dim3(64), 0, s, n_rep, words, n, work, rec,
                     (long long)rec_stride);
  // the smallest LDS instance that holds the tile: 4, 16, 64 or 156 KiB per workgroup
  const int side = tile < L ? tile : L;   // (a tile wider than the lattice holds L x L cells)
  const int cells = side * side;
  const int threads = cells >= kThreads ? kThreads : ((cells + 63) / 64) * 64;   // whole waves
  const dim3 tiles(ntx * ntx, n_rep);
  if (side <= 32) launch_tiles<32>(tiles, threads, s, lat, t, side, ntx, work, words);
  else if (side <= 64) launch_tiles<64>(tiles, threads, s, lat, t, side, ntx, work, words);
  else if (side <= 128) launch_tiles<128>(tiles, threads, s, lat, t, side, ntx, work, words);
  else launch_tiles<kMaxTile>(tiles, threads, s, lat, t, side, ntx, work, words);
  const long long pairs = 2LL * (ntx - 1 + periodic) * L;
  if (pairs > 0)   // (one tile with walls has no seam: decided by the arguments, never by the data)
    hipLaunchKernelGGL(spgg_clusters_tiled_seam_kernel, dim3((unsigned)((pairs + kSeamThreads - 1) / kSeamThreads), n_rep),
                       dim3(kSeamThreads), 0, s, S0, S1, stop_iter, L, t, side, ntx, periodic, work, words);
  const dim3 cells_grid((unsigned)((n + kThreads - 1) / kThreads), n_rep);
  hipLaunchKernelGGL(spgg_clusters_tiled_count_kernel, cells_grid, dim3(kThreads), 0, s, S0, S1, stop_iter, L, t, work,
                     words);
  hipLaunchKernelGGL(spgg_clusters_tiled_record_kernel, cells_grid, dim3(kThreads), 0, s, S0, S1, stop_iter, L, t,
                     (const int32_t*)work, words, sizes, rec, (long long)rec_stride);
}

}  // namespace spgg_clt
