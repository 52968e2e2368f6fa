// spgg_label_lds.h — 4-connected cooperator clusters of a w x h region held in the LDS of one
// workgroup: the labelling pass of spgg_clusters.hip (the whole lattice) and of
// spgg_clusters_tiled.hip (one tile, its edge a wall).
//
// Method (label equivalence).  label[g] (16 bit; kDefector for S = 1) starts as the row-major
// index y*w + x of the first cell of the cell's row run of cooperators (its own index g for that
// first cell), ref[x] = x.  A pass is
//   scan     every cooperator takes the minimum label m among its cooperator neighbours; if
//            m < its own label `own` it lowers ref[own] to min(ref[own], m)
//   resolve  every representative x (label[x] == x) whose ref was lowered follows ref to its
//            end r (ref[r] == r) and stores label[x] = r
//   relabel  label[g] = label[label[g]] for every cooperator
// until a scan lowers nothing: then equal labels <=> same cluster, and a cluster's label is its
// smallest index (labels only ever decrease to labels of the same cluster, and a scan that
// changes nothing means no two neighbouring cooperators differ).
//
// Termination, from the code alone:
//   * ref[x] <= x always (a scan writes m < own into ref[own], or something smaller), so a
//     resolve chase is a strictly decreasing walk to the root; it takes a step only to a smaller
//     ref, so whatever the plane holds it ends within w*h steps and needs no counter;
//   * barriers separate scan, resolve and relabel.  A scan reads label and writes ref; resolve
//     reads ref and writes label[x] of its own representative only; relabel reads label[l] of
//     a representative l < w*h (any other label is left alone), which a concurrent relabel of l
//     itself can only overwrite with the same value (label[l] is a root r after resolve, and
//     label[r] == r);
//   * the 16-bit minimum is a compare-and-swap of the containing LDS word: a failed swap means
//     another thread strictly lowered one of the word's two halves, at most 2 * 65535 times
//     (the loop is capped there);
//   * the pass loop is capped at kMaxPasses; on the cap (or a capped swap, which cannot happen)
//     label_region returns false and the caller reports it;
//   * nothing waits for another workgroup or for global memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"

namespace spgg_obs {

constexpr uint32_t kDefector = 0xffffu;   // reserved label (a region has at most 40,000 cells)
constexpr int kSwapCap = 2 * 65536;
// Pass cap (a pass = one scan): >= 4x what the NumPy model of this scheme needs on serpentines,
// spirals, rings and percolation-threshold noise at side 200 (tests/test_clusters_model_cpu.py;
// DESIGN.md section 8).
constexpr int kMaxPasses = SPGG_CLUSTERS_MAX_PASSES;

// the first of the caller's workgroup-shared words belong to the pass
enum { W_CHANGED = 0, W_FAIL, W_LABEL_WORDS };

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

// Labels the w x h cells (row-major, w*h < kDefector) of the whole workgroup's region; the four
// neighbours beyond its edge are walls, or with `wrap` the cells of the opposite edge (a side of
// 1 or 2 then meets a cell itself or the same cell twice: the minimum does not mind).
// On entry label[g] = kDefector or g, ref[g] = g, sh[0 .. W_LABEL_WORDS) = 0, and a barrier has
// passed.  Returns whether the pass converged (workgroup-uniform); then, past the barrier it ends
// with, label[g] is the smallest index of g's cluster.
__device__ __forceinline__ bool label_region(uint32_t* label, uint32_t* ref, uint32_t* sh, int w, int h, bool wrap) {
  const int m = w * h;
  const int tid = threadIdx.x, nthr = blockDim.x;
  // every cooperator starts with the label of the first cell of its row run (one thread per
  // row, w steps): the first resolve then hops from run to run instead of from cell to cell.
  // A run's first cell keeps its own index, so the labels in use are still representatives.
  for (int y = tid; y < h; y += nthr) {
    uint32_t run = kDefector;
    for (int g = y * w; g < (y + 1) * w; ++g) {
      if (half_of(label, g) == kDefector) run = kDefector;
      else if (run == kDefector) run = (uint32_t)g;
      else set_half(label, g, run);
    }
  }
  __syncthreads();

  bool converged = false;
  for (int pass = 0; pass < kMaxPasses; ++pass) {
    // scan (reads label, lowers ref)
    bool lowered = false;
    for (int g = tid; g < m; g += nthr) {
      const uint32_t own = half_of(label, g);
      if (own == kDefector) continue;
      const int y = g / w, x = g - y * w;
      uint32_t mn = own;
      if (y > 0) mn = min(mn, half_of(label, g - w));
      else if (wrap) mn = min(mn, half_of(label, g + m - w));
      if (y < h - 1) mn = min(mn, half_of(label, g + w));
      else if (wrap) mn = min(mn, half_of(label, g - m + w));
      if (x > 0) mn = min(mn, half_of(label, g - 1));
      else if (wrap) mn = min(mn, half_of(label, g + w - 1));
      if (x < w - 1) mn = min(mn, half_of(label, g + 1));
      else if (wrap) mn = min(mn, half_of(label, g - w + 1));
      if (mn < own) lowered |= lower_ref(ref, (int)own, mn, &sh[W_FAIL]);
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
    for (int x = tid; x < m; x += nthr) {
      if (half_of(label, x) != (uint32_t)x) continue;
      uint32_t r = half_of(ref, x);
      if (r == (uint32_t)x) continue;
      for (uint32_t q; (q = half_of(ref, (int)r)) < r;) r = q;   // strictly decreasing: fewer than m steps
      set_half(label, x, r);
    }
    __syncthreads();
    if (tid == 0) sh[W_CHANGED] = 0u;   // (read above, before the barrier; next written after the next one)
    // relabel
    for (int g = tid; g < m; g += nthr) {
      const uint32_t l = half_of(label, g);
      if (l < (uint32_t)m) set_half(label, g, half_of(label, (int)l));   // (kDefector is not below m)
    }
    __syncthreads();
  }
  return converged;   // false: the pass cap (or an unreachable loop cap)
}

}  // namespace spgg_obs
