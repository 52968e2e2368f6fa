// spgg_clusters.h — cooperator-cluster labelling of the strategy plane (spgg_clusters.hip).
//
// Replaces the reference's final scipy.ndimage.label + per-label sums (src/model/spgg.py:631-633)
// and adds the same labelling as a per-iteration record.  One workgroup labels one replica with
// the whole lattice in LDS (label equivalence: scan / resolve / relabel until a scan changes
// nothing); no workgroup waits for another and every loop is bounded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_cl {

// Largest lattice side: 16-bit label + 16-bit ref per cell = 4 * 200 * 200 = 160,000 B of the
// 163,840 B one gfx950 workgroup may declare (spgg_clusters_max_side).
constexpr int kMaxSide = 200;
constexpr int kMaxCells = kMaxSide * kMaxSide;
// Pass cap (a pass = one scan): SPGG_CLUSTERS_MAX_PASSES, >= 4x what the NumPy model of this
// scheme needs on serpentines, spirals, rings and percolation-threshold noise at side 200
// (tests/test_clusters_model_cpu.py).
constexpr int kMaxPasses = SPGG_CLUSTERS_MAX_PASSES;
constexpr int kThreads = 1024;

// Enqueue the labelling of every replica's S plane of iteration t (absorbed replicas: of their
// absorbing iteration) on `s`.  sizes may be null (record only).  lat.L <= kMaxSide (caller checks).
void launch(const spgg_obs::Lattices& lat, int t, int periodic, int32_t* sizes, int32_t* rec, int64_t rec_stride,
            hipStream_t s);

}  // namespace spgg_cl
