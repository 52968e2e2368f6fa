// spgg_policy.h — the learned policy field's record (spgg_policy.hip): per replica the counts of
// the four greedy-policy classes by strategy and state, the bonds between like and unlike classes,
// the histograms of the two action gaps, and the one-byte-per-agent plane they are made from.
//
// Nothing in the reference computes these (its only view of the Q tables are the twelve lattice
// means avg_q_* / cooperators_q_* / defectors_q_*, spgg.py:561-583).  The kernels read Q, S_t and
// the history record in place; no workgroup waits for another and every loop bound is known at
// launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_po {

constexpr int kMaxBins = 256;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// A workgroup observes one tile of kTileW x kTileH agents at a time, one agent per thread: a wave takes two
// tile rows, so its 16-byte Q rows are two runs of 512 contiguous bytes per state plane.
constexpr int kTileW = 32, kTileH = 8;
static_assert(kTileW * kTileH == kThreads, "one agent per thread");
// Workgroups of the policy kernel per replica: every one of them adds to the replica's row, so few
// enough that the same-address atomics do not queue (the history record's stripes hold theirs to
// 64 per address), enough that a batch of few replicas still fills the device (2048 workgroups:
// 8 per CU), at most 512 -- one replica of side 1000 then takes 8 tiles per workgroup.
constexpr int groups_per_replica(int tiles, int n_rep) {
  int g = (2048 + n_rep - 1) / n_rep;
  g = g < 64 ? 64 : g > 512 ? 512 : g;
  return tiles < g ? tiles : g;
}
// Cells one workgroup of the bond count pairs with their right and lower neighbours.
constexpr int kBondCells = 2048;

// int32 slots of one record row (spgg_abi.h): 16 counts, 4 + 1 bonds, 2 x 2 histograms of bins + 2.
constexpr int width(int bins) { return SPGG_POLICY_COUNTS + 4 * (bins + 2); }

// What the kernels read beside the lattices: the table in place, the history record that holds
// iteration t-1's GMAX, and whether the table in memory still lacks that iteration's NI term.
struct Tables {
  const double* Q;                // [n_rep][2][n][2], Double-Q [n_rep][2][n][4]
  const double* stats;            // [n_rep][stripes][slots][SPGG_NSTAT]
  const spgg_rep_params* params;
  int stripes, slots;
  bool double_q, second_order, action_state;
  bool unflushed;                 // no spgg_flush since the last step launch
};

// Enqueue the record of iteration t (absorbed replicas: of their absorbing iteration) on `s`: a
// launch that zeroes each replica's row, one whose workgroups take the replica's tiles, write the
// plane and add the counts and histograms, one that adds the bonds from the plane.  1 <= bins <= kMaxBins,
// out_stride >= width(bins), t - 1 < slots (caller checks).
void launch(const spgg_obs::Lattices& lat, const Tables& tb, int t, int bins, const double* edges, uint8_t* plane,
            int32_t* out, int64_t out_stride, hipStream_t s);

}  // namespace spgg_po
