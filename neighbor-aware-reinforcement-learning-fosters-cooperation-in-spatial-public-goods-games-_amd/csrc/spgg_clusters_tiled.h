// spgg_clusters_tiled.h — cooperator-cluster labelling of a strategy plane of any side, one
// replica spread over many workgroups (spgg_clusters_tiled.hip).
//
// What spgg_clusters.hip does for lattices up to side 200 in the LDS of one workgroup, for every
// side spgg_create accepts: square tiles labelled in LDS, then united across the tile edges in a
// global parent plane by a lock-free union (atomic minimum), counted per root and summed into the
// same three-value record.  Five launches on the caller's stream, always the same five; no
// workgroup waits for another and every loop is bounded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_clt {

// Tile sides a caller may ask for: local labels are 16 bits (as in spgg_clusters.hip), so a tile
// holds at most 200 x 200 cells; below 8 the seams outnumber the cells.
constexpr int kMinTile = 8;
constexpr int kMaxTile = 200;
// The library's choice (tile = 0): 16 KiB of LDS per workgroup, 256 workgroups for one L = 1000
// replica (the sides tried).
constexpr int kDefaultTile = 64;
// (Pass cap of the tile pass: SPGG_CLUSTERS_MAX_PASSES, spgg_label_lds.h.  A tile with its edge as
// a wall is a lattice of at most side 200, so the cap of spgg_clusters holds for it.)
// Retry cap of one seam union (a retry = an atomic minimum that met a word another workgroup had
// lowered first).  Every retry goes on with two indices below the word it lost, so the number of
// retries is bounded by the chain it descends, never by timing.
constexpr int kMaxRetries = SPGG_CLUSTERS_TILED_MAX_RETRIES;
constexpr int kThreads = 1024;

// Workspace of one replica in int32 words: the parent plane, the count plane and the flag words.
constexpr int kFlagWords = 8;
inline int64_t workspace_words(int64_t n) { return 2 * n + kFlagWords; }

// Enqueue the labelling of every replica's S plane of iteration t (absorbed replicas: of their
// absorbing iteration) on `s`: init, tile pass, seam pass, count, record.  8 <= tile <= 200
// (caller checks); work [n_rep][workspace_words(L * L)]; sizes may be null (record only).
void launch(const spgg_obs::Lattices& lat, int t, int periodic, int tile, int32_t* work, int32_t* sizes, int32_t* rec,
            int64_t rec_stride, hipStream_t s);

}  // namespace spgg_clt
