// spgg_correlations.h — cooperator pair counts of the strategy plane (spgg_correlations.hip).
//
// Nothing in the reference computes these.  A workgroup packs one replica's S_t into LDS, one
// bit per cell, and counts the cooperator pairs d apart along rows and along columns by
// AND + popcount over the packed rows; every workgroup owns its distances outright, so no
// workgroup waits for another and every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"
#include "spgg_observe.h"

namespace spgg_co {

constexpr int kWordBits = 32;   // one LDS word holds 32 cells of a row, cell x at bit x & 31
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// A wave owns one (direction, distance) pair, so a workgroup owns this many distances.
constexpr int kDistPerGroup = kWaves / 2;
// Rows a wave loads before it packs the first of them (loads in flight per wave).
constexpr int kPackDepth = 4;

// The packed lattice is all the LDS the kernel declares: L rows of ceil(L / 32) words.  Two
// instances: lattices of at most kSmallWords words share a CU, the rest may take all of it.
constexpr int kSmallWords = 2048;                 // 8 KiB: sides up to 256
constexpr int kFullWords = 163840 / 4;            // the 160 KiB one gfx950 workgroup may declare

constexpr int row_words(int L) { return (L + kWordBits - 1) / kWordBits; }
constexpr int lattice_words(int L) { return L * row_words(L); }   // non-decreasing in L

constexpr int max_side() {
  int L = 1;
  while (lattice_words(L + 1) <= kFullWords) ++L;
  return L;
}
// Largest lattice side (spgg_correlations_max_side): 1137 rows of 36 words = 163,728 B.
constexpr int kMaxSide = max_side();
static_assert(kMaxSide >= 1000, "cfg5 (L = 1000) must be supported");
static_assert(row_words(kMaxSide) <= 64, "a wave holds at least one whole row of words");
static_assert(2ll * kMaxSide * kMaxSide < (1ll << 31), "counts must fit int32");

// Enqueue the pair counts of every replica's S plane of iteration t (absorbed replicas: of their
// absorbing iteration) on `s`: replica k's rows[0..max_d], cols[0..max_d] at out + k*out_stride.
// 1 <= L <= kMaxSide and 0 <= max_d <= L / 2 (caller checks).
void launch(const spgg_obs::Lattices& lat, int t, int max_d, int32_t* out, int64_t out_stride, hipStream_t s);

}  // namespace spgg_co
