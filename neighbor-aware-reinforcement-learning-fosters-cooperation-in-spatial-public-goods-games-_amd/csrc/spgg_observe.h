// spgg_observe.h — what every observer of the running lattice shares (spgg_clusters.hip,
// spgg_clusters_tiled.hip, spgg_correlations.hip, spgg_reputation.hip, spgg_dwell.hip): the
// lattices a launch reads, the rule for the plane that holds iteration t, the wave reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace spgg_obs {

// The leading arguments of every observer launch: the two strategy planes [n_rep][L * L], each
// replica's absorbing iteration (0: still running) and the batch's shape.
struct Lattices {
  const uint8_t *S0, *S1;
  const int32_t* stop_iter;
  int n_rep, L;
  long long cells() const { return (long long)L * L; }
};

// The iteration whose state an observer of iteration t sees in replica rep.  The launch of
// iteration j reads plane (j - 1) & 1 and writes plane j & 1, so S_t (and R_t) lies in plane
// (t - 1) & 1.  A replica absorbed at s = stop_iter[rep] != 0 is stepped no further: for t > s
// its state is still S_s, in the plane of s -- the other plane holds S_{s-1}.  A null stop_iter:
// no replica is absorbed.
__device__ __forceinline__ int observed_iter(const int32_t* stop_iter, int rep, int t) {
  const int stop = stop_iter ? stop_iter[rep] : 0;
  return (stop == 0 || stop >= t) ? t : stop;
}

// The one of a buffer's two planes that holds observed_iter; the caller adds its replica offset.
template <class T>
__device__ __forceinline__ const T* observed_plane(const T* P0, const T* P1, const int32_t* stop_iter, int rep, int t) {
  return ((observed_iter(stop_iter, rep, t) - 1) & 1) ? P1 : P0;
}

// The sum of v over the 64 lanes, in every lane (all lanes active).
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(std::is_integral<T>::value && (sizeof(T) == 4 || sizeof(T) == 8), "32- and 64-bit integers");
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

}  // namespace spgg_obs
