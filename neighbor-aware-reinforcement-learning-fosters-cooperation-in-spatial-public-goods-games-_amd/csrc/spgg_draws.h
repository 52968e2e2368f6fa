// spgg_draws.h — the draw record of the device MT19937 generator: the layout the generator
// (spgg_mt_gen.hip), the host (spgg_kernels.hip) and the tests agree on, and the generator's launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spgg_abi.h"

namespace spgg_gen {

// Draw program of one iteration, in the reference's order: plane i is rand(L,L)
// compared with a threshold (2 words per value, i even) or randint(0,2,(L,L))
// (1 word, i odd).
//   Q-learning / Expected SARSA: D(eps) I            (algorithms.py:105,108)
//   SARSA:   D(eps) I D(eps) I D(eps) I              (+ spgg.py:434, 452)
//   Double-Q: D(eps) I D(0.5)                        (+ algorithms.py:307)
__host__ __device__ inline int draw_planes(int alg) {
  return alg == SPGG_ALG_SARSA ? 6 : alg == SPGG_ALG_DOUBLE_Q ? 3 : 2;
}
// MT words one iteration consumes, and the first word of plane p within them.
__host__ __device__ inline int64_t draw_mt_words(int64_t n, int planes) { return n * (planes / 2 * 3 + (planes & 1) * 2); }
__host__ __device__ inline uint32_t plane_word0(uint32_t n, int p) { return n * (uint32_t)(p / 2 * 3 + (p & 1) * 2); }
// u32 words of one replica's draw record: 64-draw chunks (two words each) x planes.
__host__ __device__ inline int64_t draw_words_of(int n, int alg) {
  return (int64_t)((n + 63) / 64) * 2 * draw_planes(alg);
}

// What a generator launch reads and writes (the host fills it from its context).
struct GenArgs {
  const uint32_t* key_in;  // [rep][625] chain 0's key + pos: mt_state, or the chunk's key buffer
  uint32_t* key_out;       // [rep][625] the key after the launch's last iteration (its last chain)
  const uint32_t* parts;   // chains >= 1: start windows, [rep][chain][kSplits][624] XOR parts
  const uint32_t* run_pos0;  // [rep] first word of the run's iteration 1 in its key block
  int chains, per_chain;   // chain c: iterations t0 + c*per_chain .. (+ per_chain - 1)
  uint32_t* snap;          // snapshot slot s of replica rep: snap + s*snap_stride + rep*625
  int64_t snap_stride;
  int snap_slots;
  uint32_t* draws;         // draw record of iteration t: draws + ((t-1) % draw_slots)*draw_stride
  int64_t draw_stride;
  int draw_slots;
  int draw_words;          // per replica (draw_words_of)
  const double* eps;       // [rep][eps_slots]
  int eps_slots;
  const int* stop_iter;
  uint32_t* err;           // the context's error word (SPGG_GEN_ERR_*), OR-ed on a failed wait
  int n, alg;
};

// spgg_mt_gen_kernel: iterations t0 .. t1 of every replica, `blocks` = n_rep x g.chains workgroups.
void launch_gen(const GenArgs& g, int t0, int t1, int skip_stopped, int blocks, hipStream_t s);
// spgg_mt_final_kernel: the key after iteration t_last (or a replica's last executed one) into
// g.key_out, `blocks` = n_rep workgroups.
void launch_final(const GenArgs& g, int t_last, int blocks, hipStream_t s);

}  // namespace spgg_gen
