// spgg_mt_gen.hip — the device MT19937 draw generator (gfx950): spgg_mt_gen_kernel,
// spgg_mt_final_kernel and their launches (spgg_draws.h).  The jump-ahead that starts its
// chains is spgg_mt.hip.
//
// Device MT19937, bit-identical to numpy.random.RandomState (legacy seeding,
// randomkit mt19937_gen + tempering), generating the draw records of whole
// chunks of iterations ahead of the step kernels (spgg_step runs it on its own
// stream; the draws depend on nothing but the key and the eps schedule).
//
// The raw word stream obeys x[k+624] = x[k+397] ^ twist(x[k], x[k+1]), so the 227
// words of a block [F, F+227) depend only on words >= 227 back: block-parallel.
// One workgroup per chain, no barrier after the prologue:
//   wave 0, the recurrence: the 227 positions of a block in 4 slots of lanes
//     (gen_slot_base), x[F+j] from x[F+j-227] (the lane's previous word of the slot, a
//     register) and x[F+j-624], x[F+j-623] (the LDS ring, 2-3 blocks old; read one block
//     ahead).  It publishes its completed blocks (gen_done) every kGenPub blocks; one
//     wave's LDS operations complete in order.  The ring holds kGenNB blocks at fixed positions
//     (block b at kGenPitch * (b % kGenNB), kGenPitch = 227: no padding; + a mirror of block 0
//     behind the last one), so with the block loop unrolled kGenNB
//     times every LDS address is a lane constant plus an immediate offset, and no LDS
//     operation of the recurrence sits under a branch;
//   the other kGenOut waves: temper + threshold + pack the finished words (below the
//     frontier 624 + 227*min(gen_done)): 64 draws per wave instruction, one __ballot, two
//     32-bit stores -- the draw record holds one BIT per draw (spgg_abi.h).  They publish
//     the first word they still need (gen_need), which the recurrence must not overwrite.
// Per executed iteration the reference draws rand(L,L) (2 words per double,
// algorithms.py:105) then randint(0,2,(L,L)) (1 word each, algorithms.py:108);
// SARSA twice more (spgg.py:434, 452), Double-Q then rand(L,L) < 0.5
// (algorithms.py:307).  After each iteration the key (the 624-word block holding
// the last consumed word, + pos) is saved to a snapshot ring, from which
// spgg_flush restores the key the reference would hold (spgg_mt_final_kernel).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "spgg_abi.h"
#include "spgg_device.h"
#include "spgg_draws.h"
#include "spgg_mt.h"

using namespace spgg;
using namespace spgg_gen;

namespace {

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}

using spgg_mt::mt_next;

// bit 0 of mt_temper(y) as a function of y: y0 ^ y3 ^ y14 ^ y18 ^ y22 ^ y29 (the tempering
// shifts and masks of mt_temper composed; tests/test_mt_jump_cpu.py checks it on numpy)
constexpr uint32_t kTemperBit0 = 0x20444009u;

// One recurrence wave and three output waves per chain: the A/B variants of this layout
// (2 recurrence waves, 1-3 output waves, publication periods, wave priorities, VGPR caps,
// timing ablations) were measured in round 3 and live in profiles/r03/rejected_gen_knobs.patch.
#ifndef SPGG_GEN_OUT
#define SPGG_GEN_OUT 3
#endif
constexpr int kGenOut = SPGG_GEN_OUT;            // output waves
constexpr int kGenSPW = 4;                       // slots of the lone recurrence wave
// Blocks between two progress publications of the recurrence wave (each publication waits
// for the wave's LDS writes: one exposed LDS round trip per period).
constexpr int kGenPub = 4;

// Chunks an output wave handles per batch (one wait, one need publication, one store of the
// batch's draw words; the ring coordinates stepped, not divided, from one chunk to the next).
constexpr int kGenU = 4;
constexpr int kGenThreads = 64 * (1 + kGenOut);
constexpr int kMtBlock = 227;                    // 624 - 397: words one dependency step produces
// Ring words per block: none of padding, so a chunk's words are contiguous across a block
// boundary (and into the mirror of block 0 past the last block): one lane address per read.
constexpr int kGenPitch = kMtBlock;
// Ring blocks.  Not a lever: 8 or 12 (10 / 14 KB of LDS instead of 18) measured the same whole runs
// (profiles/r04/generator_groups.txt) -- with the generator resident, the step kernel's occupancy
// is bound by VGPRs, not LDS.
#ifndef SPGG_GEN_NB
#define SPGG_GEN_NB 16
#endif
constexpr int kGenNB = SPGG_GEN_NB;
static_assert(kGenNB == 16 || kGenNB == 8, "the block loop is unrolled kGenNB times");
static_assert(kGenNB % kGenPub == 0, "publication period divides the unrolled block loop");
// an output wave reads at most kGenU x kGenOut x 128 - 1 words past its published need (a batch);
// the frontier it is guaranteed to see lies (kGenNB - kGenPub) x 227 + 1 words past the smallest need
static_assert(kGenU * kGenOut * 128 - 1 < (kGenNB - kGenPub) * kMtBlock + 1, "output waves' progress");
constexpr int kGenRingWords = kGenPitch * kGenNB;
constexpr int kGenRing = kGenRingWords + kGenPitch;  // + a mirror of block 0 behind the last one
// Progress a failed recurrence wave publishes: every output wave's wait then ends at once.
constexpr uint32_t kGenDoneAbort = (0xffffffffu - 624u) / kMtBlock;
// Bound of every wait loop between the generator's waves (0.2-0.5 s of s_sleep): a wait that
// long means a defect.  The wave then records SPGG_GEN_ERR_SPIN in the context's error word,
// which spgg_flush / spgg_status report (SPGG_E_STATE: the draws of such a run are not the
// reference's), releases the other waves (need 0xffffffff / progress kGenDoneAbort) and
// stops, so the kernel ends instead of hanging the GPU.  (The recurrence wave stops through its
// last-block path: an early return there took the kernel from 51 to 74 VGPRs.)
constexpr uint32_t kGenSpinMax = 1u << 23;
#ifndef SPGG_GEN_SLEEP_OUT  // s_sleep argument of a polling output wave (x 64 clocks)
#define SPGG_GEN_SLEEP_OUT 1
#endif
#ifndef SPGG_GEN_SLEEP_REC  // s_sleep argument of the recurrence wave waiting for the output waves
#define SPGG_GEN_SLEEP_REC 2
#endif

// The 227 positions of a block in 4 slots of 64 lanes: slot s holds positions
// base(s) + lane for lane < len(s).  Positions 169-226 need positions 0-57 of the block two
// back (every other position only blocks three back), so slots 0 and 1 -- the same wave --
// hold both: a wave reads another wave's words only from blocks >= 2 behind, which leaves
// each wave a block of slack.  The lanes past len(s) (29 = 256 - 227 of them) DUPLICATE lane
// (lane - len(s)) of their slot -- the same position, operands and previous word, so they compute
// and write the same value to the same address -- so every LDS write is unconditional and the
// ring has no padding.
__host__ __device__ constexpr int gen_slot_base(int s) { return s == 0 ? 0 : s == 1 ? 169 : s == 2 ? 58 : 122; }
__host__ __device__ constexpr int gen_slot_len(int s) { return s == 0 ? 58 : s == 1 ? 58 : s == 2 ? 64 : 47; }
__device__ __forceinline__ int gen_position(int s, int lane) {
  return gen_slot_base(s) + (lane < gen_slot_len(s) ? lane : lane - gen_slot_len(s));
}

// A wait between the generator's waves ran out of its bound: recorded for the host (one lane,
// a vector global atomic).
__device__ __forceinline__ void gen_fail(const GenArgs& g) {
  if ((threadIdx.x & 63) == 0) atomicOr(g.err, (uint32_t)SPGG_GEN_ERR_SPIN);
}

// Flags shared through LDS between the generator's waves: relaxed workgroup-scope atomics
// on the __shared__ array itself (plain ds_read / ds_write; through a generic pointer they
// become flat accesses with system-scope waits).  Every lane of a wave writes its own copy
// (no branch around the store); readers read lane 0's.  A flag store is a release: it waits
// until every earlier LDS access of the wave has completed (lgkmcnt(0); issue order alone
// does not order another wave's view of two writes), and the compiler may not move an
// access across it; a reader only touches the ring after its flag read returned.
#define LDS_LD(x) __hip_atomic_load(&(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
// after a wait on a flag: no memory access of the wave may be moved above the wait by the
// compiler (relaxed atomics do not order the plain ring accesses; the hardware does)
#define GEN_FENCE() asm volatile("" ::: "memory")
#define LDS_ST(x, v)                                                          \
  do {                                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                        \
    __hip_atomic_store(&(x), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
  } while (0)

// Word k of a launch (the key block = words 0..623) lives in ring block (k + 57) / 227 - 3
// (mod kGenNB), at offset (k + 57) % 227: blocks b >= 0 hold words 624 + 227 b ..
// (blocks are contiguous, so that is ring position (k - 624) mod kGenRingWords)
__device__ __forceinline__ uint32_t gen_word_pos(uint32_t k) {
  static_assert(kGenPitch == kMtBlock, "contiguous ring blocks");
  return (k + (uint32_t)(kGenRingWords - 624)) % (uint32_t)kGenRingWords;
}

// Iterations t0..t1 of every replica, from its key; writes the draw records, the key
// snapshots (slot t % snap_slots = the key after iteration t; t0 == 1 also slot 0 = the
// initial key) and the advanced key.  blockIdx.x = rep * chains + c: chain c runs
// iterations t0 + c*per_chain .. (+ per_chain - 1) from its window -- chain 0 from key_in
// (an aligned key block + pos), chain c >= 1 from the XOR of its parts: the window that
// starts at its first draw word, whose offset within the reference's 624-word key blocks
// is ph.  Word indices are relative to the chain's window (the host keeps a chain below
// 2^31 words).  skip_stopped: replicas already absorbed are left alone (their draws are
// never read).
__global__ __launch_bounds__(kGenThreads) void spgg_mt_gen_kernel(GenArgs g, int t0, int t1, int skip_stopped) {
  __shared__ uint32_t ring[kGenRing];
  __shared__ uint32_t gen_done[64];           // blocks the recurrence wave has published (per lane)
  __shared__ uint32_t gen_need[kGenOut][64];  // output wave w reads no word below this (per lane)
  __shared__ uint32_t pos_sh;
  const int rep = blockIdx.x / g.chains, ch = blockIdx.x - rep * g.chains, tid = threadIdx.x;
  bool last_chain;  // the chain whose iterations end the launch: it writes key_out
  {
    const int ct0 = t0 + ch * g.per_chain;
    if (ct0 > t1) return;
    last_chain = ct0 + g.per_chain - 1 >= t1;
    t1 = min(t1, ct0 + g.per_chain - 1);
    t0 = ct0;
  }
  if (skip_stopped && g.stop_iter[rep] != 0) return;
  const int planes = draw_planes(g.alg);
  const uint32_t W = (uint32_t)draw_mt_words(g.n, planes);
  uint32_t ph = 0;  // offset of the window's first word within a key block
  if (ch == 0) {
    const uint32_t* key = g.key_in + (size_t)rep * 625;
    for (int i = tid; i < 624; i += kGenThreads) ring[gen_word_pos(i)] = key[i];
    if (tid == 0) pos_sh = key[624];  // next word to consume (624: the block is exhausted)
    if (t0 == 1) {
      uint32_t* s0 = g.snap + (size_t)rep * 625;
      for (int i = tid; i < 625; i += kGenThreads) s0[i] = key[i];
    }
  } else {
    const uint32_t* pp = g.parts + (size_t)(rep * g.chains + ch) * spgg_mt::kSplits * 624;
    for (int i = tid; i < 624; i += kGenThreads) {
      uint32_t v = 0;
#pragma unroll
      for (int p = 0; p < spgg_mt::kSplits; ++p) v ^= pp[p * 624 + i];
      ring[gen_word_pos(i)] = v;
    }
    if (tid == 0) pos_sh = 0;
    ph = (uint32_t)(((uint64_t)g.run_pos0[rep] + (uint64_t)(t0 - 1) * W) % 624u);
  }
  if (tid < 64) gen_done[tid] = 0;
  if (tid < 64 * kGenOut) gen_need[tid >> 6][tid & 63] = 0;
  __syncthreads();
  const uint32_t pos0 = pos_sh;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  // first word of the key block holding word E - 1 (window-relative; >= 0: W >= 624 for chains)
  auto key_block = [ph](uint32_t E) { return ((E - 1 + ph) / 624) * 624 - ph; };
  // blocks of 227 words this launch generates: through the key block of its last iteration
  uint32_t nblk;
  {
    const uint32_t E_last = pos0 + (uint32_t)(t1 - t0 + 1) * W;
    const uint32_t target_last = key_block(E_last) + 624;
    nblk = target_last > 624 ? (target_last - 624 + kMtBlock - 1) / kMtBlock : 0;
  }
  if (wave == 0) {
    // ---- the recurrence: every slot of every block ------------------------------------------
    __builtin_amdgcn_s_setprio(3);  // the critical path
    uint32_t prev[kGenSPW], ca[kGenSPW], cb[kGenSPW];
    uint32_t *wp[kGenSPW], *pa[kGenSPW], *pb[kGenSPW];  // lane addresses: own word, its two operands
#pragma unroll
    for (int i = 0; i < kGenSPW; ++i) {
      const int j = gen_position(i, lane);
      wp[i] = ring + j;
      pa[i] = ring + j + 57;  // (a word past 227 is the next block's: contiguous ring)
      pb[i] = ring + j + 58;
      prev[i] = wp[i][(kGenNB - 1) * kGenPitch];  // x[397 + j]: block -1
      ca[i] = pa[i][(kGenNB - 3) * kGenPitch];    // operands of block 0: block -3
      cb[i] = pb[i][(kGenNB - 3) * kGenPitch];
    }
    uint32_t E = pos0 + W;
    uint32_t mb = key_block(E), target = mb + 624;
    uint32_t lim = 0;   // largest F whose block may be written (output waves' reads)
    int t = t0;
    uint32_t key_mb = 0, key_pos = pos0;
    uint32_t b = 0;     // blocks completed
    bool aborted = false;  // a flow-control wait ran out of its bound
    // key after iteration t (words [mb, mb+624) and pos), to the snapshot ring; then the next
    auto retire = [&]() {
      uint32_t* sn = g.snap + (size_t)(t % g.snap_slots) * g.snap_stride + (size_t)rep * 625;
#pragma unroll 1
      for (int m = 0; m < 10; ++m) {
        const uint32_t i = lane + 64 * m;
        if (i < 624) sn[i] = ring[gen_word_pos(mb + i)];
      }
      if (lane == 0) sn[624] = E - mb;
      key_mb = mb;
      key_pos = E - mb;
      ++t;
      E += W;
      mb = key_block(E);
      target = mb + 624;
    };
    // one block: b % kGenNB == U; operands ca/cb were read one block ahead
#define SPGG_GEN_BLOCK(U)                                                                                 \
  {                                                                                                       \
    if (b == nblk) goto rec_done;                                                                         \
    while (t <= t1 && 624u + kMtBlock * b >= target) retire();                                            \
    const uint32_t F = 624u + kMtBlock * b;                                                               \
    uint32_t spin = 0;                                                                                    \
    for (; F > lim && spin < kGenSpinMax; ++spin) { /* flow control: no output wave still reads the     \
                                                       positions written */                               \
      uint32_t m = 0xffffffffu;                                                                           \
      _Pragma("unroll") for (int w = 0; w < kGenOut; ++w) m = min(m, LDS_LD(gen_need[w][0]));             \
      m = __builtin_amdgcn_readfirstlane(m);                                                              \
      /* (saturating: finished output waves publish 0xffffffff) */                                       \
      lim = m > 0xffffffffu - (kGenNB - 1) * kMtBlock ? 0xffffffffu : m + (kGenNB - 1) * kMtBlock;        \
      if (F > lim) __builtin_amdgcn_s_sleep(SPGG_GEN_SLEEP_REC);                                          \
    }                                                                                                     \
    if (F > lim) { /* the bound ran out (the condition, not the counter: a last poll that succeeds    \
                      is no failure); this block is the last: rec_done publishes kGenDoneAbort */       \
      gen_fail(g);                                                                                        \
      aborted = true;                                                                                     \
      nblk = b + 1;                                                                                       \
    }                                                                                                     \
    GEN_FENCE();                                                                                          \
    uint32_t na[kGenSPW], nb[kGenSPW];                                                                    \
    _Pragma("unroll") for (int i = 0; i < kGenSPW; ++i) {                                                 \
      constexpr int rb = ((U + 1 + kGenNB - 3) % kGenNB) * kGenPitch;                                     \
      na[i] = pa[i][rb];                                                                                  \
      nb[i] = pb[i][rb];                                                                                  \
    }                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < kGenSPW; ++i) {                                                 \
      const uint32_t x = mt_next(prev[i], ca[i], cb[i]);                                                  \
      prev[i] = x;                                                                                        \
      wp[i][U * kGenPitch] = x;                                                                           \
      if (U == 0) wp[i][kGenNB * kGenPitch] = x; /* mirror of block 0 */                                  \
      ca[i] = na[i];                                                                                      \
      cb[i] = nb[i];                                                                                      \
    }                                                                                                     \
    ++b;                                                                                                  \
    if ((U + 1) % kGenPub == 0) LDS_ST(gen_done[lane], b);                                                \
  }
    for (;;) {
      SPGG_GEN_BLOCK(0) SPGG_GEN_BLOCK(1) SPGG_GEN_BLOCK(2) SPGG_GEN_BLOCK(3)
      SPGG_GEN_BLOCK(4) SPGG_GEN_BLOCK(5) SPGG_GEN_BLOCK(6) SPGG_GEN_BLOCK(7)
#if SPGG_GEN_NB == 16
      SPGG_GEN_BLOCK(8) SPGG_GEN_BLOCK(9) SPGG_GEN_BLOCK(10) SPGG_GEN_BLOCK(11)
      SPGG_GEN_BLOCK(12) SPGG_GEN_BLOCK(13) SPGG_GEN_BLOCK(14) SPGG_GEN_BLOCK(15)
#endif
    }
#undef SPGG_GEN_BLOCK
  rec_done:
    LDS_ST(gen_done[lane], aborted ? kGenDoneAbort : b);  // (published every kGenPub blocks: the rest)
    GEN_FENCE();
    while (t <= t1) retire();  // (the frontier covers every remaining target)
    if (last_chain) {
      uint32_t* key = g.key_out + (size_t)rep * 625;
      for (int i = lane; i < 624; i += 64) key[i] = ring[gen_word_pos(key_mb + i)];
      if (lane == 0) key[624] = key_pos;
    }
    return;
  }
  // ---- output waves: chunks ow, ow + kGenOut, ... of every plane of every iteration --------
  // (per chunk: one ring read per lane, the temper / parity, one ballot; per batch of kGenU
  // chunks: one wait, the batch's first word published as the wave's need, one store)
  const int ow = wave - 1;
  const uint64_t thr_half = u53_threshold(0.5);
  const int nchunk = (g.n + 63) / 64;
  uint32_t kpos = pos0;
  uint32_t seen = 624;  // the frontier as last read
  // lane 2u + h of a batch's store: half h of the draw word of the batch's chunk u
  // (the record's word of chunk c, plane p, half h: 2 c planes + h planes + p, spgg_abi.h)
  const uint32_t lane_off = (uint32_t)(((lane >> 1) * kGenOut * 2 + (lane & 1)) * planes);
  // the draws of the plane's last chunk (n % 64 of them when partial)
  const uint64_t tail = (g.n & 63) ? (1ull << (g.n & 63)) - 1ull : ~0ull;
  for (int t = t0; t <= t1; ++t) {
    const uint64_t thr = u53_threshold(g.eps[(size_t)rep * g.eps_slots + t]);
    uint32_t* rec_out = g.draws + (size_t)((t - 1) % g.draw_slots) * g.draw_stride + (size_t)rep * g.draw_words;
    for (int p = 0; p < planes; ++p) {
      const bool dbl = (p & 1) == 0;
      // rand() < th: ((a>>5) * 2^26 + (b>>6)) / 2^53 < th as a 53-bit integer compare, decided
      // by a alone unless its 27 bits equal th's (p = 2^-27: b is read only then)
      const uint64_t th = (g.alg == SPGG_ALG_DOUBLE_Q && p == 2) ? thr_half : thr;
      const uint32_t th_hi = __builtin_amdgcn_readfirstlane((uint32_t)(th >> 26));
      const uint32_t th_lo = __builtin_amdgcn_readfirstlane((uint32_t)th & ((1u << 26) - 1u));
      const uint32_t base = kpos + plane_word0((uint32_t)g.n, p);
      // (the chunk loop is instantiated per plane kind: the kind's branches leave the loop)
      auto chunks = [&](auto dbl_c) -> bool {
        constexpr bool dbl = decltype(dbl_c)::value;
        constexpr uint32_t wmul = dbl ? 2u : 1u;           // words per draw
        constexpr uint32_t cstep = 64u * wmul * kGenOut;    // words from one chunk of this wave to its next
        static_assert(cstep * kGenU < (uint32_t)kGenRingWords, "a batch stays within one turn of the ring");
        const uint32_t wlane = wmul * (uint32_t)lane;
        // the current chunk's first word and its ring position, stepped per chunk: word k sits at
        // (k - 624) mod kGenRingWords (gen_word_pos; the blocks are contiguous)
        uint32_t first = base + 64u * wmul * (uint32_t)ow;
        uint32_t rpos = gen_word_pos(first);
        for (int c = ow; c < nchunk; c += kGenOut * kGenU) {
          const int nb = min(kGenU, (nchunk - 1 - c) / kGenOut + 1);  // chunks of this batch
          const int cl = c + (nb - 1) * kGenOut;
          const uint32_t last = first + cstep * (uint32_t)(nb - 1) + wmul * (uint32_t)min(64, g.n - 64 * cl) - 1u;
          LDS_ST(gen_need[ow][lane], first);
          if (seen <= last) {  // wait for the recurrence (the check of its bound only on this path)
            uint32_t spin = 0;
            for (; seen <= last && spin < kGenSpinMax; ++spin) {
              seen = 624u + kMtBlock * __builtin_amdgcn_readfirstlane(LDS_LD(gen_done[0]));
              if (seen <= last) __builtin_amdgcn_s_sleep(SPGG_GEN_SLEEP_OUT);
            }
            if (seen <= last) {  // (the condition itself: a last poll that succeeds is no failure)
              gen_fail(g);
              LDS_ST(gen_need[ow][lane], 0xffffffffu);
              return false;
            }
          }
          GEN_FENCE();
          // the batch's words first (one LDS round trip; a chunk past the batch reads a ring word
          // it drops), then per chunk: the chunk's <= 128 words are contiguous from its ring position
          // (past the last block: the mirror of block 0)
          uint32_t rp[kGenU], x[kGenU];
#pragma unroll
          for (int u = 0; u < kGenU; ++u) {
            rp[u] = u == 0 ? rpos : rp[u - 1] + cstep;
            if (u > 0) rp[u] -= rp[u] >= (uint32_t)kGenRingWords ? (uint32_t)kGenRingWords : 0u;
            x[u] = ring[rp[u] + wlane];
          }
          uint32_t val = 0;
#pragma unroll
          for (int u = 0; u < kGenU; ++u) {
            if (u < nb) {
              bool flag;
              if (dbl) {
                const uint32_t ah = mt_temper(x[u]) >> 5;
                flag = ah < th_hi;
                if (ah == th_hi) flag = (mt_temper(ring[rp[u] + wlane + 1]) >> 6) < th_lo;
              } else {  // randint(0, 2) = the tempered word's low bit = parity of raw bits 0,3,14,18,22,29
                flag = (__builtin_popcount(x[u] & kTemperBit0) & 1) != 0;
              }
              // (lanes past n read stale words: masked)
              const uint64_t bits = __builtin_amdgcn_ballot_w64(flag) & (c + u * kGenOut == nchunk - 1 ? tail : ~0ull);
              val = lane == 2 * u ? (uint32_t)bits : lane == 2 * u + 1 ? (uint32_t)(bits >> 32) : val;
            }
          }
          rpos += cstep * (uint32_t)nb;
          rpos -= rpos >= (uint32_t)kGenRingWords ? (uint32_t)kGenRingWords : 0u;
          if (lane < 2 * nb) *at(rec_out, (uint32_t)(2 * c * planes + p) + lane_off) = val;
          first += cstep * (uint32_t)nb;
        }
        return true;
      };
      if (!(dbl ? chunks(std::true_type{}) : chunks(std::false_type{}))) return;
    }
    kpos += W;
  }
  LDS_ST(gen_need[ow][lane], 0xffffffffu);  // done: never blocks the recurrence
}

// spgg_flush (MT19937): the key the reference holds after the run -- after the last
// iteration a replica executed (its absorbing iteration draws nothing) -- from the ring.
__global__ void spgg_mt_final_kernel(GenArgs g, int t_last) {
  const int rep = blockIdx.x;
  const int st = g.stop_iter[rep];
  const int src = st ? st - 1 : t_last;
  const uint32_t* sn = g.snap + (size_t)(src % g.snap_slots) * g.snap_stride + (size_t)rep * 625;
  uint32_t* key = g.key_out + (size_t)rep * 625;
  for (int i = threadIdx.x; i < 625; i += blockDim.x) key[i] = sn[i];
}

}  // namespace

namespace spgg_gen {

void launch_gen(const GenArgs& g, int t0, int t1, int skip_stopped, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(spgg_mt_gen_kernel, dim3(blocks), dim3(kGenThreads), 0, s, g, t0, t1, skip_stopped);
}

void launch_final(const GenArgs& g, int t_last, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(spgg_mt_final_kernel, dim3(blocks), dim3(256), 0, s, g, t_last);
}

}  // namespace spgg_gen
