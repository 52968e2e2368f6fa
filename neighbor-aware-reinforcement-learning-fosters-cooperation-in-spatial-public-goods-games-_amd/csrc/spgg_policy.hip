// spgg_policy.hip — the learned policy field's record: what the agents' Q tables say they would do
// (its own object, like spgg_reputation.hip).
//
// Replaces: nothing in the reference on the device; its only view of the tables are the twelve
// lattice means of spgg.py:561-583.
//
// The table T an agent acts on at iteration t is the reference's self.q_table at the start of t.
// Between two step launches the Q buffer is not that table: it holds iteration t-1's TD update
// without its neighbour-influence term, which launch t's phase 1a (or spgg_flush) applies
// (spgg_abi.h, the Q row of the buffer table).  For a live replica at t > 1 with no flush enqueued
// since the last step the policy kernel therefore rebuilds the term exactly as phase 1a's
// recomputed record does -- always from the bits of S_t, whatever the operator or kernel family:
//   rew   = w_P * P(S_{t-1}) + w_rep * 0.5 * [a == 0]      S_{t-1} in bit 3, a in bit 0 of S_t
//   md    = max(0, max_k rew[nb_k] - rew)                   the 4 / 12 NI offsets
//   nu    = +-(kappa * md) / (gmax + lambda_eps)            sign: bit 2; gmax: stats[t-1][GMAX], max over stripes
//   T[s_old, a] = Q[s_old, a] + nu                          s_old: bit 1 (Double-Q: both tables, then their mean)
// -- the same f64 operations on the same operands, so T is the reference's table bit for bit.  An
// absorbed replica's table was persisted by its absorbing launch, a flushed one's by the flush; a
// replica with kappa == 0 has nu = +0: those read Q as it stands and stage nothing.
//
// Policy kernel.  Grid (groups_per_replica workgroups) x (replica); a workgroup takes the tiles
// of kTileW x kTileH agents blockIdx.x, blockIdx.x + gridDim.x, .. of its replica, one agent per
// thread, and adds to the replica's row once, after its last tile: every workgroup adds to the same
// few addresses, and same-address atomics of several thousand workgroups are what one replica of
// side 1000 waited for (measured: 128 us a round at one tile per workgroup).  A
// workgroup that rebuilds the term stages the S_t window of its tile + (M + 2) cells into LDS (the
// general modulus wraps tiny lattices), makes the rewards of tile + M ring in LDS as f64, then each
// thread reads its agent's two 16-byte Q rows (Double-Q: four) from the state planes -- agents
// contiguous across lanes -- adds the term by selects (an indexed row would go to scratch:
// DESIGN.md section 4), and derives
//   g_s = T[s,0] >= T[s,1] ? 0 : 1    c = g_0 + 2 g_1    gap_s = T[s,0] - T[s,1]
//   sigma = bit 0 of S    z = bit 4 of S (t' = 1: from R_1 = 0 -- reputation state 0, action state sigma == 0)
// The sixteen counts[c][sigma][z] go through ballots per wave, the gap bins through one LDS
// histogram per wave (slot 0: below edges[0], 1 .. bins: np.histogram's rule, bins + 1: above
// edges[bins]); the workgroup adds its non-zero slots to the replica's row with int32 atomics
// (exact, order-free) and stores the plane byte c | sigma << 2 | z << 3.
//
// Bond kernel.  Grid (chunk of kBondCells cells) x (replica): every cell of the plane is paired with
// its right and its lower neighbour on the periodic lattice (np.roll(., -1) on axis 1 and axis 0; at
// L <= 2 the aliased pairs count as they fall); a bond of two cells of class c counts in
// bonds_same[c], any other in bonds_mixed.  Ballots per wave, one atomic per non-zero slot.
#include "spgg_policy.h"

#include "spgg_device.h"

namespace spgg_po {
namespace {

using namespace spgg_obs;
using spgg::Cells13;
using spgg::div_uniform;
using spgg::max0_f64;
using spgg::max_f64;
using spgg::payoff13;

// ---- the helpers of the step kernel's phase 1a, restated (spgg_kernels.hip) -----------------

// the NI term of iteration t-1: lambda times +-1 by whether the best neighbour's action matched
__device__ __forceinline__ double pending_nu(uint8_t b, double md, double kappa, double lam_den, double lam_rcp) {
  const double lam = div_uniform(kappa * md, lam_den, lam_rcp);   // (kappa*max(0,md))/(gmax+eps)
  return ((b >> 2) & 1) ? lam : -lam;
}

// (s_old, a) entry index of iteration t-1 recorded in S_t bits 0-1
__device__ __forceinline__ int pending_entry(uint8_t b) { return ((b >> 1) & 1) * 2 + (b & 1); }

// max(0, max_k rew[nb_k] - rew[ca]): the maximum of the rounded differences is the rounded
// difference of the maximum (x -> RN(x - r0) is non-decreasing)
template <bool M2>
__device__ __forceinline__ double prev_max_diff(const double* rew, int ca, int w) {
  const double r0 = rew[ca];
  double m = max_f64(max_f64(rew[ca - w], rew[ca + w]), max_f64(rew[ca - 1], rew[ca + 1]));
  if constexpr (M2) {
    m = max_f64(m, max_f64(max_f64(rew[ca - 2 * w], rew[ca + 2 * w]), max_f64(rew[ca - 2], rew[ca + 2])));
    m = max_f64(m, max_f64(max_f64(rew[ca - w - 1], rew[ca - w + 1]), max_f64(rew[ca + w - 1], rew[ca + w + 1])));
  }
  return max0_f64(m - r0);
}

__device__ __forceinline__ int greedy2(double v0, double v1) { return v0 >= v1 ? 0 : 1; }   // np.argmax: ties -> 0
__device__ __forceinline__ double mean2(double x, double y) { return (x + y) * 0.5; }       // (q1 + q2) / 2

// ---- the record ---------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void spgg_policy_zero_kernel(int32_t* __restrict__ out, long long out_stride,
                                                                    int count) {
  for (int i = threadIdx.x; i < count; i += kThreads) out[(long long)blockIdx.x * out_stride + i] = 0;
}

// the slot of x among e[0 .. bins] (ascending): 0 below e[0], bins + 1 above e[bins], else 1 + the
// i with e[i] <= x < e[i + 1] (x == e[bins]: the last bin) -- spgg_reputation.hip's bin_of with the
// two outer slots; 9 halvings cover the 258 outcomes
__device__ __forceinline__ int slot_of(const double* e, int bins, double x) {
  int lo = 0, hi = bins + 1;   // lo ends as the number of edges <= x
#pragma unroll
  for (int it = 0; it < 9; ++it) {
    if (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
  }
  if (lo == bins + 1) return x == e[bins] ? bins : bins + 1;
  return lo;   // 0: below e[0]; else bin lo - 1, slot lo
}

template <bool M2, bool QB>
__global__ __launch_bounds__(kThreads) void spgg_policy_kernel(
    const uint8_t* __restrict__ S0, const uint8_t* __restrict__ S1, const int32_t* __restrict__ stop_iter, Tables tb,
    int L, int tiles_x, int tiles, int t, int bins, const double* __restrict__ edges, uint8_t* __restrict__ plane,
    int32_t* __restrict__ out, long long out_stride) {
  constexpr int M = M2 ? 2 : 1;
  constexpr int HS = M + 2;                                     // the payoff of a ring cell reads two cells further
  constexpr int RW = kTileW + 2 * M, RH = kTileH + 2 * M;       // the reward region: tile + M ring
  constexpr int SW = kTileW + 2 * HS, SH = kTileH + 2 * HS;     // the S window
  __shared__ uint8_t sS[SW * SH];
  __shared__ double sRew[RW * RH];
  __shared__ double tab[12];
  __shared__ double sE[kMaxBins + 1];
  __shared__ uint32_t h[kWaves][4 * (kMaxBins + 2)];
  __shared__ uint32_t cnt[16];

  if (bins < 1 || bins > kMaxBins) return;   // (the host refuses these: spgg_policy)
  const int rep = blockIdx.y;
  const size_t n = (size_t)L * L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int stop = stop_iter ? stop_iter[rep] : 0;
  const int tt = observed_iter(stop_iter, rep, t);
  const uint8_t* sp = (((tt - 1) & 1) ? S1 : S0) + (size_t)rep * n;   // n bytes apart: unaligned for odd L
  const spgg_rep_params& pg = tb.params[rep];
  const double kappa = pg.kappa;
  // the table in memory lacks iteration t-1's NI term (workgroup-uniform); kappa == 0: the term is +0
  const bool ni = tb.unflushed && stop == 0 && t > 1 && kappa != 0.0;
  const int hw = 4 * (bins + 2);

  for (int i = tid; i <= bins; i += kThreads) sE[i] = edges[(size_t)rep * (bins + 1) + i];
  for (int i = tid; i < kWaves * hw; i += kThreads) h[i / hw][i - (i / hw) * hw] = 0u;
  if (tid < 16) cnt[tid] = 0u;

  double lam_den = 1.0, lam_rcp = 1.0;
  if (ni) {
    if (tid < 12) tab[tid] = tid < 6 ? pg.pay_c[tid] : pg.pay_d[tid - 6];
    const size_t stripe_len = (size_t)tb.slots * SPGG_NSTAT;
    const double* rrow = tb.stats + (size_t)rep * tb.stripes * stripe_len + (size_t)(t - 1) * SPGG_NSTAT + SPGG_ST_GMAX;
    double gmax = 0.0;
    for (int k = 0; k < tb.stripes; ++k) gmax = fmax(gmax, rrow[k * stripe_len]);
    lam_den = gmax + pg.lambda_eps;
    lam_rcp = 1.0 / lam_den;   // IEEE
  }
  __syncthreads();   // the edges, the zeroed counters, the tables

  uint32_t mine = 0u;   // lane k < 16: counts[k] of this wave over its tiles
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {   // workgroup-uniform
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    if (ni) {
      // (the last tile's readers of sS and sRew are past this point only after their last read: the
      // barrier below follows the writes of sS, the next one those of sRew)
      for (int i = tid; i < SW * SH; i += kThreads) {
        const int wy = i / SW, wx = i - wy * SW;
        sS[i] = sp[(size_t)spgg::wrap(y0 - HS + wy, L) * L + spgg::wrap(x0 - HS + wx, L)];
      }
      __syncthreads();           // the window
      const double w_p = pg.w_p, w_rep = pg.w_rep, norm_min = pg.norm_min, norm_den = pg.norm_den, norm_rcp = pg.norm_rcp;
      for (int i = tid; i < RW * RH; i += kThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const uint8_t* c = sS + (ry + 2) * SW + (rx + 2);
#define CO(dy, dx) (((c[(dy) * SW + (dx)] >> 3) & 1) ? 0 : 1)   // cooperator of S_{t-1}
        Cells13 k;
        k.c00 = CO(0, 0); k.cm0 = CO(-1, 0); k.cp0 = CO(1, 0); k.c0m = CO(0, -1); k.c0p = CO(0, 1);
        k.cmm = CO(-1, -1); k.cmp = CO(-1, 1); k.cpm = CO(1, -1); k.cpp = CO(1, 1);
        k.cM0 = CO(-2, 0); k.cP0 = CO(2, 0); k.c0M = CO(0, -2); k.c0P = CO(0, 2);
#undef CO
        const double P = payoff13(k, tab, norm_min, norm_den, norm_rcp);
        const double rr = (c[0] & 1) ? 0.0 : 0.5;                    // a_{t-1} = S_t (spgg.py:424-427)
        const double wpp = w_p * P, wrr = w_rep * rr;
        sRew[i] = wpp + wrr;
      }
      __syncthreads();   // the rewards
    }

    const int lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int gx = x0 + lx, gy = y0 + ly;
    const bool owned = gx < L && gy < L;
    int key = 0;
    if (owned) {
      const size_t g = (size_t)gy * L + gx;
      const uint8_t b = sp[g];
      // T rows (T[0,0], T[0,1]) and (T[1,0], T[1,1]) from the state planes, 16 bytes per load
      double q[4], qb[4];
      const double2* Qr = reinterpret_cast<const double2*>(tb.Q) + (size_t)rep * n * (QB ? 4 : 2);
      if constexpr (QB) {
        const double2 a0 = Qr[2 * g], b0 = Qr[2 * g + 1], a1 = Qr[2 * (n + g)], b1 = Qr[2 * (n + g) + 1];
        q[0] = a0.x; q[1] = a0.y; q[2] = a1.x; q[3] = a1.y;
        qb[0] = b0.x; qb[1] = b0.y; qb[2] = b1.x; qb[3] = b1.y;
      } else {
        const double2 a0 = Qr[g], a1 = Qr[n + g];
        q[0] = a0.x; q[1] = a0.y; q[2] = a1.x; q[3] = a1.y;
      }
      if (ni) {
        const int e = pending_entry(b);
        const double md = prev_max_diff<M2>(sRew, (ly + M) * RW + (lx + M), RW);
        const double nu = pending_nu(b, md, kappa, lam_den, lam_rcp);
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // selects on a constant index: the rows stay in registers
          q[k] = e == k ? q[k] + nu : q[k];
          if constexpr (QB) qb[k] = e == k ? qb[k] + nu : qb[k];   // both tables (spgg.py:496-502)
        }
      }
      if constexpr (QB) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = mean2(q[k], qb[k]);
      }
      const int cls = greedy2(q[0], q[1]) + 2 * greedy2(q[2], q[3]);
      const int sigma = b & 1;
      const int z = tt == 1 ? (tb.action_state ? (sigma == 0 ? 1 : 0) : 0) : (b >> 4) & 1;
      key = cls * 4 + sigma * 2 + z;
      plane[(size_t)rep * n + g] = (uint8_t)(cls | sigma << 2 | z << 3);
      uint32_t* hs = h[wave] + sigma * 2 * (bins + 2);
      atomicAdd(&hs[slot_of(sE, bins, q[0] - q[1])], 1u);
      atomicAdd(&hs[(bins + 2) + slot_of(sE, bins, q[2] - q[3])], 1u);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const unsigned long long m = __ballot(owned && key == k);
      if (lane == k) mine += (uint32_t)__popcll(m);
    }
  }   // tiles
  if (lane < 16 && mine) atomicAdd(&cnt[lane], mine);
  __syncthreads();
  int32_t* o = out + (long long)rep * out_stride;
  if (tid < 16 && cnt[tid]) atomicAdd(o + tid, (int32_t)cnt[tid]);
  for (int i = tid; i < hw; i += kThreads) {
    uint32_t c = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += h[w][i];
    if (c) atomicAdd(o + SPGG_POLICY_COUNTS + i, (int32_t)c);
  }
}

__global__ __launch_bounds__(kThreads) void spgg_policy_bonds_kernel(const uint8_t* __restrict__ plane, int L,
                                                                     int32_t* __restrict__ out, long long out_stride) {
  __shared__ uint32_t cnt[5];
  const int rep = blockIdx.y;
  const long long n = (long long)L * L;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint8_t* p = plane + (size_t)rep * n;
  if (tid < 5) cnt[tid] = 0u;
  __syncthreads();
  uint32_t mine = 0u;   // lane k < 4: bonds_same[k], lane 4: bonds_mixed, of this wave
  const long long base = (long long)blockIdx.x * kBondCells;
#pragma unroll 2
  for (int j = 0; j < kBondCells / kThreads; ++j) {
    const long long i = base + j * kThreads + tid;
    const bool valid = i < n;
    int right = 4, down = 4;
    if (valid) {
      const int y = (int)(i / L), x = (int)(i - (long long)y * L);
      const int c = p[i] & 3;
      const int cr = p[(long long)y * L + (x + 1 == L ? 0 : x + 1)] & 3;
      const int cd = p[(long long)(y + 1 == L ? 0 : y + 1) * L + x] & 3;
      right = c == cr ? c : 4;
      down = c == cd ? c : 4;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned long long a = __ballot(valid && right == k), b = __ballot(valid && down == k);
      if (lane == k) mine += (uint32_t)(__popcll(a) + __popcll(b));
    }
  }
  if (lane < 5 && mine) atomicAdd(&cnt[lane], mine);
  __syncthreads();
  if (tid < 5 && cnt[tid]) atomicAdd(out + (long long)rep * out_stride + 16 + tid, (int32_t)cnt[tid]);
}

}  // namespace

void launch(const spgg_obs::Lattices& lat, const Tables& tb, int t, int bins, const double* edges, uint8_t* plane,
            int32_t* out, int64_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(spgg_policy_zero_kernel, dim3(lat.n_rep), dim3(kThreads), 0, s, out, (long long)out_stride,
                     width(bins));
  const int tiles_x = (lat.L + kTileW - 1) / kTileW, tiles_y = (lat.L + kTileH - 1) / kTileH;
  auto kernel = spgg_policy_kernel<false, false>;
  if (tb.second_order) kernel = tb.double_q ? spgg_policy_kernel<true, true> : spgg_policy_kernel<true, false>;
  else if (tb.double_q) kernel = spgg_policy_kernel<false, true>;
  const int tiles = tiles_x * tiles_y;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups_per_replica(tiles, lat.n_rep), lat.n_rep), dim3(kThreads), 0, s, lat.S0,
                     lat.S1, lat.stop_iter, tb, lat.L, tiles_x, tiles, t, bins, edges, plane, out, (long long)out_stride);
  const dim3 grid((unsigned)((lat.cells() + kBondCells - 1) / kBondCells), lat.n_rep);
  hipLaunchKernelGGL(spgg_policy_bonds_kernel, grid, dim3(kThreads), 0, s, plane, lat.L, out, (long long)out_stride);
}

}  // namespace spgg_po
