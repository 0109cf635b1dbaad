// What the kernels that walk a Young lottery on the 64-column block shape share: the forward
// sweep (transition.hip), the sequence-space Jacobian (transition_jac.hip), the values
// (welfare.hip) and the 256-thread row reductions (welfare.hip, dist_stats.hip).  The device
// pieces are inlined into their kernels; entry points that promise each other's bits call the
// same piece, so they add in the same order by construction.
#pragma once
#include "common.h"
#include "hist_cluster.h"
#include "internal.h"

namespace aiy {

constexpr int kTrBlock = 256;
constexpr int kTrWaves = kTrBlock / kWave;

constexpr int kTrRangePer = 4;   // sources per thread (one per thread: ~2 M tiny workgroups at Table II size)

// A block owns kTrCols columns (one per lane); its waves share the states.
constexpr int kTrCols = kWave;
constexpr int kTrTile = AIY_MAX_STATES * kTrCols;   // doubles of the block's LDS tile [s][lane]

// ---------------------------------------------------------------------------------
// Host: sizes, argument check
// ---------------------------------------------------------------------------------
// Largest sizes the pull kernels index (host-only).
inline bool tr_pull_sizes_ok(int n_cal, int S, int n_a) {
  return n_cal >= 1 && n_cal <= 65535 && S >= 1 && S <= AIY_MAX_STATES && n_a >= 2 &&
         (long long)S * (n_a + 1) < 2147483647LL && n_a < 2147483647 - 2 * kTrBlock * kTrRangePer;
}

inline int tr_nblk(int n_a) { return (n_a + kTrCols - 1) / kTrCols; }   // blocks of kTrCols columns

// The argument check of (n_cal, S, n_a) and, with_T, T; more_ok: the caller's own limits.
inline int32_t tr_check(aiy_handle* h, int n_cal, int S, int n_a, bool with_T = false, int T = 1, bool more_ok = true) {
  if (with_T && T < 1) return fail(h, AIY_ERR_ARG, "T=%d must be >= 1", T);
  if (n_a < 2) return fail(h, AIY_ERR_ARG, "n_a=%d must be >= 2", n_a);
  if (S < 1 || S > AIY_MAX_STATES) return fail(h, AIY_ERR_ARG, "S=%d outside 1..%d", S, AIY_MAX_STATES);
  if (tr_pull_sizes_ok(n_cal, S, n_a) && more_ok) return AIY_OK;
  if (with_T) return fail(h, AIY_ERR_ARG, "bad sizes n_cal=%d S=%d n_a=%d T=%d", n_cal, S, n_a, T);
  return fail(h, AIY_ERR_ARG, "bad sizes n_cal=%d S=%d n_a=%d", n_cal, S, n_a);
}

// jb[t][cal][s][d] = first j with lo[t][cal][s][j] >= d (d in [0, n_a]) for the T periods of a
// [T][n_cal][S][n_a] lottery, and the row check (tr_range_kernel, transition.hip).  Blocks on
// `st` for the flag (4 bytes at d_flag).  AIY_ERR_UNSUPPORTED, with last_error naming the
// check, when a row is not non-decreasing or leaves [0, n_a - 2]; jb is then not to be used.
int32_t tr_build_ranges(aiy_handle* h, int n_cal, int S, int n_a, int T, const int* lo, int* jb, int* d_flag,
                        hipStream_t st);

// g[d][j] = sum over s, ascending, of mass[d][s][j] for the n_dist distributions of a
// [n_dist][S][n_a] stack (tr_marginal_kernel, transition.hip).  Asynchronous on `st`.
void tr_launch_marginal(long long n_dist, int S, int n_a, const double* mass, double* g, hipStream_t st);

// The windows of every row of a [T][n_cal][S][n_a] lottery whose rows need not be monotone
// (tr_windows_kernel, transition.hip): jlo[row][d] = first j whose prefix maximum
// of lo is >= d, jhi[row][d] = first j whose suffix minimum is > d, d in [0, n_a], so the sources
// with lo = d lie in [jlo[d], jhi[d]); on a monotone row jlo[d] = jb[d] and jhi[d] = jb[d + 1].
// Blocks on `st` for d_flag[0] and d_flag[1], the number of rows with a decreasing pair (to
// *rows_turned).  AIY_ERR_UNSUPPORTED, naming the check, when an entry leaves [0, n_a - 2] or a
// row's windows hold more than kTrAnyCap (n_a + 1) sources; the arrays are then not to be used.
constexpr int kTrAnyCap = 4;
int32_t tr_build_windows(aiy_handle* h, int n_cal, int S, int n_a, int T, const int* lo, int* jlo, int* jhi,
                         int* d_flag, int* rows_turned, hipStream_t st);

// ---------------------------------------------------------------------------------
// The 64-column kernels: grid (tr_nblk(n_a), n_cal[, periods]), kTrBlock threads, a kTrTile LDS tile
// ---------------------------------------------------------------------------------
struct TrPlace {
  int cal, wave, lane, col;   // wave is wave-uniform (an SGPR); col: the lane's column
  bool active;                // col < n_a
  size_t rows;                // cal S: the calibration's first row of a [n_cal][S][.] array
};
__device__ __forceinline__ TrPlace tr_place(int S, int n_a) {
  TrPlace p;
  p.cal = blockIdx.y;
  p.wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  p.lane = threadIdx.x & (kWave - 1);
  p.col = blockIdx.x * kTrCols + p.lane;
  p.active = p.col < n_a;
  p.rows = (size_t)p.cal * S;
  return p;
}

// The pull of one (state, column d): T_s[d] = the wlo mass terms of the sources with lo = d, then
// the (1 - wlo) mass terms of those with lo = d - 1, both ascending in j (np.add.at's order in
// hist_step); J, W, Q: the state's rows of jb, wlo and the mass.  A lane whose range is longer
// than a wave has it summed by the whole wave (lane-strided partials, then wave_sum_lane63).
// WITH_C: every term times its consumption (Rt ag[j] + ls) - ad is added to cacc.  Every lane of
// the wave must call it.
// ANY (rows that need not be monotone, tr_build_windows): J and H are the state's rows of jlo and
// jhi, L its row of lo.  The sources with lo = d lie in the window [J[d], H[d]) and those with
// lo = d - 1 in [J[d - 1], H[d - 1]); both are walked as above and a source counts only where L
// says so, the consumption term included.  On a monotone row the windows are the ranges and
// every source in them matches: the same terms in the same order.
template <bool WITH_C, bool ANY = false>
__device__ __forceinline__ double tr_pull(const int* J, const double* W, const double* Q, int d, bool active, int lane,
                                          const double* ag, double Rt, double ls, double ad, double& cacc,
                                          const int* L = nullptr, const int* H = nullptr) {
  int a0 = 0, a1 = 0, a2 = 0;   // lo = d - 1: [a0, e1), lo = d: [a1, a2); e1 = a1 unless ANY
  int h0 = 0;
  if (active) {
    a1 = J[d];
    if constexpr (ANY) {
      a2 = H[d];
      a0 = d > 0 ? J[d - 1] : a1;
      h0 = d > 0 ? H[d - 1] : a1;
    } else {
      a2 = J[d + 1];
      a0 = d > 0 ? J[d - 1] : a1;
    }
  }
  const int e1 = ANY ? h0 : a1;
  const bool heavy = (a2 - a1 > kWave) || (e1 - a0 > kWave);
  double ts = 0.0;
  if (!heavy) {
    for (int j = a1; j < a2; ++j) {                      // np.add.at(T, lo, w q), ascending j
      if constexpr (ANY) {
        if (L[j] != d) continue;
      }
      const double term = W[j] * Q[j];
      ts += term;
      if constexpr (WITH_C) cacc += term * ((Rt * ag[j] + ls) - ad);
    }
    for (int j = a0; j < e1; ++j) {                      // np.add.at(T, lo + 1, (1 - w) q)
      if constexpr (ANY) {
        if (L[j] != d - 1) continue;
      }
      const double term = (1.0 - W[j]) * Q[j];
      ts += term;
      if constexpr (WITH_C) cacc += term * ((Rt * ag[j] + ls) - ad);
    }
  }
  unsigned long long hm = __ballot(heavy);
  while (hm) {   // wave-uniform: the whole wave sums one lane's ranges
    const int hl = __builtin_ctzll(hm);
    hm &= hm - 1ull;
    const int b0 = __builtin_amdgcn_readlane(a0, hl), b1 = __builtin_amdgcn_readlane(a1, hl),
              b2 = __builtin_amdgcn_readlane(a2, hl);
    int g1 = b1, dh = 0;   // the end of the lo = d - 1 part; ANY: the heavy lane's column
    if constexpr (ANY) {
      g1 = __builtin_amdgcn_readlane(h0, hl);
      dh = __builtin_amdgcn_readlane(d, hl);
    }
    double adh = 0.0;
    if constexpr (WITH_C) adh = __shfl(ad, hl, kWave);
    double pa = 0.0, pb = 0.0, pc = 0.0;
    for (int j = b1 + lane; j < b2; j += kWave) {
      if constexpr (ANY) {
        if (L[j] != dh) continue;
      }
      const double term = W[j] * Q[j];
      pa += term;
      if constexpr (WITH_C) pc += term * ((Rt * ag[j] + ls) - adh);
    }
    for (int j = b0 + lane; j < g1; j += kWave) {
      if constexpr (ANY) {
        if (L[j] != dh - 1) continue;
      }
      const double term = (1.0 - W[j]) * Q[j];
      pb += term;
      if constexpr (WITH_C) pc += term * ((Rt * ag[j] + ls) - adh);
    }
    const double ta = wave_sum_lane63(pa), tb = wave_sum_lane63(pb);
    const double tot = __shfl(ta, kWave - 1, kWave) + __shfl(tb, kWave - 1, kWave);
    double tc = 0.0;
    if constexpr (WITH_C) tc = __shfl(wave_sum_lane63(pc), kWave - 1, kWave);
    if (lane == hl) {
      ts = tot;
      if constexpr (WITH_C) cacc += tc;
    }
  }
  return ts;
}

// tr_pull (monotone rows) for GC masses at once: Q is the state's row of the first mass and mass
// g's row lies g * gstride doubles behind it (g < ng <= GC live; the others repeat the last live
// one and their results are the caller's to drop).  The ranges, their order, the whole-wave path
// and, mass by mass, every floating-point operation are tr_pull's -- W[j] and the consumption
// factor are loaded / formed once per source and the GC sums ts[g] (and cacc[g], WITH_C) are kept
// in registers -- so ts[g] and cacc[g] have the bits tr_pull gives on mass g alone.  Every lane
// of the wave must call it.
template <int GC, bool WITH_C>
__device__ __forceinline__ void tr_pull_multi(const int* J, const double* W, const double* Q, size_t gstride, int ng,
                                              int d, bool active, int lane, const double* ag, double Rt, double ls,
                                              double ad, double (&ts)[GC], double (&cacc)[GC]) {
  int a0 = 0, a1 = 0, a2 = 0;   // lo = d - 1: [a0, a1), lo = d: [a1, a2)
  if (active) {
    a1 = J[d];
    a2 = J[d + 1];
    a0 = d > 0 ? J[d - 1] : a1;
  }
  const bool heavy = (a2 - a1 > kWave) || (a1 - a0 > kWave);
  auto row = [&](int g) { return Q + (size_t)(g < ng ? g : ng - 1) * gstride; };   // wave-uniform
#pragma unroll
  for (int g = 0; g < GC; ++g) ts[g] = 0.0;
  if (!heavy) {
    for (int j = a1; j < a2; ++j) {                      // np.add.at(T, lo, w q), ascending j
      const double wj = W[j];
      double cf = 0.0;
      if constexpr (WITH_C) cf = (Rt * ag[j] + ls) - ad;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const double term = wj * row(g)[j];
        ts[g] += term;
        if constexpr (WITH_C) cacc[g] += term * cf;
      }
    }
    for (int j = a0; j < a1; ++j) {                      // np.add.at(T, lo + 1, (1 - w) q)
      const double wj = 1.0 - W[j];
      double cf = 0.0;
      if constexpr (WITH_C) cf = (Rt * ag[j] + ls) - ad;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const double term = wj * row(g)[j];
        ts[g] += term;
        if constexpr (WITH_C) cacc[g] += term * cf;
      }
    }
  }
  unsigned long long hm = __ballot(heavy);
  while (hm) {   // wave-uniform: the whole wave sums one lane's ranges
    const int hl = __builtin_ctzll(hm);
    hm &= hm - 1ull;
    const int b0 = __builtin_amdgcn_readlane(a0, hl), b1 = __builtin_amdgcn_readlane(a1, hl),
              b2 = __builtin_amdgcn_readlane(a2, hl);
    double adh = 0.0;
    if constexpr (WITH_C) adh = __shfl(ad, hl, kWave);
    double pa[GC], pb[GC], pc[GC];
#pragma unroll
    for (int g = 0; g < GC; ++g) pa[g] = pb[g] = pc[g] = 0.0;
    for (int j = b1 + lane; j < b2; j += kWave) {
      const double wj = W[j];
      double cf = 0.0;
      if constexpr (WITH_C) cf = (Rt * ag[j] + ls) - adh;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const double term = wj * row(g)[j];
        pa[g] += term;
        if constexpr (WITH_C) pc[g] += term * cf;
      }
    }
    for (int j = b0 + lane; j < b1; j += kWave) {
      const double wj = 1.0 - W[j];
      double cf = 0.0;
      if constexpr (WITH_C) cf = (Rt * ag[j] + ls) - adh;
#pragma unroll
      for (int g = 0; g < GC; ++g) {
        const double term = wj * row(g)[j];
        pb[g] += term;
        if constexpr (WITH_C) pc[g] += term * cf;
      }
    }
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      const double ta = wave_sum_lane63(pa[g]), tb = wave_sum_lane63(pb[g]);
      const double tot = __shfl(ta, kWave - 1, kWave) + __shfl(tb, kWave - 1, kWave);
      double tc = 0.0;
      if constexpr (WITH_C) tc = __shfl(wave_sum_lane63(pc[g]), kWave - 1, kWave);
      if (lane == hl) {
        ts[g] = tot;
        if constexpr (WITH_C) cacc[g] += tc;
      }
    }
  }
}

// Block sum in a fixed order (xor butterflies per wave, waves ascending); thread 0 holds it.
__device__ __forceinline__ double tr_block_sum(double v, double* red) {
  v = wave_sum_fixed(v);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  double k = 0.0;
  if (threadIdx.x == 0)
    for (int q = 0; q < kTrWaves; ++q) k += red[q];
  return k;
}

// The two mixes of the lane's column of the LDS tile X[s][lane] by P [S][S] (wave-uniform):
// forward, mass'[sp] = sum over s, ascending, of P[s, sp] X[s] (hist_mix_kernel's order) ...
__device__ __forceinline__ double tr_mix_forward(const double* P, const double* X, int S, int sp, int lane) {
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += P[(size_t)s * S + sp] * X[s * kTrCols + lane];
  return acc;
}
// ... and adjoint, G[s] = sum over s', ascending, of P[s, s'] X[s'] (Ps: row s of P).
__device__ __forceinline__ double tr_mix_adjoint(const double* Ps, const double* X, int S, int lane) {
  double acc = 0.0;
  for (int sp = 0; sp < S; ++sp) acc += Ps[sp] * X[sp * kTrCols + lane];
  return acc;
}

// The adjoint of the lottery at one source: the weights wl, 1 - wl on g[d], g[d + 1].
__device__ __forceinline__ double tr_gather(const double* g, int d, double wl) {
  return wl * g[d] + (1.0 - wl) * g[d + 1];
}

// The adjoint step of a block, in two halves around the caller's barrier.  First wave w puts
// value(s, o), o the offset of (cal, s, column) in a [n_cal][S][n_a] array, into the tile for
// s = w, w + 4, ... (0 in the columns past n_a, where value is not called) ...
template <class Value>
__device__ __forceinline__ void tr_adjoint_values(const TrPlace& p, int S, int n_a, double* X, Value value) {
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves) {
    double v = 0.0;
    if (p.active) v = value(s, (p.rows + s) * (size_t)n_a + p.col);
    X[s * kTrCols + p.lane] = v;
  }
}
// ... then, behind the barrier, it mixes the block's own columns into G_out (P: [n_cal][S][S]).
__device__ __forceinline__ void tr_adjoint_mix(const TrPlace& p, int S, int n_a, const double* P, const double* X,
                                               double* G_out) {
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves) {
    const double acc = tr_mix_adjoint(P + (p.rows + s) * S, X, S, p.lane);
    if (p.active) G_out[(p.rows + s) * (size_t)n_a + p.col] = acc;
  }
}

// ---------------------------------------------------------------------------------
// The row kernels: one workgroup of kTrBlock threads per row of n nodes
// ---------------------------------------------------------------------------------
// Thread k owns the contiguous chunk [j0, j1) of ceil(n / kTrBlock) nodes from k * chunk (threads
// past the end own nothing); returns the chunk length.
__device__ __forceinline__ int row_chunk(int n, int k, int& j0, int& j1) {
  const int chunk = (n + kTrBlock - 1) / kTrBlock;
  const long long c0 = (long long)k * chunk;
  j0 = c0 < n ? (int)c0 : n;
  j1 = c0 + chunk < n ? (int)(c0 + chunk) : n;
  return chunk;
}
// The sum of the threads' v: wave_sum_lane63, then the waves in ascending order through
// s_wave[kTrWaves].  Holds a block barrier; thread 0 gets the sum.
__device__ __forceinline__ double row_block_sum(double v, double* s_wave) {
  const double ws = wave_sum_lane63(v);
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) s_wave[threadIdx.x / kWave] = ws;
  __syncthreads();
  double tot = 0.0;
  if (threadIdx.x == 0)
    for (int q = 0; q < kTrWaves; ++q) tot += s_wave[q];
  return tot;
}

}  // namespace aiy
