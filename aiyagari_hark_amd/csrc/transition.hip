// Perfect-foresight transition paths of the stationary economy for gfx950.
//
// One household-block evaluation for given price paths R[0..T], w[0..T] is
//   backward  u = T .. 1: (m_{u-1}, c_{u-1}) = EGM step from (m_u, c_u) at period u's prices,
//             and the Young lottery of period u from the SAME interpolated consumption
//             (the s' = s query of the step is the lottery's query R_u a_j + w_u l_s);
//             a last lottery-only launch handles period 0;
//   forward   t = 0 .. T-1: mass_{t+1} = lottery pull of mass_t mixed over states,
//             Ks[t+1] = sum mass_{t+1} a, C[t] = sum mass_t (q_t - a'_t).
// Every period is one launch, enqueued back to back on the call's stream: no host
// synchronisation, no graph and no in-kernel grid barrier inside a sweep.
//
//   tr_backward_kernel   block = (calibration, tile of 64 asset nodes), wave w owns next
//                        states s' = w, w + 4, ...: interp_row_wave's search on row s' of
//                        period u's tables (the wave-uniform bounds found by 64 probes a
//                        round, the lanes' brackets in an LDS window), V[s'] to LDS, lottery
//                        (lo, wlo) of (s', node); then wave w owns current states s:
//                        E = beta sum V P in NumPy's pairwise order, c = E^(-1/rho), m = a + c.
//                        The arithmetic is aiy_egm_step's (n_M = 1) and aiy_hist_lottery's
//                        expression for expression, so the results are bit-identical to
//                        chaining the two.
//   tr_range_kernel      jb[t][cal][s][d] = first j with lo >= d for every period at once (as
//                        hist_range_kernel) and the row check: non-decreasing, in [0, n_a - 2].
//   tr_forward_kernel    block = (calibration, 64 destination columns), one column per lane,
//                        the waves share the states: tr_pull (transition_common.h) of every
//                        (s, column) into LDS, then tr_mix_forward for each s'.  No atomics on
//                        mass.  The block's partial of Ks[t + 1] and C[t] goes to
//                        [period][calibration][block]; tr_sum_kernel adds the blocks in block
//                        order after the sweep (two fixed-order levels).
//
//   tr_marginal_kernel   (aiy_transition_forward_marginals only) the sum over s, ascending, of the
//                        mass a period's step just wrote: thread = (calibration, node).
//
//   tr_windows_kernel    (aiy_transition_forward_any) in place of tr_range_kernel for
//                        rows that need not be monotone: a workgroup per row, jlo / jhi from the
//                        row's prefix maximum and suffix minimum, the range and work checks and the
//                        count of turned rows; tr_forward_kernel<., true> then pulls through the
//                        windows with lo as the predicate.
//
// Offsets into the [T][n_cal][S][n_a] arrays are size_t (24 x 300 x 7 x 10 000 > 2^31).
#include "common.h"
#include "egm_common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>

namespace aiy {

// ---------------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------------
struct TrBack {
  int S, n_a, T, u;            // u: the period of the tables read (its prices, its lottery)
  const double* a_grid;        // [n_cal][n_a]
  const double* P;             // [n_cal][S][S]
  const double* lab;           // [n_cal][S]
  const double* beta;          // [n_cal]
  const double* crra;          // [n_cal]
  const double* R;             // [n_cal][T + 1]
  const double* w;             // [n_cal][T + 1]
  const double* m_in;          // [n_cal][S][n_a + 1] tables of period u
  const double* c_in;
  double* m_out;               // tables of period u - 1 (STEP)
  double* c_out;
  int* lo;                     // [n_cal][S][n_a] lottery of period u, or null
  double* wlo;
};

// Bound of a wave-uniform query q over the sorted x[lo, hi), searched by the whole wave: every
// round the 64 lanes probe 64 evenly spaced nodes (one load each), so a 10 000-node row takes
// 3 dependent loads where a binary search takes 14.  UPPER: the first index with x > q
// (searchsorted 'right'), else the first with x >= q ('left') -- on a sorted row the index the
// binary searches of common.h return.  Every lane of the wave must call it.
template <bool UPPER>
__device__ __forceinline__ int tr_wave_bound(const double* __restrict__ x, int lo, int hi, double q, int lane) {
  while (lo < hi) {   // wave-uniform
    const int stride = (hi - lo + kWave - 1) / kWave;
    const int idx = lo + lane * stride;
    bool below = false;
    if (idx < hi) {
      const double v = x[idx];
      below = UPPER ? v <= q : v < q;
    }
    const int cnt = __popcll(__ballot(below));   // the probes below q are a prefix (sorted row)
    if (cnt == 0) return lo;
    const int last = lo + (cnt - 1) * stride;    // bound in (last, last + stride], and <= hi
    hi = last + stride < hi ? last + stride : hi;
    lo = last + 1;
  }
  return lo;
}

__device__ __forceinline__ void tr_wave_sync() {   // LDS hand-off inside one wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// interp_row_wave (HARK LinearInterp of a row of n + 1 nodes at the lanes' queries; all lanes
// active) with the two wave-uniform searches done by tr_wave_bound and, where the nodes
// [lb(qmin) - 1, lb(qmax)] fit a kWin window, the lanes' own searches done in the wave's LDS
// slice (X, Y: kWin doubles each).  Same lower bound, lerp_at's arithmetic: the same bits.
__device__ __forceinline__ double tr_interp_row(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                double q, int lane, double* X, double* Y) {
  const double qmin = wave_min(q), qmax = wave_max(q);
  int lo = 0, hi = n;
  if (qmin == qmin && qmax == qmax && qmin <= qmax) {
    lo = tr_wave_bound<false>(x, 0, n, qmin, lane);
    hi = tr_wave_bound<false>(x, lo, n, qmax, lane);   // lb(q) lies in [lb(qmin), lb(qmax)]
  }
  const int base = lo > 0 ? lo - 1 : 0;
  if (hi - base >= kWin) {   // wave-uniform: window too small, the lanes search global memory
    int i = lower_bound(x, lo, hi, q);
    i = i < 1 ? 1 : i;
    return lerp_at(x, y, i, q, x[0]);
  }
  const int t0 = base + lane, t1 = t0 + kWave;   // nodes base .. hi <= n; beyond them never read
  const int u0 = t0 <= n ? t0 : n, u1 = t1 <= n ? t1 : n;
  const double x0v = x[u0], y0v = y[u0], x1v = x[u1], y1v = y[u1];
  tr_wave_sync();   // the previous row's readers are done with the slice
  X[lane] = x0v;
  Y[lane] = y0v;
  X[lane + kWave] = x1v;
  Y[lane + kWave] = y1v;
  tr_wave_sync();
  int a = lo - base, b = hi - base;
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (X[mid] < q) a = mid + 1; else b = mid;
  }
  int i = base + a;
  i = i < 1 ? 1 : i;
  const int k = i - base;   // in [1, hi - base]
  const double xl = X[k - 1], xh = X[k], yl = Y[k - 1], yh = Y[k];
  const double alpha = (q - xl) / (xh - xl);
  const double v = (1.0 - alpha) * yl + alpha * yh;
  // below x[0] only when the window starts at node 0 (else x[0] <= x[lo - 1] < qmin)
  return (base == 0 && q < X[0]) ? __builtin_nan("") : v;
}

// hist_lottery_kernel's lottery of savings ap onto a_grid (n nodes): d = clip(searchsorted(ag,
// ap, 'right') - 1, 0, n - 2) and the weight on d, the searches as in tr_interp_row.
__device__ __forceinline__ void tr_lottery(const double* __restrict__ ag, int n, double ap, int lane, double* X,
                                           int& d, double& wl) {
  const double pmin = wave_min(ap), pmax = wave_max(ap);
  int lo = 0, hi = n;
  if (pmin == pmin && pmax == pmax && pmin <= pmax) {
    lo = tr_wave_bound<true>(ag, 0, n, pmin, lane);
    hi = tr_wave_bound<true>(ag, lo, n, pmax, lane);
  }
  // nodes d, d + 1 of every lane: from lo - 1 (clipped into [0, n - 2]) to min(hi, n - 1)
  const int base = lo > 0 ? (lo - 1 < n - 2 ? lo - 1 : n - 2) : 0;
  const bool fits = hi - base < kWin;   // wave-uniform
  double g0, g1;
  if (fits) {
    const int t0 = base + lane, t1 = t0 + kWave;
    const double v0 = ag[t0 < n ? t0 : n - 1], v1 = ag[t1 < n ? t1 : n - 1];
    tr_wave_sync();
    X[lane] = v0;
    X[lane + kWave] = v1;
    tr_wave_sync();
  }
  if (fits && ap == ap) {
    int a = lo - base, b = hi - base;
    while (a < b) {
      const int mid = a + ((b - a) >> 1);
      if (X[mid] <= ap) a = mid + 1; else b = mid;
    }
    d = base + a - 1;
    d = d < 0 ? 0 : (d > n - 2 ? n - 2 : d);   // d in [base, min(hi, n - 1) - 1]
    g0 = X[d - base];
    g1 = X[d + 1 - base];
  } else {   // NaN savings or a window too small: hist_lottery_kernel's own search
    d = upper_bound(ag, 0, n, ap) - 1;
    d = d < 0 ? 0 : (d > n - 2 ? n - 2 : d);
    g0 = ag[d];
    g1 = ag[d + 1];
  }
  wl = (g1 - ap) / (g1 - g0);
  wl = wl < 0.0 ? 0.0 : (wl > 1.0 ? 1.0 : wl);
}

// Phase 1 of one wave: its next states' interpolated consumption at q = R a + w l(s'), the
// marginal values (STEP) and the lottery of (s', node) (lo != null).
template <int PK, bool STEP>
__device__ __forceinline__ void tr_back_phase1(const TrBack& A, int cal, int wave, int lane, int i, double a,
                                               double R, const double* Wl, double gam, double* Vs, double* X,
                                               double* Y) {
  const int S = A.S, n = A.n_a, n1 = n + 1;
  const double* ag = A.a_grid + (size_t)cal * n;
#pragma unroll 1
  for (int sp = wave; sp < S; sp += kTrWaves) {
    const double q = R * a + Wl[sp];                      // mNextArray (AS:1024) == the lottery's m
    const size_t row = ((size_t)cal * S + sp) * n1;
    const double c = tr_interp_row(A.m_in + row, A.c_in + row, n, q, lane, X, Y);
    if constexpr (STEP) Vs[sp * kTile + lane] = R * marg_u<PK>(c, gam);   // RnextArray * vPnext
    if (A.lo != nullptr) {   // block-uniform
      int d;
      double wl;
      tr_lottery(ag, n, q - c, lane, X, d, wl);
      if (i < n) {
        const size_t o = ((size_t)cal * S + sp) * n + i;
        A.lo[o] = d;
        A.wlo[o] = wl;
      }
    }
  }
}

// Phase 2 of one wave: its current states' (m, c) of period u - 1.
template <int SMAX, int PK>
__device__ __forceinline__ void tr_back_phase2(const TrBack& A, int cal, int wave, int lane, int ic, double a,
                                               double beta, double gam, const double* Vs, const double* Pl) {
  const int S = A.S, n1 = A.n_a + 1;
#pragma unroll 1
  for (int s = wave; s < S; s += kTrWaves) {
    const double* Ps = Pl + s * S;
    const double sum = np_pairwise_sum<SMAX>(S, [&](int t) { return Vs[t * kTile + lane] * uniform_f64(Ps[t]); });
    const double E = beta * sum;                          // EndOfPrdvP (AS:1485)
    const double c = inv_marg<PK>(E, gam);                // AS:1490
    const double m = a + c;                               // AS:1499
    const size_t row = ((size_t)cal * S + s) * n1;
    A.m_out[row + ic + 1] = m;
    A.c_out[row + ic + 1] = c;
    if (ic == 0) {
      A.m_out[row] = kBorrowNode;
      A.c_out[row] = kBorrowNode;
    }
  }
}

template <int SMAX, bool STEP>
__global__ __launch_bounds__(kTrBlock) void tr_backward_kernel(TrBack A) {
  const int cal = blockIdx.y, tile = blockIdx.x;
  const int S = A.S;
  __shared__ double Vs[STEP ? SMAX * kTile : 1];
  __shared__ double Pl[STEP ? SMAX * SMAX : 1];
  __shared__ double s_Wl[SMAX];
  __shared__ double s_win[kTrWaves][2 * kWin];   // per wave: X | Y node windows
  const double R = A.R[(size_t)cal * (A.T + 1) + A.u];
  const double w = A.w[(size_t)cal * (A.T + 1) + A.u];
  if constexpr (STEP) {
    const double* Pc = A.P + (size_t)cal * S * S;
    for (int q = threadIdx.x; q < S * S; q += kTrBlock) Pl[q] = Pc[q];
  }
  if ((int)threadIdx.x < S) s_Wl[threadIdx.x] = w * A.lab[(size_t)cal * S + threadIdx.x];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  const int i = tile * kTile + lane;
  // lanes past the grid (last tile) repeat node n_a - 1: the same values to the same addresses
  const int ic = i < A.n_a ? i : A.n_a - 1;
  const double a = A.a_grid[(size_t)cal * A.n_a + ic];
  const double gam = A.crra[cal];
  const double beta = A.beta[cal];
  const int pk = crra_kind(gam);   // block-uniform power kind
  double* X = s_win[wave];
  double* Y = X + kWin;
  __syncthreads();
  if (pk == 1) tr_back_phase1<1, STEP>(A, cal, wave, lane, i, a, R, s_Wl, gam, Vs, X, Y);
  else if (pk == 3) tr_back_phase1<3, STEP>(A, cal, wave, lane, i, a, R, s_Wl, gam, Vs, X, Y);
  else if (pk == 5) tr_back_phase1<5, STEP>(A, cal, wave, lane, i, a, R, s_Wl, gam, Vs, X, Y);
  else tr_back_phase1<0, STEP>(A, cal, wave, lane, i, a, R, s_Wl, gam, Vs, X, Y);
  if constexpr (STEP) {
    __syncthreads();
    if (pk == 1) tr_back_phase2<SMAX, 1>(A, cal, wave, lane, ic, a, beta, gam, Vs, Pl);
    else if (pk == 3) tr_back_phase2<SMAX, 3>(A, cal, wave, lane, ic, a, beta, gam, Vs, Pl);
    else if (pk == 5) tr_back_phase2<SMAX, 5>(A, cal, wave, lane, ic, a, beta, gam, Vs, Pl);
    else tr_back_phase2<SMAX, 0>(A, cal, wave, lane, ic, a, beta, gam, Vs, Pl);
  }
}

template <int SMAX>
static void launch_back_s(const TrBack& A, int n_cal, bool step, hipStream_t st) {
  const dim3 grid((A.n_a + kTile - 1) / kTile, n_cal);
  if (step) hipLaunchKernelGGL((tr_backward_kernel<SMAX, true>), grid, dim3(kTrBlock), 0, st, A);
  else hipLaunchKernelGGL((tr_backward_kernel<SMAX, false>), grid, dim3(kTrBlock), 0, st, A);
}
static void launch_back(const TrBack& A, int n_cal, bool step, hipStream_t st) {
  if (A.S <= 8) launch_back_s<8>(A, n_cal, step, st);
  else if (A.S <= 16) launch_back_s<16>(A, n_cal, step, st);
  else if (A.S <= 32) launch_back_s<32>(A, n_cal, step, st);
  else launch_back_s<64>(A, n_cal, step, st);
}

// ---------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------
// jb[row][d] = first j with lo[row][j] >= d, d in [0, n_a], for rows r0 .. r0 + gridDim.z S of
// the [T n_cal S] rows (one thread per source j; j == n_a closes the row), and the row check.
// A thread writes jb only between two entries it found in range, so a bad row writes nothing
// out of bounds.
__global__ __launch_bounds__(kTrBlock) void tr_range_kernel(int S, int n_a, size_t r0, const int* __restrict__ lo,
                                                            int* __restrict__ jb, int* flag) {
  const size_t r = r0 + (size_t)blockIdx.z * S + blockIdx.y;
  const int* L = lo + r * n_a;
  int* J = jb + r * (n_a + 1);
#pragma unroll
  for (int k = 0; k < kTrRangePer; ++k) {
    const int j = (blockIdx.x * kTrRangePer + k) * kTrBlock + threadIdx.x;
    if (j > n_a) continue;
    const int prev = j == 0 ? -1 : L[j - 1];
    const int cur = j == n_a ? n_a : L[j];
    const bool prev_ok = j == 0 || (prev >= 0 && prev <= n_a - 2);
    const bool cur_ok = j == n_a || (cur >= 0 && cur <= n_a - 2);
    if (!prev_ok || !cur_ok || cur < prev) {
      atomicOr(flag, 1);
      continue;
    }
    for (int d = prev + 1; d <= cur; ++d) J[d] = j;
  }
}

// The inverse index of every period of a lottery and its row check (transition_common.h).
int32_t tr_build_ranges(aiy_handle* h, int n_cal, int S, int n_a, int T, const int* lo, int* jb, int* d_flag,
                        hipStream_t st) {
  AIY_HIP(h, hipMemsetAsync(d_flag, 0, sizeof(int), st));
  const long long n_tc = (long long)T * n_cal;   // (period, calibration) pairs, <= 65535 per launch
  for (long long z0 = 0; z0 < n_tc; z0 += 65535) {
    const unsigned nz = (unsigned)std::min<long long>(65535, n_tc - z0);
    const unsigned nx = (unsigned)((n_a + kTrBlock * kTrRangePer) / (kTrBlock * kTrRangePer));   // sources 0 .. n_a
    hipLaunchKernelGGL(tr_range_kernel, dim3(nx, S, nz), dim3(kTrBlock), 0, st, S, n_a,
                       (size_t)z0 * S, lo, jb, d_flag);
  }
  AIY_CHECK_LAUNCH(h);
  int flag = 0;
  AIY_HIP(h, hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  if (flag != 0)
    return fail(h, AIY_ERR_UNSUPPORTED,
                "transition lottery check failed: a row of lo is not monotone (non-decreasing) or leaves [0, n_a - 2]");
  return AIY_OK;
}

// The windows of rows that need not be monotone (transition_common.h): one
// workgroup per row r0 + blockIdx.y S + blockIdx.x of the [T n_cal S] rows.  Thread k owns
// row_chunk's chunk k.  It reduces the chunk's maximum and minimum, the block scans them (an
// exclusive prefix maximum and an exclusive suffix minimum over the 256 chunks: wave shuffles,
// then the four wave totals through LDS), and the thread walks its chunk twice: ascending with the
// running prefix maximum M, writing jlo[d] = j for d in (M, lo[j]] where lo[j] raises it, and
// descending with the running suffix minimum m, writing jhi[d] = j + 1 for d in [lo[j], m) where
// lo[j] lowers it -- tr_range_kernel's pattern.  The last thread closes jlo (d above the row's
// maximum: n_a), thread 0 closes jhi (d below the row's minimum: 0, and jhi[n_a] = n_a).  Every d
// in [0, n_a] is written exactly once per array.
// A row with an entry outside [0, n_a - 2] raises flag bit 1 (value 1) and writes nothing: the
// block leaves before the first write loop.  The row's sum over d of jhi[d] - jlo[d] is formed
// from the same steps that write (j times the number of d a step writes; integers, thread order):
// above kTrAnyCap (n_a + 1) it raises flag bit 2 (value 2).  flag[1] counts the rows with at
// least one decreasing pair.
// STAGED (rows of at most kTrWinStage entries): the block first copies the row into LDS, one
// entry per thread and round, and the three walks read it there -- a thread's chunk is contiguous,
// so the walks' own loads are a chunk apart from lane to lane.
#ifndef AIY_TR_WIN_STAGE
#define AIY_TR_WIN_STAGE 12288
#endif
constexpr int kTrWinStage = AIY_TR_WIN_STAGE;

template <bool STAGED>
__global__ __launch_bounds__(kTrBlock) void tr_windows_kernel(int S, int n_a, size_t r0, const int* __restrict__ lo,
                                                              int* __restrict__ jlo, int* __restrict__ jhi,
                                                              int* flag) {
  const size_t r = r0 + (size_t)blockIdx.y * S + blockIdx.x;
  const int* L = lo + r * n_a;
  int* Jl = jlo + r * (n_a + 1);
  int* Jh = jhi + r * (n_a + 1);
  const int k = threadIdx.x, lane = k & (kWave - 1), wave = k / kWave;
  __shared__ int s_row[STAGED && kTrWinStage > 0 ? kTrWinStage : 1];
  if constexpr (STAGED) {
    for (int j = k; j < n_a; j += kTrBlock) s_row[j] = L[j];
    __syncthreads();
    L = s_row;
  }
  int j0, j1;
  row_chunk(n_a, k, j0, j1);
  // the chunk's extremes, the range check and the decreasing pairs (the pair (j0 - 1, j0) is this thread's)
  int cmax = -1, cmin = n_a;
  bool bad = false, turned = false;
  int prev = j0 > 0 && j0 < j1 ? L[j0 - 1] : -1;
  for (int j = j0; j < j1; ++j) {
    const int v = L[j];
    bad |= v < 0 || v > n_a - 2;
    turned |= v < prev;
    cmax = v > cmax ? v : cmax;
    cmin = v < cmin ? v : cmin;
    prev = v;
  }
  if (__syncthreads_or(bad)) {   // block-uniform: nothing of this row is written
    if (k == 0) atomicOr(flag, 1);
    return;
  }
  // inclusive scans in the wave, the wave totals through LDS
  int pmax = cmax, smin = cmin;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int u = __shfl_up(pmax, o, kWave), v = __shfl_down(smin, o, kWave);
    if (lane >= o) pmax = u > pmax ? u : pmax;
    if (lane + o < kWave) smin = v < smin ? v : smin;
  }
  __shared__ int s_max[kTrWaves], s_min[kTrWaves];
  __shared__ long long s_sum[kTrWaves];
  if (lane == kWave - 1) s_max[wave] = pmax;
  if (lane == 0) s_min[wave] = smin;
  // exclusive: the neighbour lane's inclusive value, then the waves before / after this one
  int M = __shfl_up(pmax, 1, kWave), m = __shfl_down(smin, 1, kWave);
  if (lane == 0) M = -1;
  if (lane == kWave - 1) m = n_a;
  __syncthreads();
  for (int q = 0; q < kTrWaves; ++q) {
    if (q < wave) M = s_max[q] > M ? s_max[q] : M;
    if (q > wave) m = s_min[q] < m ? s_min[q] : m;
  }
  // every entry is in [0, n_a - 2] from here on, so M in [-1, n_a - 2] and m in [0, n_a]
  long long sum = 0;   // sum of the jhi this thread writes minus sum of the jlo it writes
  for (int j = j0; j < j1; ++j) {
    const int v = L[j];
    if (v > M) {
      for (int d = M + 1; d <= v; ++d) Jl[d] = j;
      sum -= (long long)(v - M) * j;
      M = v;
    }
  }
  if (k == kTrBlock - 1) {   // its inclusive prefix is the row's maximum
    for (int d = M + 1; d <= n_a; ++d) Jl[d] = n_a;
    sum -= (long long)(n_a - M) * n_a;
  }
  for (int j = j1 - 1; j >= j0; --j) {
    const int v = L[j];
    if (v < m) {
      for (int d = v; d < m; ++d) Jh[d] = j + 1;
      sum += (long long)(m - v) * (j + 1);
      m = v;
    }
  }
  if (k == 0) {   // its inclusive suffix is the row's minimum (n_a >= 2: chunk 0 is never empty)
    for (int d = 0; d < m; ++d) Jh[d] = 0;
    Jh[n_a] = n_a;
    sum += n_a;
  }
  // the row's window length and whether any pair turned
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
  if (lane == 0) s_sum[wave] = sum;
  const int any_turned = __syncthreads_or(turned);
  if (k == 0) {
    long long tot = 0;
    for (int q = 0; q < kTrWaves; ++q) tot += s_sum[q];
    if (tot > (long long)kTrAnyCap * ((long long)n_a + 1)) atomicOr(flag, 2);
    if (any_turned) atomicAdd(flag + 1, 1);
  }
}

int32_t tr_build_windows(aiy_handle* h, int n_cal, int S, int n_a, int T, const int* lo, int* jlo, int* jhi,
                         int* d_flag, int* rows_turned, hipStream_t st) {
  AIY_HIP(h, hipMemsetAsync(d_flag, 0, 2 * sizeof(int), st));
  const long long n_tc = (long long)T * n_cal;   // (period, calibration) pairs, <= 65535 per launch
  for (long long z0 = 0; z0 < n_tc; z0 += 65535) {
    const unsigned nz = (unsigned)std::min<long long>(65535, n_tc - z0);
    if (n_a <= kTrWinStage)
      hipLaunchKernelGGL(tr_windows_kernel<true>, dim3(S, nz), dim3(kTrBlock), 0, st, S, n_a, (size_t)z0 * S, lo, jlo,
                         jhi, d_flag);
    else
      hipLaunchKernelGGL(tr_windows_kernel<false>, dim3(S, nz), dim3(kTrBlock), 0, st, S, n_a, (size_t)z0 * S, lo, jlo,
                         jhi, d_flag);
  }
  AIY_CHECK_LAUNCH(h);
  int flag[2] = {0, 0};
  AIY_HIP(h, hipMemcpyAsync(flag, d_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  if (flag[0] & 1)
    return fail(h, AIY_ERR_UNSUPPORTED, "transition lottery check failed: a row of lo leaves [0, n_a - 2]");
  if (flag[0] & 2)
    return fail(h, AIY_ERR_UNSUPPORTED,
                "transition lottery check failed: a row of lo is too disordered for the windowed pull (its windows "
                "hold more than %d (n_a + 1) = %lld sources)",
                kTrAnyCap, (long long)kTrAnyCap * ((long long)n_a + 1));
  if (rows_turned) *rows_turned = flag[1];
  return AIY_OK;
}

struct TrFwd {
  int n_cal, S, n_a, T, nblk;
  const double* wlo;     // [T][n_cal][S][n_a]
  const int* jb;         // [T][n_cal][S][n_a + 1]; ANY: jlo
  const int* jhi;        // ANY: [T][n_cal][S][n_a + 1]
  const int* lo;         // ANY: [T][n_cal][S][n_a]
  const double* P;       // [n_cal][S][S]
  const double* a_grid;  // [n_cal][n_a]
  const double* R;       // [n_cal][T + 1] (WITH_C)
  const double* w;
  const double* lab;     // [n_cal][S]
  double* Kpart;         // [T + 1][n_cal][nblk]
  double* Cpart;         // [T][n_cal][nblk]
};

// Ks[0] = sum mass_0 a with the column partition of the forward step.
__global__ __launch_bounds__(kTrBlock) void tr_K0_kernel(TrFwd A, const double* __restrict__ mass) {
  const int cal = blockIdx.y, S = A.S, n_a = A.n_a;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const int d = blockIdx.x * kTrCols + lane;
  double v = 0.0;
  if (d < n_a) {
    const double ad = A.a_grid[(size_t)cal * n_a + d];
    for (int s = wave; s < S; s += kTrWaves) v += mass[((size_t)cal * S + s) * n_a + d] * ad;
  }
  __shared__ double red[kTrWaves];
  const double k = tr_block_sum(v, red);
  if (threadIdx.x == 0) A.Kpart[(size_t)cal * A.nblk + blockIdx.x] = k;
}

// ANY: the windowed pull of rows that need not be monotone (A.jb = jlo, A.jhi, A.lo); everything
// behind the pull is the same code.
template <bool WITH_C, bool ANY>
__global__ __launch_bounds__(kTrBlock) void tr_forward_kernel(TrFwd A, int t, const double* __restrict__ mass,
                                                              double* __restrict__ mass_out) {
  const int S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  const int d = p.col;
  const size_t trow = ((size_t)t * A.n_cal + p.cal) * S;   // first row of (t, cal) in the [T][n_cal][S][.] arrays
  const double* ag = A.a_grid + (size_t)p.cal * n_a;
  const double ad = ag[p.active ? d : n_a - 1];
  double Rt = 0.0, wt = 0.0;
  if constexpr (WITH_C) {
    Rt = A.R[(size_t)p.cal * (A.T + 1) + t];
    wt = A.w[(size_t)p.cal * (A.T + 1) + t];
  }
  __shared__ double Tl[kTrTile];   // T_s[d] of the block's columns
  double cacc = 0.0;
  // pull: wave w forms T_s of the block's columns for s = w, w + 4, ...
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves) {
    double ls = 0.0;
    if constexpr (WITH_C) ls = wt * A.lab[p.rows + s];
    const size_t jrow = (trow + s) * (size_t)(n_a + 1), lrow = (trow + s) * (size_t)n_a;
    const double* Q = mass + (p.rows + s) * (size_t)n_a;
    if constexpr (ANY)
      Tl[s * kTrCols + p.lane] = tr_pull<WITH_C, true>(A.jb + jrow, A.wlo + lrow, Q, d, p.active, p.lane, ag, Rt, ls, ad,
                                                       cacc, A.lo + lrow, A.jhi + jrow);
    else
      Tl[s * kTrCols + p.lane] =
          tr_pull<WITH_C>(A.jb + jrow, A.wlo + lrow, Q, d, p.active, p.lane, ag, Rt, ls, ad, cacc);
  }
  __syncthreads();
  // mix: wave w forms mass'[s'] for s' = w, w + 4, ...
  const double* Pc = A.P + p.rows * S;
  double kacc = 0.0;
#pragma unroll 1
  for (int sp = p.wave; sp < S; sp += kTrWaves) {
    const double acc = tr_mix_forward(Pc, Tl, S, sp, p.lane);
    if (p.active) {
      mass_out[(p.rows + sp) * (size_t)n_a + d] = acc;
      kacc += acc * ad;
    }
  }
  __shared__ double red[kTrWaves];
  const double k = tr_block_sum(kacc, red);
  if (threadIdx.x == 0) A.Kpart[((size_t)(t + 1) * A.n_cal + p.cal) * A.nblk + blockIdx.x] = k;
  if constexpr (WITH_C) {
    const double c = tr_block_sum(cacc, red);
    if (threadIdx.x == 0) A.Cpart[((size_t)t * A.n_cal + p.cal) * A.nblk + blockIdx.x] = c;
  }
}

// Ks[cal][k] (k <= T) and C[cal][t] (t < T): the blocks' partials in block order.
__global__ void tr_sum_kernel(TrFwd A, double* __restrict__ Ks, double* __restrict__ C) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nK = (long long)(A.T + 1) * A.n_cal;
  if (q < nK) {
    const int k = (int)(q / A.n_cal), cal = (int)(q % A.n_cal);
    const double* p = A.Kpart + (size_t)q * A.nblk;
    double v = 0.0;
    for (int b = 0; b < A.nblk; ++b) v += p[b];
    Ks[(size_t)cal * (A.T + 1) + k] = v;
  }
  if (C != nullptr && q < (long long)A.T * A.n_cal) {
    const int t = (int)(q / A.n_cal), cal = (int)(q % A.n_cal);
    const double* p = A.Cpart + (size_t)q * A.nblk;
    double v = 0.0;
    for (int b = 0; b < A.nblk; ++b) v += p[b];
    C[(size_t)cal * A.T + t] = v;
  }
}

template <bool ANY>
static void launch_fwd(const TrFwd& A, int t, bool with_c, const double* src, double* dst, hipStream_t st) {
  const dim3 grid(A.nblk, A.n_cal);
  if (with_c) hipLaunchKernelGGL((tr_forward_kernel<true, ANY>), grid, dim3(kTrBlock), 0, st, A, t, src, dst);
  else hipLaunchKernelGGL((tr_forward_kernel<false, ANY>), grid, dim3(kTrBlock), 0, st, A, t, src, dst);
}

// g[dist][j] = ((mass[dist][0][j] + mass[dist][1][j]) + ...) + mass[dist][S - 1][j]: the marginal
// over assets of a stack of [S][n_a] masses.  A thread owns one (distribution, node) and adds
// its S values in ascending s; consecutive lanes own consecutive nodes.  No atomics.
__global__ __launch_bounds__(kTrBlock) void tr_marginal_kernel(int S, int n_a, const double* __restrict__ mass,
                                                               double* __restrict__ g) {
  const int j = blockIdx.x * kTrBlock + threadIdx.x;
  if (j >= n_a) return;
  const double* m = mass + (size_t)blockIdx.y * S * n_a + j;
  double v = m[0];
  for (int s = 1; s < S; ++s) v += m[(size_t)s * n_a];
  g[(size_t)blockIdx.y * n_a + j] = v;
}

// transition_common.h: the marginals of n_dist distributions, full width over nodes x distributions
void tr_launch_marginal(long long n_dist, int S, int n_a, const double* mass, double* g, hipStream_t st) {
  const unsigned nx = (unsigned)((n_a + kTrBlock - 1) / kTrBlock);
  for (long long d0 = 0; d0 < n_dist; d0 += 65535) {   // grid.y <= 65535
    const unsigned ny = (unsigned)std::min<long long>(65535, n_dist - d0);
    hipLaunchKernelGGL(tr_marginal_kernel, dim3(nx, ny), dim3(kTrBlock), 0, st, S, n_a,
                       mass + (size_t)d0 * S * n_a, g + (size_t)d0 * n_a);
  }
}

// ---------------------------------------------------------------------------------
// Work space (caller-owned): every region starts on a 256-byte boundary.
// ---------------------------------------------------------------------------------
struct TrWork {
  double *tab, *alt, *kpart, *cpart, *ks, *c;   // tab: (m, c) x ping-pong; alt: ping-pong partner of mass
  int *jb, *flag;
  size_t bytes, tab_doubles;                    // tab_doubles: one [n_cal][S][n_a + 1] table
  int nblk;
};

static bool tr_sizes_ok(int n_cal, int S, int n_a, int T) {
  return tr_pull_sizes_ok(n_cal, S, n_a) && T >= 1;
}

static TrWork tr_work_take(Carve& c, int n_cal, int S, int n_a, int T) {
  TrWork L;
  L.nblk = tr_nblk(n_a);
  L.tab_doubles = (size_t)n_cal * S * (n_a + 1);
  L.tab = c.take<double>(4 * L.tab_doubles);
  L.jb = c.take<int>((size_t)T * n_cal * S * (n_a + 1));
  L.alt = c.take<double>((size_t)n_cal * S * n_a);
  L.kpart = c.take<double>((size_t)(T + 1) * n_cal * L.nblk);
  L.cpart = c.take<double>((size_t)T * n_cal * L.nblk);
  L.ks = c.take<double>((size_t)n_cal * (T + 1));
  L.c = c.take<double>((size_t)n_cal * T);
  L.flag = c.take<int>(256 / sizeof(int));
  L.bytes = c.bytes();
  return L;
}
static TrWork tr_work(Carve c, int n_cal, int S, int n_a, int T) { return tr_work_take(c, n_cal, S, n_a, T); }

// aiy_transition_forward_any: tr_work's regions, then the second window array and the counters
// (the check's flag word and the number of turned rows).
struct TrAnyWork {
  TrWork w;       // w.jb holds jlo
  int *jhi, *count;
  size_t bytes;
};
static TrAnyWork tr_any_work(Carve c, int n_cal, int S, int n_a, int T) {
  TrAnyWork L;
  L.w = tr_work_take(c, n_cal, S, n_a, T);
  L.jhi = c.take<int>((size_t)T * n_cal * S * (n_a + 1));
  L.count = c.take<int>(256 / sizeof(int));
  L.bytes = c.bytes();
  return L;
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_transition_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T) {
  if (!tr_sizes_ok(n_cal, S, n_a, T)) return -1;
  return (int64_t)tr_work(Carve(), n_cal, S, n_a, T).bytes;
}

extern "C" int64_t aiy_transition_any_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T) {
  if (!tr_sizes_ok(n_cal, S, n_a, T)) return -1;
  return (int64_t)tr_any_work(Carve(), n_cal, S, n_a, T).bytes;
}

extern "C" int32_t aiy_transition_backward(aiy_handle* h, const aiy_transition_model* M, void* work, int32_t* lo,
                                           double* wlo, double* m0_out, double* c0_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (!M) return fail(h, AIY_ERR_ARG, "null model");
  const int n_cal = M->n_cal, S = M->S, n_a = M->n_a, T = M->T;
  int32_t rc = tr_check(h, n_cal, S, n_a, true, T);
  if (rc) return rc;
  if (!M->a_grid || !M->P || !M->lab || !M->beta || !M->crra || !M->R || !M->w || !M->m_term || !M->c_term)
    return fail(h, AIY_ERR_ARG, "null model array");
  if (!work || !lo || !wlo) return fail(h, AIY_ERR_ARG, "null buffer");
  if ((m0_out == nullptr) != (c0_out == nullptr)) return fail(h, AIY_ERR_ARG, "m0_out/c0_out must both be set or NULL");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const TrWork L = tr_work(Carve(work), n_cal, S, n_a, T);
  double* tab = L.tab;
  auto m_buf = [&](int b) { return tab + (size_t)(2 * b) * L.tab_doubles; };
  auto c_buf = [&](int b) { return tab + (size_t)(2 * b + 1) * L.tab_doubles; };
  const size_t per = (size_t)n_cal * S * n_a;   // one period's lottery
  TrBack A;
  A.S = S; A.n_a = n_a; A.T = T;
  A.a_grid = M->a_grid; A.P = M->P; A.lab = M->lab; A.beta = M->beta; A.crra = M->crra; A.R = M->R; A.w = M->w;
  const double* mi = M->m_term;
  const double* ci = M->c_term;
  for (int u = T; u >= 1; --u) {   // tables u -> u - 1 (buffer u & 1), lottery of period u < T
    A.u = u;
    A.m_in = mi; A.c_in = ci;
    A.m_out = m_buf(u & 1); A.c_out = c_buf(u & 1);
    A.lo = u < T ? lo + (size_t)u * per : nullptr;
    A.wlo = u < T ? wlo + (size_t)u * per : nullptr;
    launch_back(A, n_cal, true, st);
    mi = A.m_out; ci = A.c_out;
  }
  A.u = 0;   // lottery of period 0 from the tables of period 0
  A.m_in = mi; A.c_in = ci;
  A.m_out = nullptr; A.c_out = nullptr;
  A.lo = lo; A.wlo = wlo;
  launch_back(A, n_cal, false, st);
  AIY_CHECK_LAUNCH(h);
  if (m0_out) {
    AIY_HIP(h, hipMemcpyAsync(m0_out, mi, L.tab_doubles * sizeof(double), hipMemcpyDeviceToDevice, st));
    AIY_HIP(h, hipMemcpyAsync(c0_out, ci, L.tab_doubles * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  return AIY_OK;
}

// The forward sweep of aiy_transition_forward; with `marg` also the marginal of every period's
// mass, [T + 1][n_cal][n_a], one tr_marginal_kernel launch behind the launch that wrote the mass.
// ANY: aiy_transition_forward_any's -- `work` is tr_any_work's, the check is tr_build_windows and
// the number of turned rows goes to rows_turned (host, may be null).
// With `masses` (aiy_transition_forward_masses) also every period's mass, [T + 1][n_cal][S][n_a]: a
// device-to-device copy of mass_0 and of each period's freshly written buffer; no launch differs.
template <bool ANY>
static int32_t tr_forward_sweep(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, const int32_t* lo,
                                const double* wlo, const double* P, const double* a_grid, const double* R,
                                const double* w, const double* lab, void* work, double* mass, double* Ks_out,
                                double* C_out, double* marg, aiy_stream stream, int32_t* rows_turned = nullptr,
                                double* masses = nullptr) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a, true, T);
  if (rc) return rc;
  if (!lo || !wlo || !P || !a_grid || !work || !mass || !Ks_out) return fail(h, AIY_ERR_ARG, "null buffer");
  if (C_out && (!R || !w || !lab)) return fail(h, AIY_ERR_ARG, "C_out needs R, w and lab");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  TrWork L;
  int* jhi = nullptr;
  if constexpr (ANY) {
    const TrAnyWork LA = tr_any_work(Carve(work), n_cal, S, n_a, T);
    L = LA.w;
    jhi = LA.jhi;
    // the windows of every period and the row checks, before anything is pushed
    int turned = 0;
    rc = tr_build_windows(h, n_cal, S, n_a, T, lo, L.jb, jhi, LA.count, &turned, st);
    if (rc) return rc;
    if (rows_turned) *rows_turned = turned;
  } else {
    L = tr_work(Carve(work), n_cal, S, n_a, T);
    // inverse index of every period and the row check, before anything is pushed
    rc = tr_build_ranges(h, n_cal, S, n_a, T, lo, L.jb, L.flag, st);
    if (rc) return rc;
  }
  int* jb = L.jb;
  double *alt = L.alt, *d_Ks = L.ks, *d_C = L.c;
  TrFwd A;
  A.n_cal = n_cal; A.S = S; A.n_a = n_a; A.T = T; A.nblk = L.nblk;
  A.wlo = wlo; A.jb = jb; A.P = P; A.a_grid = a_grid; A.R = R; A.w = w; A.lab = lab;
  A.jhi = jhi; A.lo = ANY ? lo : nullptr;
  A.Kpart = L.kpart;
  A.Cpart = L.cpart;
  const bool with_c = C_out != nullptr;
  const size_t per_marg = (size_t)n_cal * n_a, per_mass = (size_t)n_cal * S * n_a;
  hipLaunchKernelGGL(tr_K0_kernel, dim3(L.nblk, n_cal), dim3(kTrBlock), 0, st, A, (const double*)mass);
  if (marg) tr_launch_marginal(n_cal, S, n_a, mass, marg, st);
  if (masses) AIY_HIP(h, hipMemcpyAsync(masses, mass, per_mass * sizeof(double), hipMemcpyDeviceToDevice, st));
  for (int t = 0; t < T; ++t) {   // period t reads mass (t even) / alt (t odd)
    const double* src = (t & 1) ? alt : mass;
    double* dst = (t & 1) ? mass : alt;
    launch_fwd<ANY>(A, t, with_c, src, dst, st);
    if (marg) tr_launch_marginal(n_cal, S, n_a, dst, marg + (size_t)(t + 1) * per_marg, st);
    if (masses)
      AIY_HIP(h, hipMemcpyAsync(masses + (size_t)(t + 1) * per_mass, dst, per_mass * sizeof(double),
                                hipMemcpyDeviceToDevice, st));
  }
  const long long n_sum = (long long)(T + 1) * n_cal;
  hipLaunchKernelGGL(tr_sum_kernel, dim3((unsigned)((n_sum + 255) / 256)), dim3(256), 0, st, A, d_Ks,
                     with_c ? d_C : (double*)nullptr);
  AIY_CHECK_LAUNCH(h);
  if (T & 1)
    AIY_HIP(h, hipMemcpyAsync(mass, alt, (size_t)n_cal * S * n_a * sizeof(double), hipMemcpyDeviceToDevice, st));
  AIY_HIP(h, hipMemcpyAsync(Ks_out, d_Ks, (size_t)n_cal * (T + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (with_c) AIY_HIP(h, hipMemcpyAsync(C_out, d_C, (size_t)n_cal * T * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  return AIY_OK;
}

extern "C" int32_t aiy_transition_forward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                          const int32_t* lo, const double* wlo, const double* P, const double* a_grid,
                                          const double* R, const double* w, const double* lab, void* work, double* mass,
                                          double* Ks_out, double* C_out, aiy_stream stream) {
  return tr_forward_sweep<false>(h, n_cal, S, n_a, T, lo, wlo, P, a_grid, R, w, lab, work, mass, Ks_out, C_out,
                                 nullptr, stream);
}

extern "C" int32_t aiy_transition_forward_marginals(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                                    const int32_t* lo, const double* wlo, const double* P,
                                                    const double* a_grid, const double* R, const double* w,
                                                    const double* lab, void* work, double* mass, double* Ks_out,
                                                    double* C_out, double* marg_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (!marg_out) return fail(h, AIY_ERR_ARG, "null marg_out");
  return tr_forward_sweep<false>(h, n_cal, S, n_a, T, lo, wlo, P, a_grid, R, w, lab, work, mass, Ks_out, C_out,
                                 marg_out, stream);
}

extern "C" int32_t aiy_transition_forward_masses(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                                 const int32_t* lo, const double* wlo, const double* P,
                                                 const double* a_grid, const double* R, const double* w,
                                                 const double* lab, void* work, double* mass, double* Ks_out,
                                                 double* C_out, double* mass_path_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (!mass_path_out) return fail(h, AIY_ERR_ARG, "null mass_path_out");
  return tr_forward_sweep<false>(h, n_cal, S, n_a, T, lo, wlo, P, a_grid, R, w, lab, work, mass, Ks_out, C_out,
                                 nullptr, stream, nullptr, mass_path_out);
}

extern "C" int32_t aiy_transition_forward_any(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                              const int32_t* lo, const double* wlo, const double* P,
                                              const double* a_grid, const double* R, const double* w,
                                              const double* lab, void* work, double* mass, double* Ks_out,
                                              double* C_out, double* marg_out, int32_t* rows_turned_out,
                                              aiy_stream stream) {
  return tr_forward_sweep<true>(h, n_cal, S, n_a, T, lo, wlo, P, a_grid, R, w, lab, work, mass, Ks_out, C_out,
                                marg_out, stream, rows_turned_out);
}
