// Device-resident general equilibrium of the stationary Aiyagari household (build-defined
// row E1): the WHOLE root search of every calibration in ONE launch.
//
// aiy_ge_stationary's host loop (ge.hip) steps all calibrations of a batch together: each
// K_s(r) evaluation is an EGM solve (host checks every 32 cycles), a lottery launch and one
// distribution-solve launch, and every launch lasts as long as its slowest calibration.
// Here each calibration owns a CLUSTER of G workgroups (512 threads, one per CU; the same
// clusters as the resident histogram, hist_resident.hip) that runs, with no host round
// trip and no waiting for other calibrations:
//
//   loop over K_s(r) evaluations (the search policy GeEval of ge_search.h -- plan() before an
//   evaluation, accept() after it, the same two calls as ge.hip's loop -- every workgroup of
//   the cluster on bit-identical inputs):
//     prices      R = 1 + r, w = (1 - alpha) (alpha / (r + delta))^(alpha / (1 - alpha))
//     start       secant start of the household tables and the mass from the last two
//                 evaluations (x0 = cur + theta (cur - prev)), as ge.hip
//     EGM         cycles of solve_Aiyagari (Aiyagari_Support.py:1478-1504) over the
//                 workgroup's own asset nodes: V[s'][i] = R c_{s'}(R a_i + w l_{s'})^-rho by
//                 the wavefront-cooperative window interpolation of egm.hip (rows another
//                 workgroup wrote: `sc1` loads), E = beta sum_s' V P in NumPy's pairwise
//                 order, c = E^(-1/rho), m = a + c written write-through (`sc1`); the HARK
//                 stopping rule (sup-norm of the tables <= tol, NaN stops) rides on the
//                 cycle's cluster barrier; the geometric extrapolation of ge.hip every 32
//                 cycles
//     lottery     (s, j) -> a' = m - c_s(m), m = R a_j + w l_s, bracket in the asset grid
//     histogram   BiCGSTAB on (I - T) mass = 0 (hist_bicg.h, the kernel of hist_krylov.hip)
//     K_s         sum mass a (cluster reduction); f = K_s - K_d; loose-bracketing sign test
//   until the search is done; workgroup 0 writes r, K, K_s, the counts and the status.
//
// The kernel's phases -- ge_vote, ge_secant_tables, the lottery, ge_mass_start, ge_capital,
// ge_write_out -- are __forceinline__ functions over GeCtx and the file-scope LDS, one body with
// one register allocation; its two solves are functions of their own, each with its own
// allocation: the household solve (ge_household_isolated: ge_household_solve with the cycle of
// one CRRA kind, ge_extrapolate, ge_anderson) and the push form of the BiCGSTAB solve
// (hk_solve_isolated, hist_bicg.h).
//
// The launch ends when the slowest calibration's whole search ends (the host loop's launches
// each waited for the slowest calibration of that step).  Workgroup placement: block b runs
// on XCD b % 8 (observed dispatch, speed only), so the blocks are dealt XCD-contiguous and a
// cluster's exchanges mostly stay inside one XCD's L2; correctness never depends on it
// (every cross-workgroup value is written and read at agent scope).
#include "common.h"
#include "egm_common.h"
#include "ge_search.h"
#include "hist_bicg.h"
#include "hist_cluster.h"
#include "internal.h"

#include <algorithm>
#include <cmath>

namespace aiy {

// Workgroup size (template TH; the plan launches 512).  A cycle / matvec costs about the same
// per column of a workgroup whatever the thread organisation: 26.8 / 23.7 us at G = 10
// (1 000 columns, 512 threads x 2 columns), 23.0 / 25.5 us with 1 024 threads x 1 column
// (spills at 128 VGPRs), 15.5 / 12.4 us at G = 21 (477 columns, 512 threads x 1 column)
// (profiles/r03i_*, r03j_*): a cluster's time scales with its columns per CU.
constexpr int kGeTHMax = 1024;
constexpr int kGeWavesMax = kGeTHMax / kWave;   // 16
constexpr int kGeMaxTiles = 16;           // 64-node tiles of one workgroup's own columns (<= 1024)
constexpr int kGeBufs = 5;                // table buffers per calibration: ping, pong, cur, prev, init
// Periodic Anderson mixing of the EGM cycles (AIY_OPT_GE_ANDERSON): every p-th cycle the
// household iterate moves to the type-II Anderson combination of the last kGeAaM + 1 plain
// cycles (their outputs kept in a ring of kGeAaHist slots), plain cycles in between.  A CPU
// study on the oracle's EGM (scratch prototype; N_a = 3 000, the Table II cells near their
// roots, warm and cold starts) put it at 1.5-2.5x fewer cycles to the same HARK stopping rule
// than the period-32 geometric extrapolation it replaces (m = 3, p = 12: 97-128 against
// 196-248 cycles from a start 2e-2 away in r, 49-97 against 112-178 from 2e-5).
constexpr int kGeAaM = 3;
constexpr int kGeAaHist = kGeAaM + 2;
// One asset column per thread (G >= 20 at N_a = 10 000: every relaunch and the 8-GPU shape):
// the BiCGSTAB solve's alpha reduction rides on its first matvec's barrier (hist_bicg.h
// FUSEA), one cluster reduction per iteration instead of two.  A diagnostic build with
// -DAIY_DIAG_NO_FUSEA runs the plain recurrence everywhere (A/B timing).
#ifdef AIY_DIAG_NO_FUSEA
constexpr bool kGeFuseA = false;
#else
constexpr bool kGeFuseA = true;
#endif
// With two columns per thread (the first, 24-cell launch of a Table II sweep) the default keeps the
// two-reduction form: FUSEA there (-DAIY_FUSEA_KC2=2: u's own points read back from HBM beside the
// new p; =1: prefetched across the second reduction) measured SLOWER, 411-427 against 481-491 GE
// solves/s for the Table II sweep (gpurun_out/r08e_abaa_*: the last wave, which sweeps the riding
// reduction, owns columns at two per thread and delays its gather; the x loads move behind the
// matvec)
#ifndef AIY_FUSEA_KC2
#define AIY_FUSEA_KC2 0
#endif
constexpr bool kGeFuseAKc2 = AIY_FUSEA_KC2 != 0;
// The asset-grid solve of an i.i.d. cell (hist_bicg.h IID) at two columns per thread: its vectors are
// one value per column, all in registers, so the register pressure that ruled the riding reduction
// out above is gone; the last wave still owns columns.  -DAIY_IID_FUSEA_KC2=0|1 builds either.
#ifndef AIY_IID_FUSEA_KC2
#define AIY_IID_FUSEA_KC2 0
#endif
constexpr bool kGeIidFuseAKc2 = AIY_IID_FUSEA_KC2 != 0;
template <int NW>
constexpr size_t ge_egm_lds() { return (size_t)NW * (8 * kTile + 4 * kWin) * sizeof(double); }   // V tiles + windows

struct GeCalDev {
  double alpha, delta, disc, r_lo, r_hi;
};

struct GeState;
struct GeRun {
  int n_cal, S, n_a, G, nj, cap, n_work;   // n_work = G x (calibrations of this launch)
  const double* a_grid;   // [n_cal][n_a]
  const double* P;        // [n_cal][S][S]
  const double* lab;      // [n_cal][S]
  const double* beta;     // [n_cal]
  const double* crra;     // [n_cal]
  const GeCalDev* cal;    // [n_cal]
  int method;
  double r_tol, egm_tol, hist_tol;
  int max_steps, max_cyc, max_hist;
  int warm_hist, warm_egm, secant, loose, extrap;
  int extrap_period;      // EGM cycles between extrapolation checks (>= 4)
  int iid_on;             // AIY_OPT_HIST_IID: i.i.d. cells take the collapsed household cycle and solve
  int* out_iid;           // [n_cal] 1: the calibration's distribution solves ran on the asset grid
  int aa_period;          // EGM Anderson mixing every aa_period cycles (0: off; AIY_OPT_GE_ANDERSON)
  double* aah;            // [n_cal][kGeAaHist][S][n_a] the last kGeAaHist EGM outputs (c, own nodes)
  int logsec;             // log-secant bracketing (AIY_OPT_GE_LOGSEC, with loose bracketing)
  double loose_hist;      // loose-bracketing histogram tolerance (AIY_OPT_GE_LOOSE_HIST)
  double* qb;             // [n_cal][S][n_a] pull form: the matvec input rows
  int* ainv;              // [n_cal][S][n_a + 1] pull form: inverse lottery
  double* tab;            // [n_cal][kGeBufs][2][S][n_a + 1]
  double* mass;           // [n_cal][S][n_a]
  double* pmass;          // [n_cal][S][n_a] previous evaluation's mass
  double* pg;             // [n_cal][S][n_a] BiCGSTAB p rows
  int* lo;                // [n_cal][S][n_a]
  double* wlo;            // [n_cal][S][n_a]
  double* slab;           // [launch cals][G][2][cap]
  int* span;              // [launch cals][G][SMAX][4]
  unsigned* ctr;          // [launch cals][kHcCtrStride]
  unsigned long long* gran;   // [launch cals][2][G][kHcRedRec]
  // rebalancing: a launch covers some calibrations (cal_ids) and stops at the next evaluation
  // boundary of every cluster once stop_at of them have finished; stopped ones save their
  // search state and the host relaunches them with larger clusters
  const int* cal_ids;     // [launch cals] cluster -> calibration
  GeState* saved;         // [n_cal] search state of a stopped calibration
  const int* resume;      // [n_cal] 1: start from saved[cal]
  unsigned* done_ctr;     // calibrations of this launch whose search has ended
  int stop_at;            // 0: never stop
  int* out_done;          // [n_cal] 1: search ended (outputs written), 0: stopped
  unsigned* err;
  double* out_r;
  double* out_K;
  double* out_Ks;
  int* out_steps;
  int* out_cyc;
  int* out_its;
  int* out_status;
  double* out_prof;       // [n_cal][kGeProf] workgroup 0's phase times (us) and counts
  double* out_evlog;      // [n_cal][kGeEvLog][kGeEvRec] per-evaluation record (measurement)
};
// per-calibration profile of the launch (workgroup 0, s_memrealtime at 100 MHz): EGM, lottery,
// distribution solve, K reduction + search, whole search (us); EGM cycles, matvecs, evaluations
constexpr int kGeProf = 8;
// per-evaluation log: r, (K_s - K_d) / K_d, EGM cycles, matvecs, loose, EGM + histogram us
constexpr int kGeEvLog = 32;
constexpr int kGeEvRec = 6;

// Search state of one calibration, one copy per workgroup (thread 0 writes, all read): the
// search and the planned evaluation (GeEval, ge_search.h), and the device's own bookkeeping.
struct GeState {
  GeEval ev;
  GeEvalOpts opt;          // the launch's search options: thread 0 plans from LDS (planning from the
                           // kernel arguments cost 32-48 B of scratch per lane)
  double Ks, dist, lam_prev, fext;
  int status, n, stop, nan_stop, moved, extrap;
  int in_hist;             // stopped (rebalancing) inside this evaluation's distribution solve
  int buf[kGeBufs];        // roles: 0 ping, 1 pong, 2 cur, 3 prev, 4 init -> buffer index
  long long cyc_sum, its_sum;
  unsigned long long t_egm, t_lot, t_hist, t_k, t0, t_ev0;
  unsigned nc_prev[2];
  unsigned nbc;            // counting barriers passed
};

// Cluster-wide reduction of nv per-thread values (bit v of kmax: NaN-propagating max, else
// sum) by hist_cluster.h's hc_reduce (every workgroup computes the same s_res), on the granules
// and the epoch counter the BiCGSTAB solves of the same launch use.  It is also a barrier:
// every workgroup has published after all its waves drained their stores.
template <int TH>
__device__ __forceinline__ bool ge_reduce(unsigned long long* gran, int G, int w, unsigned& ne, const double* vals,
                                          int nv, unsigned kmax, double (*s_part)[kGeWavesMax], double* s_res,
                                          int* s_flag, unsigned* err) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return hc_reduce<TH>(gran, G, w, ne, vals, nv, kmax, s_part, s_res, s_flag, err, [] {});
}

// Interpolation pass over the workgroup's own asset columns, one 64-column tile per wave at
// a time (wave wv: tiles wv, wv + 8; column j = j0 + 64 tile + lane = j0 + tid + 512 k, the
// hist_bicg.h column of the same thread): for every row s of `src` (S rows of n_a + 1
// nodes) the HARK LinearInterp at q = R a_j + Wl[s], by the window search of egm.hip over
// agent-scope loads; sink(tile, lane column, s, q, value) takes the result.
template <int SMAX, int NW, typename Sink, typename Begin, typename End>
__device__ __forceinline__ void ge_rows_pass(int S, int n_a, int j0, int j1, const double* __restrict__ a_grid,
                                             const double* __restrict__ src_m, const double* __restrict__ src_c,
                                             double R, const double* s_Wl, int* s_hint, double* lds_win,
                                             Sink&& sink, Begin&& begin, End&& end) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int n = n_a, n1 = n_a + 1;
  const int ntile = (j1 - j0 + kTile - 1) / kTile;
  double* X = lds_win + (size_t)wv * 4 * kWin;
  double* Y = X + kWin;
  double* XB = X + 2 * kWin;
  double* YB = X + 3 * kWin;
#pragma unroll 1
  for (int tile = wv; tile < ntile; tile += NW) {
    const int jr = j0 + tile * kTile + lane;
    const int j = jr < j1 ? jr : j1 - 1;   // lanes past the range repeat the last column
    const double a = a_grid[j];
    int* hint = s_hint + tile * SMAX;
    auto fetch = [&](int r, RowWin& wn) {
      const int rr = r < S ? r : S - 1;
      load_win<true>(src_m + (size_t)rr * n1, src_c + (size_t)rr * n1, n, win_base(hint[rr], n1), lane, wn);
    };
    unsigned redo = 0u;
    auto step_unit = [&](int u, const RowWin& wa, const RowWin& wb) {
      const int ra = 2 * u, rb = 2 * u + 1;
      if (ra >= S) return;   // wave-uniform
      const bool has_b = rb < S;
      const int rbb = has_b ? rb : ra;
      const bool na = __any(stage_win(wa, n, X, Y, lane));
      const bool nb = __any(stage_win(wb, n, XB, YB, lane));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const double qa = R * a + s_Wl[ra];   // mNextArray (AS:1024)
      const double qb = R * a + s_Wl[rbb];
      int lba, lbb;
      bool oka, okb;
      const double fa = search_win(wa.base, na, n, qa, X, Y, lba, oka);
      const double fb = search_win(wb.base, nb, n, qb, XB, YB, lbb, okb);
      hint[ra] = __builtin_amdgcn_readfirstlane(lba);
      if (has_b) hint[rb] = __builtin_amdgcn_readfirstlane(lbb);
      if (__any(!oka)) redo |= 1u << ra;
      else sink(tile, jr, j, ra, qa, fa);
      if (has_b) {
        if (__any(!okb)) redo |= 1u << rb;
        else sink(tile, jr, j, rb, qb, fb);
      }
    };
    RowWin a0, b0, a1, b1;
    fetch(0, a0);
    fetch(1, b0);
    begin(tile, j);   // (its loads behind the first windows': they are needed last, in end())
#pragma unroll 1
    for (int u = 0; 2 * u < S; u += 2) {
      fetch(2 * u + 2, a1);
      fetch(2 * u + 3, b1);
      step_unit(u, a0, b0);
      fetch(2 * u + 4, a0);
      fetch(2 * u + 5, b0);
      step_unit(u + 1, a1, b1);
    }
#pragma unroll 1
    while (redo != 0u) {   // wave-uniform
      const int s = __builtin_ctz(redo);
      redo &= redo - 1u;
      const double q = R * a + s_Wl[s];
      int lb;
      const double f = interp_row_global_agent(src_m + (size_t)s * n1, src_c + (size_t)s * n1, n, q, lb);
      hint[s] = __builtin_amdgcn_readfirstlane(lb);
      sink(tile, jr, j, s, q, f);
    }
    end(tile, j, a);
  }
}

// One EGM cycle of the workgroup's own nodes: src (cycle n - 1; nullptr: the terminal
// c = m) -> dst (cycle n).  Returns the workgroup's part of the HARK distance (track).
template <int SMAX, int SC, int PK, int NW>
__device__ __forceinline__ double ge_egm_cycle(int S, int n_a, int j0, int j1, const double* __restrict__ a_grid,
                                               const double* src_m, const double* src_c, double* dst_m,
                                               double* dst_c, bool track, double R, double beta, double gam,
                                               const double* s_Wl, const double* s_Pe, int* s_hint,
                                               double* lds_v, double* lds_win, double* ring, bool iid) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int n1 = n_a + 1;
  double* Vw = lds_v + (size_t)wv * SMAX * kTile;   // this wave's V[s'][lane]
  const int ntile = (j1 - j0 + kTile - 1) / kTile;
  double dmax = 0.0;
  if (src_m == nullptr) {   // terminal guess: IdentityFunction (AS:898) of mNextArray
#pragma unroll 1
    for (int tile = wv; tile < ntile; tile += NW) {
      const int jr = j0 + tile * kTile + lane;
      const int j = jr < j1 ? jr : j1 - 1;
      const double a = a_grid[j];
      for (int sp = 0; sp < S; ++sp) {
        const double c = (R * a + s_Wl[sp]) * 1.0;
        Vw[sp * kTile + lane] = R * marg_u<PK>(c, gam);   // read back by the same lane only
      }
      double c = 0.0;
      for (int s = 0; s < S; ++s) {
        if (s == 0 || !iid) {   // (i.i.d.: every state's expectation is state 0's, bit for bit)
          double sum;
          if constexpr (SC > 0) sum = pairwise_dot<SC>(Vw + lane, s_Pe + s * SC);
          else sum = np_pairwise_sum<SMAX>(S, [&](int t) { return Vw[t * kTile + lane] * uniform_f64(s_Pe[s * S + t]); });
          c = inv_marg<PK>(beta * sum, gam);
        }
        store_f64_agent(&dst_m[(size_t)s * n1 + j + 1], a + c);
        store_f64_agent(&dst_c[(size_t)s * n1 + j + 1], c);
        if (ring) store_f64_agent(&ring[(size_t)s * n_a + j], c);
        if (j == 0) {
          store_f64_agent(&dst_m[(size_t)s * n1], kBorrowNode);
          store_f64_agent(&dst_c[(size_t)s * n1], kBorrowNode);
        }
      }
    }
    return 0.0;
  }
  // tiles one after another per wave: the previous tables' values at the lane's node
  // (distance) in flight from the tile's start, V of the tile's rows (phase 1), then its
  // outputs (phase 2)
  constexpr int NP = SC > 0 ? SC : SMAX;
  double pmv[NP], pcv[NP];
  // (loaded whether or not the distance is tracked, rows past S clamped: behind a branch the
  // compiler cannot count these loads, and the wait for the tile's node a, loaded before them,
  // became a wait for all of them -- vmcnt(0) in front of the first window loads of every tile)
  auto begin = [&](int, int j) {
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      const int rr = s < S ? s : S - 1;
      pmv[s] = load_f64_agent(&src_m[(size_t)rr * n1 + j + 1]);
      pcv[s] = load_f64_agent(&src_c[(size_t)rr * n1 + j + 1]);
    }
  };
  // i.i.d. income (iid, wave-uniform: every row of P the same bits): E[s] is the same number for
  // every s, so the expectation and inv_marg run for s = 0 only and c, m are reused for s >= 1;
  // the stores and the distance stay per state
  auto end = [&](int, int j, double a) {   // phase 2 (each lane reads its own V)
    double c = 0.0, m = 0.0;
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      if (s < S) {
        __builtin_amdgcn_sched_barrier(0);   // one state's P reads at a time (no hoisting of all S x S)
        if (s == 0 || !iid) {
          double sum;
          if constexpr (SC > 0) sum = pairwise_dot<SC>(Vw + lane, s_Pe + s * SC);
          else sum = np_pairwise_sum<SMAX>(S, [&](int t) { return Vw[t * kTile + lane] * uniform_f64(s_Pe[s * S + t]); });
          const double E = beta * sum;                     // EndOfPrdvP (AS:1485)
          c = inv_marg<PK>(E, gam);                        // AS:1490
          m = a + c;                                       // AS:1499
        }
        store_f64_agent(&dst_m[(size_t)s * n1 + j + 1], m);
        store_f64_agent(&dst_c[(size_t)s * n1 + j + 1], c);
        if (ring) store_f64_agent(&ring[(size_t)s * n_a + j], c);   // Anderson history (own nodes)
        if (track) dmax = nan_max(dmax, nan_max(fabs(m - pmv[s]), fabs(c - pcv[s])));
        if (j == 0) {   // the (1e-7, 1e-7) node (AS:1503-1504)
          store_f64_agent(&dst_m[(size_t)s * n1], kBorrowNode);
          store_f64_agent(&dst_c[(size_t)s * n1], kBorrowNode);
        }
      }
    }
  };
  ge_rows_pass<SMAX, NW>(S, n_a, j0, j1, a_grid, src_m, src_c, R, s_Wl, s_hint, lds_win,
                     [&](int, int, int, int sp, double, double f) {
                       Vw[sp * kTile + lane] = R * marg_u<PK>(f, gam);   // RnextArray * MargValueFuncCRRA
                     },
                     begin, end);
  return dmax;
}

// The kernel's LDS at file scope, so the phases of the search (__forceinline__ functions) and
// ge_household_isolated address it directly: every kernel of this file reaches it, so it has one
// fixed address in all of them (no lookup in the separate function).
constexpr int kGeSmax = 8;    // the largest resident state count (Table II: 7)
extern __shared__ double ge_dyn[];                 // histogram: span buffer + v; EGM: V tiles + windows
__shared__ double ge_s_part[kHcRed][kGeWavesMax];
__shared__ double ge_s_res[kHcRed];
__shared__ int ge_s_flag;
__shared__ double ge_s_Pe[kGeSmax * kGeSmax];     // P[s][s'] unpadded (egm_phase2's layout)
__shared__ double ge_s_Wl[kGeSmax];               // w l(s')
__shared__ int ge_s_hint[kGeMaxTiles * kGeSmax];  // window hints per (tile, row)
__shared__ unsigned ge_s_nc;
__shared__ GeState ge_st;

template <int SMAX, int SC, int PK, int NW>
__device__ __forceinline__ double ge_egm_cycle_fn(int S, int n_a, int j0, int j1, const double* a_grid,
                                               const double* src_m, const double* src_c, double* dst_m,
                                               double* dst_c, bool track, double R, double beta, double gam,
                                               double* dyn, double* ring, bool iid) {
  return ge_egm_cycle<SMAX, SC, PK, NW>(S, n_a, j0, j1, a_grid, src_m, src_c, dst_m, dst_c, track, R, beta, gam,
                                        ge_s_Wl, ge_s_Pe, ge_s_hint, dyn, dyn + (size_t)NW * SMAX * kTile, ring, iid);
}

// lottery of the own columns on the final tables (hist.hip hist_lottery_kernel's arithmetic)
template <int SMAX, int NW>
__device__ __forceinline__ void ge_lottery_fn(int S, int n_a, int j0, int j1, const double* a_grid, const double* fm,
                                           const double* fc, double R, bool have_prev, int* LO, double* WL,
                                           bool write_through) {
  ge_rows_pass<SMAX, NW>(S, n_a, j0, j1, a_grid, fm, fc, R, ge_s_Wl, ge_s_hint, ge_dyn + (size_t)NW * SMAX * kTile,
                     [&](int, int jr, int, int s, double q, double c) {
                       if (jr >= j1) return;
                       const double ap = q - c;
                       const size_t o = (size_t)s * n_a + jr;
                       int d = -1;
                       if (have_prev) {   // last evaluation's bracket as the first guess
                         const int h = LO[o];
                         if (h >= 0 && h < n_a - 1 && a_grid[h] <= ap && ap < a_grid[h + 1]) d = h;
                       }
                       if (d < 0) {       // searchsorted(a_grid, a', 'right') - 1
                         int lo = 0, hi = n_a;
                         while (lo < hi) {
                           const int mid = lo + ((hi - lo) >> 1);
                           if (a_grid[mid] <= ap) lo = mid + 1; else hi = mid;
                         }
                         d = lo - 1;
                       }
                       d = d < 0 ? 0 : (d > n_a - 2 ? n_a - 2 : d);
                       double wl = (a_grid[d + 1] - ap) / (a_grid[d + 1] - a_grid[d]);
                       wl = wl < 0.0 ? 0.0 : (wl > 1.0 ? 1.0 : wl);
                       if (write_through) {   // the pull form reads foreign lottery entries
                         __hip_atomic_store(to_global(&LO[o]), d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                         store_f64_agent(&WL[o], wl);
                       } else {
                         LO[o] = d;
                         WL[o] = wl;
                       }
                     },
                     [](int, int) {}, [](int, int, double) {});
}

// What the phases of one workgroup's search share: its calibration's arrays, its own asset
// columns [j0, j1) and its place (workgroup w of G, launch-local cluster lc); built once at
// kernel entry.  (The counts nb / ne of the plain barriers / cluster reductions passed travel
// beside it: hk_solve_* takes their addresses, which would pin the whole struct in memory.)
struct GeCtx {
  double* tab;            // the calibration's kGeBufs table buffers
  double* X;              // mass
  double* PX;             // previous evaluation's mass
  int* LO;
  double* WL;
  unsigned* ctr;
  unsigned long long* cw;     // counting-barrier words
  unsigned long long* gran;
  const double* a_grid;
  double* aah;            // the calibration's Anderson ring: kGeAaHist slots of [S][n_a]
  unsigned* err;
  double beta, gam;
  size_t tab_sz;
  int j0, j1, w, G, S, n_a, cal, lc;
  int iid;                // i.i.d. income (every row of P the same bits) with AIY_OPT_HIST_IID on
  __device__ __forceinline__ double* tabm(int b) const { return tab + (size_t)b * 2 * tab_sz; }
  __device__ __forceinline__ double* tabc(int b) const { return tab + (size_t)b * 2 * tab_sz + tab_sz; }
};

__device__ __forceinline__ GeEvalOpts ge_eval_opts(const GeRun& g) {
  return {g.method, g.loose, g.logsec, g.warm_egm, g.warm_hist, g.secant, g.r_tol, g.egm_tol, g.hist_tol, g.loose_hist};
}

// plain cluster barrier after the workgroup's stores drained; false: timed out (the kernel returns)
__device__ __forceinline__ bool ge_barrier(const GeCtx& cx, unsigned& nb, unsigned* err) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ++nb;
  return hc_barrier(err, cx.ctr, (unsigned)cx.G * nb, &ge_s_flag);
}

// A vote of the cluster on its counting barrier: every workgroup's thread 0 adds `flag` (bit
// fields, each counted over the cluster) to the parity word of this barrier; dlt (thread 0) is
// what the cluster added.  Every workgroup sees the same dlt, so all take the same decision.
__device__ __forceinline__ bool ge_vote(const GeCtx& cx, unsigned* err, unsigned flag, unsigned& dlt) {
  GeState& st = ge_st;
  const int tid = threadIdx.x;
  if (tid == 0) ++st.nbc;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned k = st.nbc, par = k & 1u;
  if (!hc_barrier_count(err, &cx.cw[par], (unsigned)cx.G * ((k + par) / 2), flag, &ge_s_nc, &ge_s_flag))
    return false;
  if (tid == 0) {
    dlt = ge_s_nc - st.nc_prev[par];
    st.nc_prev[par] = ge_s_nc;
  }
  return true;
}

// Secant start of the household tables into `init` (own nodes): cur + theta (cur - prev).
template <int TH>
__device__ __forceinline__ void ge_secant_tables(const GeCtx& cx, int b_cur, int b_prev, int b_init, double theta) {
  const int tid = threadIdx.x, n1 = cx.n_a + 1;
  for (int s = 0; s < cx.S; ++s) {
    for (int k = cx.j0 + tid; k < cx.j1; k += TH) {
      const size_t o = (size_t)s * n1 + k + 1;
      const double cm = load_f64_agent(&cx.tabm(b_cur)[o]), pm = load_f64_agent(&cx.tabm(b_prev)[o]);
      const double cc = load_f64_agent(&cx.tabc(b_cur)[o]), pc = load_f64_agent(&cx.tabc(b_prev)[o]);
      store_f64_agent(&cx.tabm(b_init)[o], theta == 0.0 ? cm : cm + theta * (cm - pm));
      store_f64_agent(&cx.tabc(b_init)[o], theta == 0.0 ? cc : cc + theta * (cc - pc));
    }
    if (cx.j0 == 0 && tid == 0) {
      store_f64_agent(&cx.tabm(b_init)[(size_t)s * n1], kBorrowNode);
      store_f64_agent(&cx.tabc(b_init)[(size_t)s * n1], kBorrowNode);
    }
  }
}

// Geometric extrapolation at a check (ge_search.h egm_extrap_factor; egm.hip egm_extrap_kernel):
// the tables of cycle n (b_dst) move along their change from cycle n - 1 (b_src), own nodes.
template <int TH>
__device__ __forceinline__ bool ge_extrapolate(const GeCtx& cx, unsigned& nb, unsigned* err, int b_dst, int b_src,
                                               double dclu, int n) {
  GeState& st = ge_st;
  const int tid = threadIdx.x, n1 = cx.n_a + 1;
  if (tid == 0) {
    st.fext = egm_extrap_factor(dclu, st.dist, st.ev.etol, n, st.lam_prev);
    if (st.fext != 0.0) st.moved = 1;
  }
  __syncthreads();
  const double f = st.fext;
  if (f != 0.0) {
    double* cm = cx.tabm(b_dst);
    double* cc = cx.tabc(b_dst);
    const double* pm = cx.tabm(b_src);
    const double* pc = cx.tabc(b_src);
    for (int s = 0; s < cx.S; ++s)
      for (int k = cx.j0 + tid; k < cx.j1; k += TH) {
        const size_t o = (size_t)s * n1 + k + 1;
        const double x = load_f64_agent(&cm[o]), y = load_f64_agent(&cc[o]);
        store_f64_agent(&cm[o], x + f * (x - load_f64_agent(&pm[o])));
        store_f64_agent(&cc[o], y + f * (y - load_f64_agent(&pc[o])));
      }
    if (!ge_barrier(cx, nb, err)) return false;
  }
  return true;
}

// slot of cycle c's c table in the Anderson ring
__device__ __forceinline__ double* ge_ring(const GeCtx& cx, int c) {
  return cx.aah + (size_t)(c % kGeAaHist) * cx.S * cx.n_a;
}

// Type-II Anderson mix (ge_search.h aa_*) over the plain chain w0 .. w4 = the outputs of cycles
// n - 4 .. n (p >= kGeAaHist: no mix inside the window).  The Gram terms go through two cluster
// reductions in fixed order, so every workgroup solves the same 3 x 3 system to the same bits;
// x_{n+1} = w4 - dF gamma replaces the cycle's output (own nodes, m = a + c), visible to every
// workgroup after a barrier.
template <int TH>
__device__ __forceinline__ bool ge_anderson(const GeCtx& cx, unsigned& nb, unsigned& ne, int n, int b_dst) {
  static_assert(kGeAaM == 3 && kGeAaHist == 5, "the mixing is written for m = 3");
  const int tid = threadIdx.x, n1 = cx.n_a + 1;
  const double* W0 = ge_ring(cx, n - 4);
  const double* W1 = ge_ring(cx, n - 3);
  const double* W2 = ge_ring(cx, n - 2);
  const double* W3 = ge_ring(cx, n - 1);
  const double* W4 = ge_ring(cx, n);
  double gp[9];
  for (int q = 0; q < 9; ++q) gp[q] = 0.0;
  for (int s = 0; s < cx.S; ++s)
    for (int k = cx.j0 + tid; k < cx.j1; k += TH) {
      const size_t o = (size_t)s * cx.n_a + k;
      const double w0 = load_f64_agent(W0 + o), w1 = load_f64_agent(W1 + o), w2 = load_f64_agent(W2 + o);
      const double w3 = load_f64_agent(W3 + o), w4 = load_f64_agent(W4 + o);
      aa_gram_add(w0, w1, w2, w3, w4, gp);
    }
  double gs[9], gam[3];
  if (!ge_reduce<TH>(cx.gran, cx.G, cx.w, ne, gp, 6, 0u, ge_s_part, ge_s_res, &ge_s_flag, cx.err)) return false;
  for (int q = 0; q < 6; ++q) gs[q] = ge_s_res[q];
  if (!ge_reduce<TH>(cx.gran, cx.G, cx.w, ne, gp + 6, 3, 0u, ge_s_part, ge_s_res, &ge_s_flag, cx.err)) return false;
  for (int q = 0; q < 3; ++q) gs[6 + q] = ge_s_res[q];
  if (aa_solve(gs, gam)) {
    double* dm = cx.tabm(b_dst);
    double* dc = cx.tabc(b_dst);
    for (int s = 0; s < cx.S; ++s)
      for (int k = cx.j0 + tid; k < cx.j1; k += TH) {
        const size_t o = (size_t)s * cx.n_a + k;
        const double w1 = load_f64_agent(W1 + o), w2 = load_f64_agent(W2 + o);
        const double w3 = load_f64_agent(W3 + o), w4 = load_f64_agent(W4 + o);
        const double cn = aa_mix(gam, w1, w2, w3, w4);
        store_f64_agent(&dm[(size_t)s * n1 + k + 1], cx.a_grid[k] + cn);   // AS:1499
        store_f64_agent(&dc[(size_t)s * n1 + k + 1], cn);
      }
    if (tid == 0) ge_st.moved = 1;
    if (!ge_barrier(cx, nb, cx.err)) return false;
  }
  return true;
}

// the launch's settings the household solve reads (GeRun's)
struct GeHhOpt {
  int max_cyc, aa_period, extrap_period;
};

// Cycle n's output goes into the Anderson ring only where a mix will read it: the next mix is at
// the first multiple N >= n of the period p and reads cycles N - kGeAaHist + 1 .. N, and it runs
// only under ge_anderson's entry condition (ge_household_solve below: N >= p, which every such
// N meets, and N >= kGeAaHist + 1).  At p = 12 that is 5 cycles of 12; a period below kGeAaHist
// keeps every cycle.
__device__ __forceinline__ bool ge_ring_wanted(int n, int p) {
  const int ph = n % p;
  const int mix = ph == 0 ? n : n + (p - ph);
  return (ph == 0 || ph > p - kGeAaHist) && mix >= kGeAaHist + 1;
}

// The household solve ([HARK] solve_agent: cycles until the sup-norm change of the tables is
// <= tol, NaN stops; cold -- init_m == nullptr -- cycle 1 from the terminal guess).  Returns
// the buffer of the final tables, -1: a barrier timed out.
template <int SMAX, int SC, int PK, int TH>
__device__ __forceinline__ int ge_household_solve(const GeCtx& cx, unsigned& nb, unsigned& ne, const GeHhOpt& g,
                                                  double R, const double* init_m, const double* init_c, double* dyn) {
  constexpr int NW = TH / kWave;
  GeState& st = ge_st;
  const int tid = threadIdx.x;
  int final_buf = -1;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (!ge_barrier(cx, nb, cx.err)) return -1;   // every workgroup's start tables visible
    // Anderson mixing (the first attempt; a NaN after a mix reruns the solve plain) replaces
    // the geometric extrapolation
    const bool aa = g.aa_period > 0 && attempt == 0;
    const bool ext = st.extrap != 0 && attempt == 0 && !aa;
    if (tid == 0) {
      st.lam_prev = -1.0;
      st.moved = 0;
      st.nan_stop = 0;
    }
    int n = 1;
    const int last_allowed = g.max_cyc + 1;
    bool converged = false;
    while (true) {
      const int b_dst = st.buf[n & 1], b_src = st.buf[(n - 1) & 1];
      const double* sm = n == 1 ? init_m : cx.tabm(b_src);
      const double* sc = n == 1 ? init_c : cx.tabc(b_src);
      const bool track = n >= 2;
      double* ring = aa && ge_ring_wanted(n, g.aa_period) ? ge_ring(cx, n) : nullptr;
      const double dl = ge_egm_cycle_fn<SMAX, SC, PK, NW>(cx.S, cx.n_a, cx.j0, cx.j1, cx.a_grid, sm, sc, cx.tabm(b_dst),
                                                          cx.tabc(b_dst), track, R, cx.beta, cx.gam, dyn, ring, cx.iid != 0);
      // cluster distance: the value itself at the extrapolation checks (cycles 32k - 1,
      // 32k), else only its two facts (some part > tol; some part NaN) on a counting barrier
      const int xp = g.extrap_period;
      const bool want_value = ext && n >= xp - 1 && ((n % xp) == xp - 1 || (n % xp) == 0);
      double dclu = 0.0;
      bool go;
      if (want_value) {
        double v[1] = {dl};
        if (!ge_reduce<TH>(cx.gran, cx.G, cx.w, ne, v, 1, 1u, ge_s_part, ge_s_res, &ge_s_flag, cx.err)) return -1;
        dclu = ge_s_res[0];
        go = dclu > st.ev.etol;   // NaN: stop (HARK: go = distance > tolerance)
        if (tid == 0) st.nan_stop = dclu != dclu;
      } else {
        const double dw = wave_nan_max(dl);
        if ((tid & (kWave - 1)) == 0) ge_s_part[0][tid / kWave] = dw;
        __syncthreads();
        unsigned flag = 0u, dlt = 0u;
        if (tid == 0) {
          double d = ge_s_part[0][0];
          for (int q = 1; q < TH / kWave; ++q) d = nan_max(d, ge_s_part[0][q]);
          flag = (d > st.ev.etol ? 1u : 0u) | (d != d ? (1u << 16) : 0u);
        }
        if (!ge_vote(cx, cx.err, flag, dlt)) return -1;
        if (tid == 0) {
          st.stop = (dlt & 0xffffu) == 0u || (dlt >> 16) != 0u;
          st.nan_stop = (dlt >> 16) != 0u;
        }
        __syncthreads();
        go = !st.stop;
      }
      if (track && !go) {
        converged = true;
        break;
      }
      if (n >= last_allowed) break;
      if (want_value && (n % xp) == 0) {
        if (!ge_extrapolate<TH>(cx, nb, cx.err, b_dst, b_src, dclu, n)) return -1;
      } else if (want_value) {
        if (tid == 0) st.dist = dclu;
      }
      if (aa && n >= g.aa_period && n >= kGeAaHist + 1 && (n % g.aa_period) == 0) {
        if (!ge_anderson<TH>(cx, nb, ne, n, b_dst)) return -1;
      }
      ++n;
    }
    if (tid == 0) {
      st.n = n;
      if (!converged) st.status |= 1;
    }
    __syncthreads();
    final_buf = st.buf[n & 1];
    // an extrapolated solve that ended in NaN: the whole solve again, plain (ge.hip)
    if (!(st.moved && st.nan_stop)) break;
    if (tid == 0) {
      st.extrap = 0;
      st.status &= ~1;
    }
    __syncthreads();
  }
  return final_buf;
}

// ge_household_solve as its own (not inlined) function, one per CRRA kind: inlined, the four
// kinds' cycles, the lottery, the mixing and the search loop's live state shared one register
// allocation, and its spills sat in the cycle's tile loop.  The boundary is
// hk_solve_isolated's (hist_bicg.h, §4j): the arguments arrive in VGPRs and are read into SGPRs
// once at entry, the pointers typed global; the dynamic LDS comes by its 32-bit address, so its
// accesses stay ds_ instructions; the barrier / reduction counts go in and out by pointer.  The
// function does not depend on the columns per thread: the kernels of one state count share it.
struct GeHhArgs {
  gptr<double> tab, aah;
  gptr<unsigned> ctr, err;
  gptr<unsigned long long> gran;
  gptr<const double> a_grid, init_m, init_c;
  double beta, gam, R;
  int j0, j1, w, G, S, n_a, iid;
  GeHhOpt opt;
  unsigned dyn_lds;   // hk_lds_addr(ge_dyn)
};
template <int SMAX, int SC, int PK, int TH>
__device__ __noinline__ int ge_household_isolated(GeHhArgs a, unsigned* nb_io, unsigned* ne_io) {
  double* dyn = (double*)(lptr<double>)(size_t)(unsigned)hk_uni((int)a.dyn_lds);
  GeCtx cx;
  cx.tab = (double*)hk_uni(a.tab);
  cx.aah = (double*)hk_uni(a.aah);
  cx.ctr = (unsigned*)hk_uni(a.ctr);
  cx.cw = reinterpret_cast<unsigned long long*>(cx.ctr + 2);
  cx.err = (unsigned*)hk_uni(a.err);
  cx.gran = (unsigned long long*)hk_uni(a.gran);
  cx.a_grid = (const double*)hk_uni(a.a_grid);
  cx.X = cx.PX = cx.WL = nullptr;   // (the distribution's arrays: not the household solve's)
  cx.LO = nullptr;
  cx.beta = hk_uni(a.beta); cx.gam = hk_uni(a.gam);
  cx.j0 = hk_uni(a.j0); cx.j1 = hk_uni(a.j1); cx.w = hk_uni(a.w); cx.G = hk_uni(a.G);
  cx.S = SC > 0 ? SC : hk_uni(a.S);
  cx.n_a = hk_uni(a.n_a);
  cx.cal = cx.lc = 0;
  cx.iid = hk_uni(a.iid);
  cx.tab_sz = (size_t)cx.S * (cx.n_a + 1);
  const GeHhOpt opt = {hk_uni(a.opt.max_cyc), hk_uni(a.opt.aa_period), hk_uni(a.opt.extrap_period)};
  unsigned nb = *nb_io, ne = *ne_io;
  const int fb = ge_household_solve<SMAX, SC, PK, TH>(cx, nb, ne, opt, hk_uni(a.R), (const double*)hk_uni(a.init_m),
                                                     (const double*)hk_uni(a.init_c), dyn);
  *nb_io = nb;
  *ne_io = ne;
  return fb;
}

// The distribution's start (own columns): uniform, or the last mass -- with a secant start its
// secant extrapolation from the last two -- the last one kept as the previous mass.
template <int TH>
__device__ __forceinline__ void ge_mass_start(const GeCtx& cx, bool fresh, bool warm, bool secant, double theta) {
  const int tid = threadIdx.x;
  if (fresh) {
    const double u0 = 1.0 / ((double)cx.S * cx.n_a);
    for (int s = 0; s < cx.S; ++s)
      for (int k = cx.j0 + tid; k < cx.j1; k += TH) cx.X[(size_t)s * cx.n_a + k] = u0;
  } else if (warm) {
    for (int s = 0; s < cx.S; ++s)
      for (int k = cx.j0 + tid; k < cx.j1; k += TH) {
        const size_t o = (size_t)s * cx.n_a + k;
        const double x = cx.X[o];
        if (secant) cx.X[o] = theta == 0.0 ? x : x + theta * (x - cx.PX[o]);
        cx.PX[o] = x;
      }
  }
}

// K_s = sum mass a over the cluster, into ge_s_res[0] of every workgroup
template <int TH>
__device__ __forceinline__ bool ge_capital(const GeCtx& cx, unsigned& ne, unsigned* err) {
  double part = 0.0;
  for (int k = cx.j0 + (int)threadIdx.x; k < cx.j1; k += TH) {
    double ms = 0.0;
    for (int s = 0; s < cx.S; ++s) ms += cx.X[(size_t)s * cx.n_a + k];
    part += ms * cx.a_grid[k];
  }
  double v[1] = {part};
  return ge_reduce<TH>(cx.gran, cx.G, cx.w, ne, v, 1, 0u, ge_s_part, ge_s_res, &ge_s_flag, err);
}

// a finished search's outputs and profile (workgroup 0, thread 0)
__device__ __forceinline__ void ge_write_out(const GeCtx& cx, const GeRun& g, const GeCalDev& cd) {
  const GeState& st = ge_st;
  const int cal = cx.cal;
  __hip_atomic_fetch_add(to_global(g.done_ctr), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  g.out_done[cal] = 1;
  g.out_r[cal] = st.ev.rs.x;
  g.out_K[cal] = ge_prices(st.ev.rs.x, cd.alpha, cd.delta).Kd;
  g.out_Ks[cal] = st.Ks;
  g.out_steps[cal] = st.ev.steps;
  g.out_cyc[cal] = (int)min(st.cyc_sum, 0x7fffffffll);
  g.out_its[cal] = (int)min(st.its_sum, 0x7fffffffll);
  g.out_status[cal] = st.status | (st.ev.rs.done ? 0 : 4);
  double* pf = g.out_prof + (size_t)cal * kGeProf;
  pf[0] = st.t_egm * 0.01;
  pf[1] = st.t_lot * 0.01;
  pf[2] = st.t_hist * 0.01;
  pf[3] = st.t_k * 0.01;
  pf[4] = (__builtin_amdgcn_s_memrealtime() - st.t0) * 0.01;
  pf[5] = (double)st.cyc_sum;
  pf[6] = (double)st.its_sum;
  pf[7] = (double)st.ev.steps;
}

// setup -> while the search is not over { stop vote; plan; household solve; lottery; mass
// start; distribution solve; K_s; accept } -> save the stopped search, or write it out
// PULL: the launch's distribution solves by the lottery pull (AIY_OPT_HIST_PULL, the same for every
// cluster of a launch): each kernel carries one form of the solve.
template <int SMAX, int SC, int KC, int TH, bool PULL>
__global__ __launch_bounds__(TH) void ge_cluster_kernel(GeRun g) {
  constexpr int NW = TH / kWave;
  static_assert(SMAX <= kGeSmax, "file-scope LDS sized for kGeSmax states");
  GeState& st = ge_st;

  const int per = gridDim.x >> 3;
  const int u = (blockIdx.x & 7) * per + (blockIdx.x >> 3);   // XCD-contiguous work order
  if (u >= g.n_work) return;
  const int G = g.G, S = g.S, n_a = g.n_a;
  const int tid = threadIdx.x;
  GeCtx cx;
  cx.G = G; cx.S = S; cx.n_a = n_a;
  cx.lc = u / G; cx.w = u - cx.lc * G;   // launch-local cluster, workgroup in it
  const int lc = cx.lc, w = cx.w, cal = g.cal_ids[lc];
  cx.cal = cal;
  cx.j0 = w * g.nj; cx.j1 = min(cx.j0 + g.nj, n_a);
  const int j0 = cx.j0, j1 = cx.j1;
  cx.a_grid = g.a_grid + (size_t)cal * n_a;
  cx.beta = g.beta[cal]; cx.gam = g.crra[cal];
  const GeCalDev cd = g.cal[cal];
  cx.tab_sz = (size_t)S * (n_a + 1);
  cx.tab = g.tab + (size_t)cal * kGeBufs * 2 * cx.tab_sz;
  const size_t row0 = (size_t)cal * S * n_a;
  cx.X = g.mass + row0;
  cx.PX = g.pmass + row0;
  cx.LO = g.lo + row0;
  cx.WL = g.wlo + row0;
  cx.ctr = g.ctr + (size_t)lc * kHcCtrStride;
  cx.cw = reinterpret_cast<unsigned long long*>(cx.ctr + 2);
  cx.gran = g.gran + (size_t)lc * 2 * G * kHcRedRec;
  cx.aah = g.aah + (size_t)cal * kGeAaHist * S * n_a;
  cx.err = g.err;
  unsigned nb = 0, ne = 0;   // plain barriers / reductions passed (hk_solve counts on)
  const int pk = crra_kind(cx.gam);

  for (int q = tid; q < S * S; q += TH) ge_s_Pe[q] = g.P[(size_t)cal * S * S + q];
  for (int q = tid; q < kGeMaxTiles * SMAX; q += TH) ge_s_hint[q] = -1;
  if (tid == 0) {
    if (g.resume[cal]) {   // a calibration stopped by an earlier launch: its search goes on
      st = g.saved[cal];
      st.t0 = __builtin_amdgcn_s_memrealtime() - st.t0;   // saved: the time spent so far
    } else {
      st.ev.init(ge_eval_opts(g), cd.r_lo, cd.r_hi);
      st.Ks = 0.0;
      st.in_hist = 0;
      st.status = 0;
      st.cyc_sum = st.its_sum = 0;
      for (int b = 0; b < kGeBufs; ++b) st.buf[b] = b;
      st.t_egm = st.t_lot = st.t_hist = st.t_k = 0ull;
      st.t0 = __builtin_amdgcn_s_memrealtime();
    }
    st.opt = ge_eval_opts(g);
    st.nc_prev[0] = st.nc_prev[1] = 0u;   // this launch's counting-barrier words start at 0
    st.nbc = 0u;
  }
  __syncthreads();
  // i.i.d. income: S >= 2 and every row of P equal to row 0 bit for bit, compared as integers (one
  // differing bit: the general path).  Every workgroup of the cluster reads the same bits of P, so
  // the flag is cluster-uniform: all of them take the same barriers and reductions below.
  {
    int iid = g.iid_on != 0 && S >= 2;
    for (int q = S; q < S * S; ++q)
      iid &= __double_as_longlong(ge_s_Pe[q]) == __double_as_longlong(ge_s_Pe[q % S]);
    cx.iid = __builtin_amdgcn_readfirstlane(iid);
  }
  if (w == 0 && tid == 0) g.out_iid[cal] = (!PULL && cx.iid) ? 1 : 0;

  bool stopped = false;
  while ((!st.ev.rs.done && st.ev.steps < g.max_steps) || st.ev.final_ks) {
    // ---- rebalancing stop: once stop_at calibrations of the launch have finished, the
    //      cluster leaves at this evaluation boundary (the decision: any workgroup saw it,
    //      counted on the cluster's barrier, so every workgroup takes it) ----
    if (g.stop_at > 0 && st.ev.steps > 0 && !st.in_hist) {
      unsigned flag = 0u, dlt = 0u;
      if (tid == 0)
        flag = __hip_atomic_load(to_global(g.done_ctr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >=
                       (unsigned)g.stop_at ? 1u : 0u;
      if (!ge_vote(cx, g.err, flag, dlt)) return;
      if (tid == 0) st.stop = dlt != 0u;
      __syncthreads();
      if (st.stop) {
        stopped = true;
        break;
      }
    }
    // a calibration stopped inside its distribution solve resumes there (prices, tables,
    // lottery and the iterate are in the saved state and HBM)
    unsigned long long tp = __builtin_amdgcn_s_memrealtime();
    if (tid == 0 && !st.in_hist) st.t_ev0 = tp;
    if (!st.in_hist) {
      // ---- this evaluation's prices, tolerances and starts (thread 0; identical everywhere) ----
      if (tid == 0) {
        st.ev.plan(st.opt, cd.alpha, cd.delta);
        st.extrap = g.extrap;
        st.moved = 0;
      }
      __syncthreads();
      if (tid < S) ge_s_Wl[tid] = st.ev.wage * g.lab[(size_t)cal * S + tid];   // W l(s') (mNextArray, AS:1024)
      const double R = st.ev.R, theta = st.ev.theta;
      // ---- starting tables: the secant start into `init` (own nodes), else cur ----
      const bool secant = st.ev.secant != 0, warm = st.ev.warm_egm != 0;
      const int b_cur = st.buf[2], b_prev = st.buf[3], b_init = st.buf[4];
      if (secant) ge_secant_tables<TH>(cx, b_cur, b_prev, b_init, theta);
      // ---- the household solve ----
      tp = __builtin_amdgcn_s_memrealtime();
      GeHhArgs ha;
      ha.tab = to_global(cx.tab); ha.aah = to_global(cx.aah); ha.ctr = to_global(cx.ctr); ha.err = to_global(g.err);
      ha.gran = to_global(cx.gran); ha.a_grid = to_global(cx.a_grid);
      ha.init_m = to_global((const double*)(secant ? cx.tabm(b_init) : (warm ? cx.tabm(b_cur) : nullptr)));
      ha.init_c = to_global((const double*)(secant ? cx.tabc(b_init) : (warm ? cx.tabc(b_cur) : nullptr)));
      ha.beta = cx.beta; ha.gam = cx.gam; ha.R = R;
      ha.j0 = j0; ha.j1 = j1; ha.w = w; ha.G = G; ha.S = S; ha.n_a = n_a; ha.iid = cx.iid;
      ha.opt = {g.max_cyc, g.aa_period, g.extrap_period};
      ha.dyn_lds = hk_lds_addr(ge_dyn);
      // one instantiation per CRRA kind (1, 3, 5, else the general pow), each with one copy of the cycle
      const int final_buf = pk == 1   ? ge_household_isolated<SMAX, SC, 1, TH>(ha, &nb, &ne)
                            : pk == 3 ? ge_household_isolated<SMAX, SC, 3, TH>(ha, &nb, &ne)
                            : pk == 5 ? ge_household_isolated<SMAX, SC, 5, TH>(ha, &nb, &ne)
                                      : ge_household_isolated<SMAX, SC, 0, TH>(ha, &nb, &ne);
      if (final_buf < 0) return;
      if (tid == 0) {
        const unsigned long long tn = __builtin_amdgcn_s_memrealtime();
        st.t_egm += tn - tp;
        st.cyc_sum += st.n;
        // buffer roles: prev <- cur, cur <- the solve's final tables, the freed ones ping-pong
        const int fb = final_buf;
        const int other = st.buf[0] == fb ? st.buf[1] : st.buf[0];
        const int old_prev = st.buf[3];
        st.buf[3] = st.buf[2];
        st.buf[2] = fb;
        st.buf[0] = other;
        st.buf[1] = old_prev;
      }
      __syncthreads();
      // ---- lottery of the own columns on the final tables (hist.hip hist_lottery_kernel) ----
      tp = __builtin_amdgcn_s_memrealtime();
      ge_lottery_fn<SMAX, NW>(S, n_a, j0, j1, cx.a_grid, cx.tabm(st.buf[2]), cx.tabc(st.buf[2]), R, st.ev.steps > 0,
                              cx.LO, cx.WL, PULL);
      ge_mass_start<TH>(cx, st.ev.fresh_mass != 0, warm, secant, theta);
      __syncthreads();
      if (tid == 0) {
        const unsigned long long tn = __builtin_amdgcn_s_memrealtime();
        st.t_lot += tn - tp;
        tp = tn;
      }
    }
    // ---- the stationary distribution: BiCGSTAB on (I - T) mass = 0 ----
    int mv;
    {
      HkArgs hk;
      hk.G = G; hk.S = S; hk.n_a = n_a; hk.cap = g.cap; hk.w = w; hk.j0 = j0; hk.j1 = j1;
      hk.LO = to_global((const int*)cx.LO); hk.WL = to_global((const double*)cx.WL); hk.X = to_global(cx.X);
      hk.Pg = to_global(g.pg + row0); hk.Vg = to_global((double*)nullptr);
      hk.slab_cl = to_global(g.slab + (size_t)lc * G * 2 * g.cap);
      hk.span_cl = to_global(g.span + (size_t)lc * G * SMAX * 4);
      hk.ctr = to_global(cx.ctr); hk.gran = to_global(cx.gran); hk.Pc = to_global(g.P + (size_t)cal * S * S);
      hk.max_iter = g.max_hist; hk.err = to_global(g.err);
      hk.tol = st.ev.htol;
      hk.stop_ctr = to_global((const unsigned*)(g.stop_at > 0 ? g.done_ctr : nullptr));
      hk.stop_at = (unsigned)g.stop_at;
      hk.Qg = to_global(g.qb + row0);
      hk.Ainv = to_global(g.ainv + (size_t)cal * S * (n_a + 1));
      hk.lottery_fresh = true;
      hk.dyn_lds = hk_lds_addr(ge_dyn);
      if constexpr (PULL) mv = hk_solve_inlined<SMAX, KC, TH, true, false, SC>(hk, &nb, &ne);
      else if (cx.iid)   // (cluster-uniform) the asset-grid solve, a function of its own
        mv = hk_solve_isolated<SMAX, KC, TH, false, (KC == 1 || kGeIidFuseAKc2) && kGeFuseA, SC, true>(hk, &nb, &ne);
      else mv = hk_solve_isolated<SMAX, KC, TH, false, (KC == 1 || kGeFuseAKc2) && kGeFuseA, SC>(hk, &nb, &ne);
    }
    if (mv == -1) return;
    if (tid == 0) {
      const unsigned long long tn = __builtin_amdgcn_s_memrealtime();
      st.t_hist += tn - tp;
      tp = tn;
    }
    if (mv <= -2) {   // rebalancing stop inside the solve: resume it in the next launch
      if (tid == 0) {
        st.its_sum += -mv - 2;
        st.in_hist = 1;
        if (w == 0) __hip_atomic_fetch_add(to_global(g.done_ctr + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      stopped = true;
      break;
    }
    if (tid == 0) st.in_hist = 0;
    if (!ge_capital<TH>(cx, ne, g.err)) return;
    const bool fin = st.ev.final_ks != 0;   // (set in an earlier pass; never cleared: the loop ends here)
    if (tid == 0) {
      const double Ks = ge_s_res[0];
      if (w == 0 && st.ev.steps < kGeEvLog && !fin) {
        double* ev = g.out_evlog + ((size_t)cal * kGeEvLog + st.ev.steps) * kGeEvRec;
        ev[0] = st.ev.rs.x;
        ev[1] = (Ks - st.ev.Kd) / st.ev.Kd;
        ev[2] = (double)st.n;
        ev[3] = (double)mv;
        ev[4] = (double)st.ev.loose;
        ev[5] = (double)(__builtin_amdgcn_s_memrealtime() - st.t_ev0) * 0.01;
      }
      st.its_sum += mv;
      if (mv >= g.max_hist) st.status |= 2;
    }
    if (fin) {   // the full-tolerance re-solve of the last evaluation: K_s only
      if (tid == 0) st.Ks = ge_s_res[0];
      __syncthreads();
      break;
    }
    if (tid == 0) {
      st.ev.accept(ge_s_res[0]);
      st.Ks = ge_s_res[0];
      st.t_k += __builtin_amdgcn_s_memrealtime() - tp;
    }
    __syncthreads();
  }
  if (stopped) {
    if (w == 0 && tid == 0) {
      st.t0 = __builtin_amdgcn_s_memrealtime() - st.t0;
      g.saved[cal] = st;
      g.out_done[cal] = 0;
    }
    return;
  }
  if (w == 0 && tid == 0) ge_write_out(cx, g, cd);
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
struct GePlan {
  int G = 0, nj = 0, kc = 0, smax = 0, sc = 0, cap = 0, blocks = 0, th = 0;
  size_t lds = 0;
  const void* fn = nullptr;
};

template <int SMAX, int SC, int KC, int TH>
static const void* ge_fn(bool pull) {
  return pull ? reinterpret_cast<const void*>(ge_cluster_kernel<SMAX, SC, KC, TH, true>)
              : reinterpret_cast<const void*>(ge_cluster_kernel<SMAX, SC, KC, TH, false>);
}

// Launch shape of the device-resident search for (n_cal, S, n_a): every calibration's
// cluster resident at once (n_cal G workgroups, one per CU, within the handle's CU limit).
static bool ge_make_plan(aiy_handle* h, int n_cal, int S, int n_a, GePlan& p) {
  if (S < 1 || S > kGeSmax || n_a < 2 || n_cal < 1) return false;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 1) return false;
  if (h->cu_limit > 0) cus = std::min(cus, h->cu_limit);
  // the cluster reductions' sweep (hc_sweep, hist_cluster.h) reads at most kHcMaxG workgroups
  const int g_cap = h->hist_cluster_cap > 0 ? h->hist_cluster_cap : 32;
  if (!hc_cluster_split(n_a, (n_a + 2 * 512 - 1) / (2 * 512), g_cap, cus, n_cal, &p.G, &p.nj)) return false;
  if (p.G > kHcMaxG) return false;
  if (p.nj > kGeMaxTiles * kTile) return false;
  if ((long long)p.G * n_cal > cus) return false;
  p.th = 512;
  const int th = p.th;
  p.kc = p.nj <= th ? 1 : 2;
  p.smax = S == 7 ? 7 : 8;   // the Table II shape: exact state count (fewer registers in the solve)
  p.sc = S == 7 ? 7 : 0;
  const bool pull = h->hist_pull != 0;   // AIY_OPT_HIST_PULL: deterministic distribution solves
  if (p.sc == 7) p.fn = p.kc == 1 ? ge_fn<7, 7, 1, 512>(pull) : ge_fn<7, 7, 2, 512>(pull);
  else p.fn = p.kc == 1 ? ge_fn<8, 0, 1, 512>(pull) : ge_fn<8, 0, 2, 512>(pull);
  HcLds lds;
  if (!hc_lds_budget(h->device, p.fn, lds)) return false;
  p.lds = lds.dyn;
  const size_t vbytes = (size_t)p.kc * p.smax * th * sizeof(double);   // BiCGSTAB v behind the spans
  const size_t egm_lds = ge_egm_lds<8>();
  if (p.lds < egm_lds || p.lds <= vbytes + 4096) return false;
  p.cap = (int)((p.lds - vbytes) / sizeof(double));
  p.blocks = (p.G * n_cal + 7) / 8 * 8;
  return true;
}

// Per-calibration arrays (kept across the rebalancing launches) first, then the per-launch
// cluster arrays sized for the most workgroups any launch can hold (cus) and the largest span
// capacity (cap_max doubles).
struct GeScratch {
  double *tab, *mass, *pmass, *pg, *qb, *wlo, *slab, *outd, *prof, *evlog, *aah;
  int *ainv, *lo, *span, *ids, *resume, *done, *outi, *iid;
  unsigned *ctr, *err;
  unsigned long long* gran;
  GeState* saved;
  GeCalDev* cal;
  size_t bytes;
};
static GeScratch ge_scratch(Carve c, int n_cal, int S, int n_a, int cus, int cap_max) {
  GeScratch L;
  const size_t pts = (size_t)n_cal * S * n_a;
  L.tab = c.take<double>((size_t)n_cal * kGeBufs * 2 * S * (n_a + 1));
  L.mass = c.take<double>(pts); L.pmass = c.take<double>(pts); L.pg = c.take<double>(pts); L.qb = c.take<double>(pts);
  L.ainv = c.take<int>((size_t)n_cal * S * (n_a + 1));
  L.lo = c.take<int>(pts); L.wlo = c.take<double>(pts);
  L.slab = c.take<double>((size_t)cus * 2 * cap_max);
  L.span = c.take<int>((size_t)cus * 8 * 4);
  L.ctr = c.take<unsigned>((size_t)n_cal * kHcCtrStride);
  L.gran = c.take<unsigned long long>((size_t)cus * 2 * kHcRedRec);
  L.ids = c.take<int>(n_cal);
  L.saved = c.take<GeState>(n_cal);
  L.resume = c.take<int>(n_cal);
  L.done = c.take<int>(n_cal);
  L.err = c.take<unsigned>(256 / sizeof(unsigned));
  L.cal = c.take<GeCalDev>(n_cal);
  L.outd = c.take<double>((size_t)n_cal * 3);
  L.outi = c.take<int>((size_t)n_cal * 4);
  L.prof = c.take<double>((size_t)n_cal * kGeProf);
  L.evlog = c.take<double>((size_t)n_cal * kGeEvLog * kGeEvRec);
  L.aah = c.take<double>((size_t)n_cal * kGeAaHist * S * n_a);
  L.iid = c.take<int>(n_cal);
  L.bytes = c.bytes();
  return L;
}

// The whole search on device when the shape allows it (1: done; 0: not applicable, the caller
// runs the host-driven loop; < 0: error).  With rebalancing (AIY_OPT_GE_REBALANCE = q > 0,
// default 55) a launch whose calibrations are more than 4 stops every cluster at its next
// evaluation boundary once q % of them have finished, and the unfinished ones are launched
// again with the freed compute units (a cluster's time scales with its columns per CU): with
// q = 50 the 24 Table II cells run as 24 x 10, then ~12 x 21, ~6 x 32, ~3 x 32 workgroups.
int32_t ge_stationary_resident(aiy_handle* h, const aiy_stationary_model* M, const aiy_ge_options* o, double* r_out,
                               double* K_out, double* Ks_out, int32_t* steps_out, int32_t* cyc_out,
                               int32_t* its_out, int32_t* status_out, hipStream_t st) {
  h->ge_iid_cells = 0;   // (also when the host-driven loop runs instead: it has no reduced solve)
  if (!h->ge_resident || o->accel >= 0) return 0;   // BiCGSTAB distribution solves only
  const int n_cal = M->n_cal, S = M->S, n_a = M->n_a;
  GePlan p0;
  if (!ge_make_plan(h, n_cal, S, n_a, p0)) return 0;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) return 0;
  if (h->cu_limit > 0) cus = std::min(cus, h->cu_limit);
  const int cap_max = (int)(kHcLdsTotal / sizeof(double));
  const int32_t rsv = h->ge.reserve(h, ge_scratch(Carve(), n_cal, S, n_a, cus, cap_max).bytes);
  if (rsv) return rsv;
  const GeScratch L = ge_scratch(Carve(h->ge.get()), n_cal, S, n_a, cus, cap_max);
  std::vector<GeCalDev> cals(n_cal);
  for (int c = 0; c < n_cal; ++c) {
    cals[c].alpha = M->alpha[c];
    cals[c].delta = M->delta[c];
    cals[c].disc = M->disc[c];
    cals[c].r_lo = o->r_lo ? o->r_lo[c] : GeEval::default_lo(M->delta[c]);
    cals[c].r_hi = o->r_hi ? o->r_hi[c] : GeEval::default_hi(M->disc[c]);
  }
  GeRun g;
  g.n_cal = n_cal; g.S = S; g.n_a = n_a;
  g.a_grid = M->a_grid; g.P = M->P; g.lab = M->lab; g.beta = M->beta; g.crra = M->crra;
  g.cal = L.cal;
  g.method = o->method; g.r_tol = o->r_tol; g.egm_tol = o->egm_tol; g.hist_tol = o->hist_tol;
  g.max_steps = o->max_steps;
  g.max_cyc = o->max_egm_cycles > 0 ? o->max_egm_cycles : 5000;
  g.max_hist = o->max_hist_iter > 0 ? o->max_hist_iter : 200000;
  g.warm_hist = o->warm_hist != 0; g.warm_egm = o->warm_egm != 0;
  g.secant = o->secant_start != 0; g.loose = o->loose_bracket != 0; g.extrap = o->egm_extrapolate != 0;
  g.extrap_period = h->ge_extrap_period;
  g.aa_period = o->egm_extrapolate != 0 ? h->ge_anderson : 0;   // (with the EGM acceleration on)
  g.aah = L.aah;
  g.iid_on = h->hist_iid; g.out_iid = L.iid;
  g.logsec = h->ge_logsec;
  g.tab = L.tab; g.mass = L.mass; g.pmass = L.pmass; g.pg = L.pg; g.qb = L.qb; g.ainv = L.ainv;
  g.loose_hist = std::pow(10.0, -(double)h->ge_loose_hist);
  g.lo = L.lo; g.wlo = L.wlo; g.slab = L.slab; g.span = L.span; g.ctr = L.ctr; g.gran = L.gran;
  int *d_ids = L.ids, *d_resume = L.resume, *outi = L.outi;
  g.cal_ids = d_ids; g.saved = L.saved; g.resume = d_resume; g.out_done = L.done;
  g.err = L.err;
  g.done_ctr = g.err + 1;
  double* outd = L.outd;
  g.out_r = outd; g.out_K = outd + n_cal; g.out_Ks = outd + 2 * n_cal;
  g.out_steps = outi; g.out_cyc = outi + n_cal; g.out_its = outi + 2 * n_cal; g.out_status = outi + 3 * n_cal;
  g.out_prof = L.prof; g.out_evlog = L.evlog;
  AIY_HIP(h, hipMemsetAsync(g.out_evlog, 0, (size_t)n_cal * kGeEvLog * kGeEvRec * sizeof(double), st));
  AIY_HIP(h, hipMemcpyAsync(L.cal, cals.data(), sizeof(GeCalDev) * n_cal, hipMemcpyHostToDevice, st));
  AIY_HIP(h, hipMemsetAsync(d_resume, 0, (size_t)n_cal * sizeof(int), st));
  AIY_HIP(h, hipMemsetAsync(g.out_done, 0, (size_t)n_cal * sizeof(int), st));
  AIY_HIP(h, h->ge_timer.ensure());
  std::vector<int> active(n_cal), done(n_cal, 0), resume(n_cal, 0);
  for (int c = 0; c < n_cal; ++c) active[c] = c;
  h->ge_rounds = 0;
  h->ge_mid_stops = 0;
  while (!active.empty()) {
    const int n = (int)active.size();
    GePlan p;
    if (!ge_make_plan(h, n, S, n_a, p)) return fail(h, AIY_ERR_STATE, "device-resident GE: no plan for %d calibrations", n);
    const Admit adm = admit_launch(p.fn, p.th, p.lds, true);
    if (adm != Admit::fits) {
      if (h->ge_rounds == 0) return 0;
      return fail(h, AIY_ERR_STATE, adm == Admit::attr_error ? "device-resident GE: dynamic LDS attribute"
                                                             : "device-resident GE: occupancy query");
    }
    g.G = p.G; g.nj = p.nj; g.cap = p.cap; g.n_work = n * p.G;
    g.stop_at = (h->ge_rebalance > 0 && n > 4) ? std::max(1, (n * h->ge_rebalance + 99) / 100) : 0;
    std::vector<int> res_h(n_cal);
    for (int c = 0; c < n_cal; ++c) res_h[c] = resume[c];
    AIY_HIP(h, hipMemcpyAsync(d_ids, active.data(), sizeof(int) * n, hipMemcpyHostToDevice, st));
    AIY_HIP(h, hipMemcpyAsync(d_resume, res_h.data(), sizeof(int) * n_cal, hipMemcpyHostToDevice, st));
    AIY_HIP(h, hipMemsetAsync(g.ctr, 0, (size_t)n * kHcCtrStride * sizeof(unsigned), st));
    AIY_HIP(h, hipMemsetAsync(g.gran, 0, (size_t)n * 2 * p.G * kHcRedRec * sizeof(unsigned long long), st));
    AIY_HIP(h, hipMemsetAsync(g.err, 0, 256, st));
    void* args[] = {&g};
    AIY_HIP(h, h->ge_timer.begin(st));
    AIY_HIP(h, hipLaunchKernel(p.fn, dim3(p.blocks), dim3(p.th), args, p.lds, st));
    AIY_HIP(h, h->ge_timer.end(st));
    unsigned errw[3] = {0, 0, 0};   // error, finished clusters, clusters stopped inside a solve
    AIY_HIP(h, hipMemcpyAsync(errw, g.err, sizeof(errw), hipMemcpyDeviceToHost, st));
    AIY_HIP(h, hipMemcpyAsync(done.data(), g.out_done, sizeof(int) * n_cal, hipMemcpyDeviceToHost, st));
    AIY_HIP(h, hipStreamSynchronize(st));
    h->ge_timer.collect();
    ++h->ge_rounds;
    h->ge_mid_stops += errw[2];
    const unsigned err = errw[0];
    if (err == 1u)
      return fail(h, AIY_ERR_STATE, "device-resident GE: cluster barrier timed out (workgroups not co-resident?)");
    if (err) return fail(h, AIY_ERR_STATE, "device-resident GE: histogram shape does not fit (error %u)", err);
    std::vector<int> next;
    for (int c : active) {
      if (!done[c]) {
        next.push_back(c);
        resume[c] = 1;
      }
    }
    if ((int)next.size() == n && g.stop_at > 0)
      return fail(h, AIY_ERR_STATE, "device-resident GE: a rebalancing launch finished no calibration");
    active.swap(next);
  }
  std::vector<double> hd(3 * (size_t)n_cal);
  std::vector<int> hi(4 * (size_t)n_cal), iid_h(n_cal, 0);
  AIY_HIP(h, hipMemcpyAsync(iid_h.data(), L.iid, sizeof(int) * n_cal, hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipMemcpyAsync(hd.data(), outd, sizeof(double) * 3 * n_cal, hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipMemcpyAsync(hi.data(), outi, sizeof(int) * 4 * n_cal, hipMemcpyDeviceToHost, st));
  h->ge_prof.assign((size_t)n_cal * kGeProf, 0.0);
  h->ge_evlog.assign((size_t)n_cal * kGeEvLog * kGeEvRec, 0.0);
  AIY_HIP(h, hipMemcpyAsync(h->ge_evlog.data(), g.out_evlog, sizeof(double) * kGeEvLog * kGeEvRec * n_cal,
                            hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipMemcpyAsync(h->ge_prof.data(), g.out_prof, sizeof(double) * kGeProf * n_cal, hipMemcpyDeviceToHost,
                            st));
  AIY_HIP(h, hipStreamSynchronize(st));
  long long cyc = 0, its = 0;
  int steps = 0;
  for (int c = 0; c < n_cal; ++c) {
    h->ge_iid_cells += iid_h[c] != 0;
    r_out[c] = hd[c];
    K_out[c] = hd[n_cal + c];
    if (Ks_out) Ks_out[c] = hd[2 * n_cal + c];
    steps = std::max(steps, hi[c]);
    cyc += hi[n_cal + c];
    its += hi[2 * n_cal + c];
    if (status_out) status_out[c] = hi[3 * n_cal + c];
    h->ge_points += (double)hi[2 * n_cal + c] * S * n_a;
    h->ge_egm_cycles += hi[n_cal + c];
  }
  if (steps_out) *steps_out = steps;
  if (cyc_out) *cyc_out = (int32_t)std::min<long long>(cyc, 0x7fffffff);
  if (its_out) *its_out = (int32_t)std::min<long long>(its, 0x7fffffff);
  return 1;
}

}  // namespace aiy

using namespace aiy;

extern "C" int32_t aiy_ge_resident_plan(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t* out4) {
  if (!h || !out4) return AIY_ERR_ARG;
  GePlan p;
  if (!h->ge_resident || !ge_make_plan(h, n_cal, S, n_a, p)) {
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    return 0;
  }
  out4[0] = p.G;
  out4[1] = p.nj;
  out4[2] = p.kc;
  out4[3] = p.blocks;
  return 1;
}

// Launches of the last device-resident search (1 + rebalancing relaunches) and how many of
// its cluster stops happened inside a distribution solve (resumed from the iterate).
extern "C" int32_t aiy_ge_last_rounds(aiy_handle* h, int32_t* launches, int32_t* mid_solve_stops) {
  if (!h) return AIY_ERR_ARG;
  if (launches) *launches = h->ge_rounds;
  if (mid_solve_stops) *mid_solve_stops = h->ge_mid_stops;
  return AIY_OK;
}

// Calibrations of the last aiy_ge_stationary call whose distribution solves ran on the asset grid
// alone (i.i.d. income, AIY_OPT_HIST_IID on, the push form of the device-resident search): the flag
// each cluster's kernel set from the P it read; 0 after a host-driven search.  Host-only.
extern "C" int32_t aiy_ge_last_iid_cells(aiy_handle* h, int32_t* cells) {
  if (!h || !cells) return AIY_ERR_ARG;
  *cells = h->ge_iid_cells;
  return AIY_OK;
}

extern "C" int32_t aiy_ge_launch_stats(aiy_handle* h, double* ms_sum, int64_t* launches, double* point_matvecs,
                                       double* egm_cycles, int32_t reset) {
  if (!h) return AIY_ERR_ARG;
  h->ge_timer.read(ms_sum, launches, reset != 0);
  if (point_matvecs) *point_matvecs = h->ge_points;
  if (egm_cycles) *egm_cycles = h->ge_egm_cycles;
  if (reset) {
    h->ge_points = 0.0;
    h->ge_egm_cycles = 0.0;
  }
  return AIY_OK;
}

// Per-evaluation log of the last device-resident search (measurement hook): out[(c * 32 + e)
// * 6 + k] for evaluation e of calibration c, k = r, (K_s - K_d) / K_d, EGM cycles, matvecs,
// loose (1: a bracketing evaluation at the loose tolerances), microseconds from the
// evaluation's start (workgroup 0's clock; a solve split by a rebalancing stop includes the
// relaunch gap, its matvecs count the resumed part only); rows past
// a calibration's evaluations are zero.  Returns the calibrations written.  Host-only.
extern "C" int32_t aiy_ge_last_eval_log(aiy_handle* h, double* out, int32_t n_cal) {
  if (!h || !out || n_cal < 0) return AIY_ERR_ARG;
  const int have = (int)(h->ge_evlog.size() / (kGeEvLog * kGeEvRec));
  const int n = std::min(have, (int)n_cal);
  std::copy(h->ge_evlog.begin(), h->ge_evlog.begin() + (size_t)n * kGeEvLog * kGeEvRec, out);
  return n;
}

// Per-calibration profile of the last device-resident GE launch (measurement hook):
// out[c * 8 + k] for k = EGM, lottery, distribution solve, K reduction + search, whole
// search (microseconds, workgroup 0's clock), EGM cycles, matvecs, evaluations.  Returns
// the calibrations written (<= n_cal).  Host-only.
extern "C" int32_t aiy_ge_last_profile(aiy_handle* h, double* out, int32_t n_cal) {
  if (!h || !out || n_cal < 0) return AIY_ERR_ARG;
  const int have = (int)(h->ge_prof.size() / kGeProf);
  const int n = std::min(have, (int)n_cal);
  std::copy(h->ge_prof.begin(), h->ge_prof.begin() + (size_t)n * kGeProf, out);
  return n;
}
