/*
 * libaiyagari -- C ABI of the MI355X (gfx950) Aiyagari household block.
 *
 * Drop-in boundary for the hot path of Dostenlinus/Aiyagari-HARK:
 *   EGM backward step -> cross-sectional step (panel / histogram) -> GE loop.
 * Every entry point cites the reference interface it replaces
 * (AS = /root/reference/Aiyagari_Support.py, AH = /root/reference/Aiyagari-HARK.py,
 * [HARK] = econ-ark 0.12 library routine called from there).
 *
 * Conventions
 *  - All array arguments are DEVICE pointers owned by the caller (the Python host
 *    allocates them as PyTorch-ROCm tensors); the library allocates only inside a
 *    handle (small scratch).  Layouts are C-contiguous, float64 unless stated.
 *  - Every call returns 0 (AIY_OK) or a negative error code; aiy_last_error() gives
 *    the message.  Argument errors are detected on the host before any launch.
 *  - `stream` is a hipStream_t (NULL = the default stream).  Calls that only enqueue
 *    work are asynchronous; calls documented as BLOCKING synchronise `stream`.
 *  - One handle per (process, device); a handle is not re-entrant across threads.
 *  - Streams: calls that use the handle's scratch (EGM convergence slots and search
 *    index, panel partial sums, histogram slots, statistics scratch) may be given any
 *    stream; when a call arrives on a different stream than the previous one, the
 *    library makes the new stream wait for the old one (event hand-off), so work on two
 *    streams through one handle is serialised, never interleaved on the scratch.
 *
 * Table layout for consumption policies (the (x_list, y_list) of the reference's
 * 28 x 15 LinearInterp objects, AS:1509-1516):
 *    m[c][s][k][j], c[c][s][k][j]   c < n_cal, s < S, k < n_M, j <= n_a
 * where node j = 0 is the prepended (1e-7, 1e-7) point (AS:1503-1504).
 */
#ifndef AIYAGARI_H
#define AIYAGARI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIY_OK 0
#define AIY_ERR_ARG (-1)
#define AIY_ERR_HIP (-2)
#define AIY_ERR_STATE (-3)
#define AIY_ERR_UNSUPPORTED (-4)
#define AIY_ERR_COMM (-5)

#define AIY_MAX_STATES 64   /* S (discrete states) supported by the EGM kernel */

typedef struct aiy_handle aiy_handle;
typedef void* aiy_stream; /* hipStream_t */

/* Shapes of one batched EGM problem. */
typedef struct {
  int32_t n_cal; /* calibrations solved together (Table II batching)                 */
  int32_t S;     /* discrete states: 4 * LaborStatesNo (KS form) or N_l (stationary)  */
  int32_t n_M;   /* aggregate-M nodes (15 in the reference, AS:753-754); 1 = stationary */
  int32_t n_a;   /* exogenous end-of-period asset nodes (aGrid, AS:880)               */
} aiy_egm_dims;

/* Per-calibration inputs of solve_Aiyagari (AS:1423-1434) after precompute_arrays
 * (AS:906-1037) with the 28x-redundant current-state axis removed:
 *   mNextArray[a,k,s,s'] = R_next[k,s'] * a_grid[a] + W_next[k,s'] * lab[s']
 *   MnextArray[a,k,s,s'] = M_next[k,s'],  RnextArray[a,k,s,s'] = R_next[k,s'],
 *   ProbArray[a,k,s,s']  = P[s,s'].                                                  */
typedef struct {
  const double* a_grid; /* [n_cal][n_a]                                           */
  const double* M_grid; /* [n_cal][n_M]   Mgrid = MSS * MgridBase (AS:837-839)     */
  const double* P;      /* [n_cal][S][S]  MrkvIndArray (AS:1780)                    */
  const double* R_next; /* [n_cal][n_M][S]                                          */
  const double* W_next; /* [n_cal][n_M][S]                                          */
  const double* M_next; /* [n_cal][n_M][S] (ignored when n_M == 1)                  */
  const double* lab;    /* [n_cal][S]     LSStates[s' / 4] (AS:985, 990-1018)       */
  const double* beta;   /* [n_cal]        DiscFac                                  */
  const double* crra;   /* [n_cal]        CRRA                                     */
} aiy_egm_inputs;

/* Library version (major * 10000 + minor * 100 + patch). */
int32_t aiy_version(void);

/* Create / destroy a handle bound to HIP device `device`. */
int32_t aiy_create(int32_t device, aiy_handle** out);
int32_t aiy_destroy(aiy_handle* h);
const char* aiy_last_error(const aiy_handle* h);

/* One backward EGM step == one call of solve_Aiyagari (AS:1423-1520) for every
 * calibration of the batch.  m_next/c_next == NULL means the terminal guess
 * IdentityFunction (AS:892-904).  Asynchronous. */
int32_t aiy_egm_step(aiy_handle* h, const aiy_egm_dims* dims, const aiy_egm_inputs* in,
                     const double* m_next, const double* c_next, double* m_out, double* c_out,
                     aiy_stream stream);

/* Infinite-horizon solve == [HARK] solve_agent with cycles = 0 (AH:237): cold start
 * from the terminal guess (pre_solve, AS:806-808), iterate solve_Aiyagari until the
 * [HARK] MetricObject distance (max |dm|, |dc| over all tables) is <= tol, or
 * max_cycles + 1 cycles ran (HARK's 5000-cycle escape clause).  Each calibration
 * stops on its own cycle; converged calibrations are skipped on device.
 *   work_m/work_c: [2][n_cal][S][n_M][n_a+1] ping-pong scratch (caller-owned)
 *   m_out/c_out:   [n_cal][S][n_M][n_a+1] converged tables
 *   cycles_out/dist_out: HOST arrays [n_cal] (completed cycles, final distance)
 * BLOCKING (polls convergence every `chunk` cycles; chunk <= 0 selects 32). */
int32_t aiy_egm_solve(aiy_handle* h, const aiy_egm_dims* dims, const aiy_egm_inputs* in, double tol,
                      int32_t max_cycles, int32_t chunk, double* work_m, double* work_c,
                      double* m_out, double* c_out, int32_t* cycles_out, double* dist_out,
                      aiy_stream stream);

/* The same loop warm-started from caller tables m_init/c_init [n_cal][S][n_M][n_a+1]
 * instead of the terminal guess (build-defined: the stationary GE search E1 re-solves the
 * household at a nearby r every step; the KS-form GE keeps HARK's cold start, Q12).
 * Cycle 1 steps from the given tables.  BLOCKING. */
int32_t aiy_egm_solve_from(aiy_handle* h, const aiy_egm_dims* dims, const aiy_egm_inputs* in, double tol,
                           int32_t max_cycles, int32_t chunk, const double* m_init, const double* c_init,
                           double* work_m, double* work_c, double* m_out, double* c_out, int32_t* cycles_out,
                           double* dist_out, aiy_stream stream);

/* Measurement hook (bench.py): n_launch launches of the EGM cycle kernel alone from
 * (m_next, c_next) (search index built once, outside the timed region), each bracketed
 * by its own pair of HIP events on `stream`; *ms_out = sum of the per-launch elapsed
 * milliseconds (gaps between launches excluded).  BLOCKING. */
int32_t aiy_egm_kernel_time(aiy_handle* h, const aiy_egm_dims* dims, const aiy_egm_inputs* in,
                            const double* m_next, const double* c_next, double* m_out, double* c_out,
                            int32_t n_launch, float* ms_out, aiy_stream stream);

/* cFunc[state](m, M) for a batch of queries (interop for .solution[0].cFunc and the
 * notebook's plots, AH:271-275): HARK LinearInterpOnInterp1D semantics.
 *   tables [S][n_M][n_a+1]; state/m/M [n]; c_out [n].  Asynchronous. */
int32_t aiy_policy_eval(aiy_handle* h, int32_t S, int32_t n_M, int32_t n_a, const double* m_tab,
                        const double* c_tab, const double* M_grid, const int32_t* state,
                        const double* m, const double* M, int64_t n, double* c_out, aiy_stream stream);

/* Search index of policy rows (accelerates every HARK LinearInterp bracket search
 * without changing its result): for each of n_rows rows x[0..n1) (the m nodes of one
 * LinearInterp, x[0] > 0, sorted) build a log-bucket table of
 * aiy_index_ints_per_row() int32 so that lower_bound(x[:-1], q) is found by a search
 * over a few nodes.  Asynchronous. */
int32_t aiy_index_ints_per_row(void);
int32_t aiy_build_index(aiy_handle* h, int64_t n_rows, int32_t n1, const double* x, int32_t* index,
                        aiy_stream stream);

/* ----------------------------- panel (rows B1-B6, C2) ----------------------------- */

/* Market constants used by calc_R_and_W (AS:1839-1894). */
typedef struct {
  double cap_share;  /* CapShare */
  double depr_fac;   /* DeprFac */
  double prod[2];    /* ProdB, ProdG */
  double agg_L[2];   /* (1 - UrateB) LbrInd, (1 - UrateG) LbrInd */
} aiy_market;

/* Household panel model for one calibration (policy fixed during a history). */
typedef struct {
  int32_t S, n_M, n_a, n_lab; /* S = 4 n_lab (KS form)                                       */
  const void* tables;       /* merged policy tables of the converged policy
                               (AiyagariType.solution[0]), from aiy_panel_build              */
  const double* M_grid;     /* [n_M]                                                       */
  const double* lab_level;  /* [n_lab] LSStates (AS:1265)                                  */
  const double* lab_cdf;    /* [n_lab][n_lab] cumsum(P[l]) / last (np.random.choice)        */
  const int32_t* mrkv_hist; /* [act_T] MrkvNow_hist (AS:1793-1805)                          */
  int32_t act_T;            /* length of mrkv_hist and of the hist_A / hist_M buffers: every
                               call is checked to simulate periods t0 + n_periods <= act_T   */
  int32_t unemployed;       /* != 0: tables built with the unemployed sub-states too
                               (Krusell-Smith mode, UrateB/UrateG > 0)                       */
} aiy_panel_model;

/* Panel policy tables (get_controls, AS:1326-1408).  Each period an agent of labour
 * state l and employment e evaluates LinearInterpOnInterp1D = (1 - alpha) f_{j-1}(m) +
 * alpha f_j(m) of its sub-state s = 4 l + 2 Mrkv + e (e = 1 only unless `unemployed`).
 * For every (l, Mrkv, e, M interval j) the
 * two rows' nodes are merged into one sorted list; on each merged segment both rows'
 * brackets are fixed, so one 64-byte record holds both, and a bracket index over the
 * merged nodes (log buckets, one 64-bit entry each) finds the record with no search
 * in the common case.  HARK's arithmetic is unchanged (results bit-identical to
 * searching the two rows).
 *   aiy_panel_table_bytes: bytes of ONE calibration's tables (-1: unsupported sizes)
 *   aiy_panel_build: m_pol, c_pol [n_cal][S][n_M][n_a+1] (device) -> tables
 *                    [n_cal][aiy_panel_table_bytes] (device).  Asynchronous. */
int64_t aiy_panel_table_bytes(int32_t n_lab, int32_t n_M, int32_t n_a, int32_t unemployed);
int32_t aiy_panel_build(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_M, int32_t n_a, int32_t n_lab,
                        int32_t unemployed, const double* m_pol, const double* c_pol, void* tables,
                        aiy_stream stream);

/* Device-resident market state ("sow_state", AS:1585), 8 doubles:
 *   [0] Mnow [1] Aprev [2] Mrkv [3] Rnow [4] Wnow [5] Urate [6] sum(a) [7] period index t */
#define AIY_SOW_DOUBLES 8

/* Simulate periods t0 .. t0 + n_periods - 1 of Market.make_history (AH:249 ->
 * [HARK] Market.make_history): for each period one [HARK] sim_one_period of every
 * local agent (get_shocks AS:1217-1256, get_states AS:1259-1283, get_controls
 * AS:1286-1409, get_poststates AS:1411-1415), then mill/calc_R_and_W (AS:1839-1894)
 * on the mean of `a` over all n_total agents of all ranks, writing sow and
 * hist_A[t] = Aprev, hist_M[t] = Mnow (the track_vars of AS:1587).  sow[7] holds the
 * period index on device.
 *   a [n_local] (in: a_prev, out: a_now), lab [n_local] uint8 labour state
 *   u: NULL -> on-device Philox4x32-10 (counter (ge_iter<<20 | t, idx, 0), key seed),
 *      else host-supplied uniforms [n_periods][u_ld] starting at period t0 (parity
 *      with np.random.choice)
 *   emp: NULL -> everyone employed (UrateB = UrateG = 0), else the employment states
 *      (uint8 0/1, device) [n_periods][emp_ld] from period t0 -- this period's EmpNow of
 *      get_shocks (AS:1222-1240; exact-count permutations drawn with the agent RNG by the
 *      caller).  Needs tables with the unemployed cells (model->unemployed).
 *   agent_offset: global index of local agent 0 (Philox counter, sharding)
 * With a communicator bound (aiy_comm_init) the per-period sum of a is all-reduced
 * over RCCL before the prices are formed; otherwise n_local must equal n_total (or use
 * the two-step form below with a caller-side all-reduce).
 * Asynchronous, except that the persistent path (AIY_OPT_RESIDENT) and hipGraph replay
 * (single rank, n_periods >= 128) return after the periods completed. */
int32_t aiy_sim_periods(aiy_handle* h, const aiy_panel_model* model, const aiy_market* mkt,
                        int64_t n_local, int64_t agent_offset, int64_t n_total, double* a,
                        uint8_t* lab, const double* u, int64_t u_ld, const uint8_t* emp, int64_t emp_ld,
                        uint64_t seed, uint32_t ge_iter, int32_t t0, int32_t n_periods, double* sow,
                        double* hist_A, double* hist_M, aiy_stream stream);

/* One sharded period in two steps with the all-reduce left to the caller (any backend:
 * torch.distributed over RCCL or gloo, MPI, ...): the agent-sharded form of
 * np.mean(np.array(aNow)) (AS:1868).
 *   aiy_sim_period_local:  period t of the n_local agents (get_shocks .. get_poststates,
 *                          AS:1217-1415); leaves their sum of a in sow[6] (device).
 *                          u: NULL (Philox by global index) or n_local host uniforms of
 *                          period t; emp: NULL or the n_local employment states of t.
 *   -- caller: sow[6] <- sum over ranks of sow[6] --
 *   aiy_sim_period_prices: mill / calc_R_and_W (AS:1839-1894) on sow[6] / n_total; writes
 *                          sow, hist_A[t], hist_M[t] and advances sow[7] to t + 1.
 * Both asynchronous on `stream`, except that aiy_sim_period_local returns after the period
 * completed when it runs the resident kernel (>= 65536 local agents, even agent_offset, no
 * employment states).
 * Sharded aiy_sim_periods (a communicator bound) runs per period the same resident launch
 * (even agent_offset; parallel.shard_range splits on agent pairs), ncclAllReduce of sow[6]
 * and the price kernel, and returns after the periods completed. */
int32_t aiy_sim_period_local(aiy_handle* h, const aiy_panel_model* model, int64_t n_local,
                             int64_t agent_offset, double* a, uint8_t* lab, const double* u,
                             const uint8_t* emp, uint64_t seed, uint32_t ge_iter, int32_t t, double* sow,
                             aiy_stream stream);
int32_t aiy_sim_period_prices(aiy_handle* h, const aiy_panel_model* model, const aiy_market* mkt,
                              int64_t n_total, int32_t t, double* sow, double* hist_A, double* hist_M,
                              aiy_stream stream);

/* The reference's per-period simulation hooks one at a time, for a driver that steps
 * [HARK] Market.make_history period by period (sow -> cultivate -> reap -> mill -> store)
 * through AgentType.sim_one_period's get_shocks / get_states / get_controls /
 * get_poststates (AiyagariType, Aiyagari_Support.py:1217-1415).  One small launch each,
 * all asynchronous on `stream`; the fused aiy_sim_periods computes the same thing per
 * period in one pass.  All arrays are DEVICE arrays of the n agents unless noted.
 *   aiy_get_shocks:     lab <- inverse-CDF draw from lab_cdf[lab] (AS:1244-1256):
 *                       u = n uniforms (device) or NULL -> Philox counter
 *                       ((ge_iter << 20) | t, (agent_offset + i) / 2) as aiy_sim_periods
 *   aiy_get_states:     m = Rnow * a_prev + Wnow * lab_level[lab] * emp (AS:1276-1283);
 *                       emp NULL means everyone employed
 *   aiy_get_controls:   c = cFunc[4 lab + 2 Mrkv + emp](m, Mnow) on the RAW policy tables
 *                       m_tab / c_tab [S][n_M][n_a + 1] of aiy_egm_solve (HARK
 *                       LinearInterpOnInterp1D, AS:1295-1408); M_grid_host: HOST [n_M]
 *   aiy_get_poststates: a = m - c (AS:1415)
 *   aiy_sum:            out[0] (device) = sum of x in a fixed order (the mill's
 *                       np.mean(aNow) numerator, AS:1868) */
int32_t aiy_get_shocks(aiy_handle* h, int32_t n_lab, const double* lab_cdf, int64_t n, int64_t agent_offset,
                       uint8_t* lab, const double* u, uint64_t seed, uint32_t ge_iter, int32_t t,
                       aiy_stream stream);
int32_t aiy_get_states(aiy_handle* h, const double* lab_level, int64_t n, double Rnow, double Wnow,
                       const double* a_prev, const uint8_t* lab, const uint8_t* emp, double* m_out,
                       aiy_stream stream);
int32_t aiy_get_controls(aiy_handle* h, int32_t S, int32_t n_M, int32_t n_a, const double* m_tab,
                         const double* c_tab, const double* M_grid_host, int32_t Mrkv, double Mnow, int64_t n,
                         const double* m, const uint8_t* lab, const uint8_t* emp, double* c_out,
                         aiy_stream stream);
int32_t aiy_get_poststates(aiy_handle* h, int64_t n, const double* m, const double* c, double* a_out,
                           aiy_stream stream);
int32_t aiy_sum(aiy_handle* h, const double* x, int64_t n, double* out, aiy_stream stream);

/* Measurement hook (bench.py): n_launch periods of the panel kernel (single rank,
 * Philox shocks) -- n_launch per-period launches, each bracketed by its own pair of HIP
 * events on `stream`, or with AIY_OPT_RESIDENT one persistent launch of n_launch periods
 * between two events; *ms_out = kernel milliseconds for the n_launch periods.  Simulates
 * periods 0 .. n_launch - 1 (mrkv_hist must hold n_launch entries) and advances a/lab/sow.
 * BLOCKING. */
int32_t aiy_sim_kernel_time(aiy_handle* h, const aiy_panel_model* model, const aiy_market* mkt,
                            int64_t n_local, double* a, uint8_t* lab, uint64_t seed, uint32_t ge_iter,
                            double* sow, int32_t n_launch, float* ms_out, aiy_stream stream);

/* Persistent-panel launch statistics (measurement hook): kernel milliseconds summed over
 * the single-rank resident launches since the last reset (each bracketed by HIP events
 * on its stream), the number of launches and the periods they simulated.  reset != 0
 * zeroes the counters after reading them.  Host-only. */
int32_t aiy_panel_launch_stats(aiy_handle* h, double* ms_sum, int64_t* launches, int64_t* periods,
                               int32_t reset);

/* Batched small-population panel (Table II in the reference's Krusell-Smith mode: 350-700
 * agents per calibration, act_T = 11 000; AH:217-249).  One workgroup owns one
 * calibration: agents stay in registers for all n_periods, the per-period mean of `a`
 * is a workgroup reduction and calc_R_and_W runs on lane 0 (no grid synchronisation),
 * so a whole history is ONE launch.  Same per-period semantics as aiy_sim_periods.
 * All calibrations share (S, n_M, n_a, n_lab); arrays are stacked over calibrations. */
typedef struct {
  int32_t n_cal, S, n_M, n_a, n_lab;
  const void* tables;       /* [n_cal][aiy_panel_table_bytes], aiy_panel_build */
  const double* M_grid;     /* [n_cal][n_M] */
  const double* lab_level;  /* [n_cal][n_lab] */
  const double* lab_cdf;    /* [n_cal][n_lab][n_lab] */
  const int32_t* mrkv_hist; /* [n_cal][act_T] */
  int32_t unemployed;       /* != 0: tables with the unemployed sub-states (aiy_panel_build) */
} aiy_panel_batch;

/* Largest per-calibration population aiy_sim_block_periods accepts. */
int32_t aiy_sim_block_max_agents(void);

/* Periods t0 .. t0 + n_periods - 1 of every calibration's history.
 *   markets, seeds: HOST arrays [n_cal]
 *   a [n_cal][n_agents], lab [n_cal][n_agents] uint8 (device, in/out)
 *   u: NULL -> Philox (counter (ge_iter<<20 | t, idx/2, 0), key seeds[c]), else host
 *      uniforms [n_cal][n_periods][n_agents]
 *   emp: NULL (everyone employed) or employment states [n_cal][n_periods][n_agents]
 *      (uint8, device; as aiy_sim_periods)
 *   sow [n_cal][AIY_SOW_DOUBLES] (device, in/out); hist_A/hist_M [n_cal][act_T] or NULL.
 * Asynchronous (the call waits for earlier work on `stream` before it refills its
 * pinned staging buffer). */
int32_t aiy_sim_block_periods(aiy_handle* h, const aiy_panel_batch* model, const aiy_market* markets,
                              int64_t n_agents, double* a, uint8_t* lab, const double* u,
                              const uint8_t* emp, const uint64_t* seeds, uint32_t ge_iter, int32_t t0, int32_t n_periods,
                              int32_t act_T, double* sow, double* hist_A, double* hist_M,
                              aiy_stream stream);

/* Handle options. */
#define AIY_OPT_USE_GRAPHS 1 /* value != 0: replay panel periods from a captured hipGraph */
#define AIY_OPT_RESIDENT 2   /* value != 0 (default): single-rank panels of >= 65536 agents run
                                 a block of periods as ONE persistent launch (agents resident in
                                 LDS, in-kernel exchange of partial sums per period); 0: one launch
                                 per period */
#define AIY_OPT_HIST_FUSED 4 /* value != 0: aiy_hist_solve runs one fused push+mix launch per iteration
                              when every lottery row is monotone; 0 (default): the push/mix pair.  The
                              fused step moves 28 B per point but its borrowing-constraint tile pulls
                              thousands of sources serially: measured slower at Table II sizes */
#define AIY_OPT_RESIDENT_SHAPE 3 /* persistent panel workgroup: 0 (default) 512 threads x 8 agents
                                    per lane per pass, quad-cooperative record loads; 1: 1024
                                    threads x 4, quad-cooperative; 2: 512 x 8, per-lane record
                                    loads (results identical) */
#define AIY_OPT_RESIDENT_STREAM 5 /* value != 0: the persistent panel streams agents from HBM even
                                     when the workgroup slice would fit in LDS (the path panels of
                                     more than ~4M agents take; for tests and measurement) */
#define AIY_OPT_HIST_RESIDENT 6  /* value != 0 (default): aiy_hist_solve runs the whole distribution
                                    iteration in ONE device-resident launch (a cluster of workgroups
                                    per calibration, in-kernel barriers); 0: the push/mix launch pair */
#define AIY_OPT_HIST_CLUSTER 7   /* maximum workgroups per calibration cluster of the resident
                                    histogram (0: default 32; the minimum the grid size needs wins) */
#define AIY_OPT_HIST_ACCEL 8     /* value E > 0: the resident histogram extrapolates every E iterations
                                    along the last change when two consecutive estimates of its
                                    contraction ratio agree (Aitken; same fixed point, fewer
                                    iterations, counts differ from the plain iteration); 0 (default):
                                    the plain iteration of oracle/stationary.py */
#define AIY_OPT_HIST_KRYLOV 9     /* value != 0: the resident histogram solves (I - T) mass = 0 by
                                    BiCGSTAB from the given mass (hist_krylov.hip; stops at a mass
                                    T x with max|T x - x| < tol, the plain iteration's rule; counts
                                    are matvecs); takes precedence over AIY_OPT_HIST_ACCEL */
#define AIY_OPT_GE_RESIDENT 10    /* value != 0: aiy_ge_stationary runs the whole search of
                                    every calibration in ONE device-resident launch (each
                                    calibration's cluster: EGM cycles, lottery, BiCGSTAB, K_s and the
                                    root search on device, ge_resident.hip) when accel < 0, S <= 8
                                    and every cluster fits the device at once; else the host loop.
                                    A new handle starts at 0 (the host loop); the Python wrapper
                                    (stationary.solve_table2) sets it by default */
#define AIY_OPT_CU_LIMIT 11       /* compute units the resident launches of this handle may fill
                                    (0: the device's; several processes sharing one GPU: a share) */
#define AIY_OPT_GE_REBALANCE 12   /* value q in [1, 100] (default 55): the device-resident GE search
                                    stops every cluster at an evaluation boundary once q % of a
                                    launch's calibrations have finished and relaunches the rest on
                                    the freed compute units (larger clusters); 0: one launch */
#define AIY_OPT_GE_EXTRAP_PERIOD 13 /* device-resident GE search: EGM cycles between the geometric
                                    extrapolation checks (4 .. 1024; default 32) when
                                    AIY_OPT_GE_ANDERSON is 0 */
#define AIY_OPT_GE_ANDERSON 23     /* device-resident GE search with egm_extrapolate: every p-th EGM cycle
                                    (p in [5, 1024], default 12) the household iterate moves to the
                                    type-II Anderson combination of the last 4 plain cycles (m = 3),
                                    instead of the geometric extrapolation; the same fixed point and
                                    HARK stopping rule (sup-norm change <= tol); 0: off */
#define AIY_OPT_GE_LOGSEC 14      /* 1: with loose bracketing, while only K_s < K_d has been seen
                                    the next point is a secant of log(K_s / K_d) against
                                    log(1/beta - 1 - r) through the last two points (aimed 20 %
                                    past the predicted root, the distance to 1/beta - 1 cut by
                                    2 .. 16) instead of a bisection step, and Brent runs in those
                                    coordinates; 2 (default): also a unit-slope step from a single
                                    point; 0: bisection bracketing, Brent in r */
#define AIY_OPT_HIST_PULL 15       /* value != 0: the BiCGSTAB distribution solves of S <= 8 states
                                    (the resident GE search and aiy_hist_solve) form every matvec by
                                    PULLING each destination's lottery sources in ascending order
                                    (hist_pull.h's inverse lottery) instead of LDS-atomic pushes:
                                    deterministic run to run; 0: the push form.  S > 8 always pulls */
#define AIY_OPT_GE_LOOSE_HIST 17   /* value v in [6, 14] (default 8): the loose-bracketing evaluations'
                                    distribution tolerance is 10^-v (their sign needs |K_s - K_d| >= 5 %
                                    of K_d).  Brent's evaluations run at an adaptive tolerance
                                    between hist_tol and this one (ge_search.h ge_adapt_htol; an
                                    evaluation whose |K_s - K_d| is not well above its error is
                                    redone at hist_tol), and the evaluation the search ends on is
                                    always re-solved at hist_tol before Ks_out is reported */
#define AIY_OPT_RESIDENT_SHAPE_STREAM 18 /* workgroup shape (AIY_OPT_RESIDENT_SHAPE's values) of the resident
                                    panel's HBM-streaming form (agents beyond LDS, e.g. configs[3]);
                                    default 1 (1024 threads x 4 agents); -1: AIY_OPT_RESIDENT_SHAPE */
#define AIY_OPT_HIST_IID 24        /* value != 0 (default 1): in the device-resident GE search a calibration
                                    whose income is i.i.d. -- S >= 2 and every row of its P equal to
                                    row 0 bit for bit, decided on the device from P itself -- runs
                                    the expectation and inverse marginal utility of an EGM cycle
                                    for one state instead of S (exact: the same bits), and, in the
                                    push form, solves its distribution on the asset grid alone
                                    (mu = M mu, M = sum_s pi_s Push_s; the mass is pi (x) mu; the
                                    same stopping rule, max|T x - x| < tol).  0: such cells run the
                                    general code.  With AIY_OPT_HIST_PULL every cell keeps the
                                    general (bit-reproducible) distribution solve */
/* (options 16, 19, 20, 21 and 22 -- fused panel draws, the 25-state resident search, the
   loader-ring panel, loose Brent evaluations, the on-chip S > 8 solve -- were measured slower
   than the defaults and removed in round 5; setting them returns AIY_ERR_ARG) */
int32_t aiy_set_option(aiy_handle* h, int32_t option, int64_t value);
/* The current value of an option (so a caller can save and restore what it changes). */
int32_t aiy_get_option(aiy_handle* h, int32_t option, int64_t* value);

/* -------------------------- RCCL binding (multi-GPU, §8e) -------------------------- */
/* 128-byte ncclUniqueId created by rank 0 and broadcast by the host. */
int32_t aiy_comm_unique_id(void* out128);
int32_t aiy_comm_init(aiy_handle* h, const void* unique_id128, int32_t nranks, int32_t rank);
/* Bind a communicator the caller owns (an ncclComm_t, e.g. torch.distributed's RCCL group:
 * ProcessGroupNCCL._comm_ptr()) instead of creating one: one communicator per device in the
 * process.  It must be on the handle's device; aiy_comm_destroy then only unbinds it. */
int32_t aiy_comm_bind(aiy_handle* h, void* comm);
/* Unbind the communicator (destroying it when aiy_comm_init created it). */
int32_t aiy_comm_destroy(aiy_handle* h);
/* Sum-all-reduce of n doubles in place over the bound communicator (asynchronous). */
int32_t aiy_allreduce_sum(aiy_handle* h, double* buf, int64_t n, aiy_stream stream);

/* --------------------- stationary extensions (E1 / E2, no reference) --------------------- */

/* Young-lottery transition of each calibration's stationary household (build-defined
 * row E2): for state s and grid node j, m = R a_j + w lab[s], a' = m - c_s(m) (HARK
 * LinearInterp on the [S][n_a+1] tables), lottery onto a_grid:
 * lo[c][s][j] (int32) and wlo (weight on lo).  Asynchronous. */
int32_t aiy_hist_lottery(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const double* m_tab,
                         const double* c_tab, const double* a_grid, const double* R, const double* w,
                         const double* lab, int32_t* lo, double* wlo, aiy_stream stream);

/* Iterate mass'[s', .] = sum_s P[s, s'] * lottery_push(mass[s, .]) until the sup-norm
 * change is < tol (per calibration) or max_iter.  mass [n_cal][S][n_a] in/out,
 * work [2][n_cal][S][n_a] scratch.  K_out (HOST [n_cal]) = sum mass * a_grid;
 * iters_out (HOST [n_cal]).  BLOCKING. */
int32_t aiy_hist_solve(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const int32_t* lo,
                       const double* wlo, const double* P, const double* a_grid, double tol,
                       int32_t max_iter, int32_t chunk, double* mass, double* work, double* K_out,
                       int32_t* iters_out, aiy_stream stream);

/* ------------- stationary general equilibrium (E1 over E2, SURVEY §8b aiy_ge_bisect) ------------- */

/* A batch of stationary Aiyagari households: the EGM inputs of aiy_egm_solve with one
 * aggregate node (device arrays) and the firm of calc_R_and_W (AS:1886-1890, L = 1). */
typedef struct {
  int32_t n_cal, S, n_a;
  const double* a_grid;  /* [n_cal][n_a]  device                                  */
  const double* P;       /* [n_cal][S][S] device: income Markov chain               */
  const double* lab;     /* [n_cal][S]    device: labour levels (simple-mean norm.) */
  const double* beta;    /* [n_cal]       device: DiscFac                           */
  const double* crra;    /* [n_cal]       device: CRRA                              */
  const double* alpha;   /* [n_cal]       HOST: CapShare                            */
  const double* delta;   /* [n_cal]       HOST: DeprFac                             */
  const double* disc;    /* [n_cal]       HOST: DiscFac (bracket end 1 / beta - 1)  */
} aiy_stationary_model;

typedef struct {
  int32_t method;        /* 0: bisection on K_s(r) - K_d(r) (oracle ge_bisect); 1: bisection to a
                            sign change, then Brent's method (scipy brentq) per calibration     */
  double r_tol;          /* bracket width (bisection) / xtol (Brent)                          */
  double egm_tol;        /* household solve tolerance (sup-norm of the tables)                */
  double hist_tol;       /* distribution iteration tolerance (sup-norm of the mass)           */
  int32_t max_steps, max_egm_cycles, max_hist_iter;
  int32_t warm_hist;     /* != 0: each step's distribution starts from the previous step's     */
  int32_t warm_egm;      /* != 0: each step's household solve starts from the previous policy */
  int32_t accel;         /* Aitken period of the distribution iteration (0: plain; < 0: BiCGSTAB) */
  const double* r_lo;    /* HOST [n_cal] or NULL: -delta / 2                                   */
  const double* r_hi;    /* HOST [n_cal] or NULL: 1 / beta - 1 - 1e-9                          */
  int32_t secant_start;  /* != 0 (with warm_hist and warm_egm): from the third step on, each
                            evaluation starts its household and distribution solves at
                            cur + theta (cur - prev), theta = (r - r_cur) / (r_cur - r_prev)
                            clamped to [-1, 1] (the fixed points and stopping rules are
                            unchanged; iterates differ from the Python-driven loop)          */
  int32_t loose_bracket; /* != 0 (method 1): while a calibration's search is still bracketing
                            (bisection before the first sign change) its evaluations run to
                            the looser tolerances egm 1e-6 / hist 10^-AIY_OPT_GE_LOOSE_HIST
                            (default 1e-8); the sign of
                            K_s - K_d is taken only where |K_s - K_d| >= 5 % of K_d, else
                            the same r is evaluated again at the full tolerances          */
  int32_t egm_extrapolate; /* != 0: the household solves move a calibration's tables along
                            their last change by lambda / (1 - lambda) at chunk boundaries
                            where the cycle distances fall at a steady rate lambda (egm.hip;
                            the stopping rule is unchanged)                                   */
  int32_t* status_out;   /* HOST [n_cal] or NULL: per calibration, bit 1 = some evaluation's
                            household solve stopped at max_egm_cycles above its tolerance,
                            bit 2 = some distribution solve stopped at max_hist_iter, bit 4 =
                            the search stopped at max_steps before r_tol (0: converged)      */
} aiy_ge_options;

/* Device scratch the call needs (caller-owned `work`), -1 for bad sizes. */
int64_t aiy_ge_stationary_work_bytes(int32_t n_cal, int32_t S, int32_t n_a);

/* General equilibrium in r of every calibration (build-defined E1; no reference code):
 * per step, K_s(r) = sum(mass * a) of the stationary distribution (aiy_egm_solve ->
 * aiy_hist_lottery -> aiy_hist_solve) against K_d(r) = (alpha / (r + delta))^(1/(1-alpha)),
 * w(r) = (1 - alpha) K_d^alpha, R = 1 + r; the brackets move on the host.
 *   r_out, K_out (= K_d(r)), Ks_out (the last evaluation's K_s, may be NULL): HOST [n_cal];
 *   Ks_out always comes from a distribution solved to hist_tol: when the search ends on an
 *   evaluation at the adaptive Brent tolerance (loose bracketing), that evaluation's
 *   distribution is solved again at hist_tol from its mass before K_s is reported;
 *   steps_out: K_s evaluations; egm_cycles_out / hist_iters_out: their sums over steps and
 *   calibrations (may be NULL).  The converged tables, lottery and mass stay in `work`.
 * BLOCKING. */
int32_t aiy_ge_stationary(aiy_handle* h, const aiy_stationary_model* model, const aiy_ge_options* opt,
                          void* work, double* r_out, double* K_out, double* Ks_out, int32_t* steps_out,
                          int32_t* egm_cycles_out, int32_t* hist_iters_out, aiy_stream stream);

/* Plan of the device-resident GE search for (n_cal, S, n_a): returns 1 and out4 =
 * {workgroups per calibration cluster, asset columns per workgroup, columns per thread,
 * blocks of the launch} when aiy_ge_stationary would run it, else 0.  Host-only. */
int32_t aiy_ge_resident_plan(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t* out4);

/* Device-resident GE launch statistics (measurement hook): kernel milliseconds (HIP events
 * around each launch on its stream), launches, (state, node) point-matvecs of the
 * distribution solves and EGM cycles inside them, since the last reset.  Host-only. */
int32_t aiy_ge_launch_stats(aiy_handle* h, double* ms_sum, int64_t* launches, double* point_matvecs,
                            double* egm_cycles, int32_t reset);

/* Per-calibration profile of the last device-resident GE launch (measurement hook):
 * out[c * 8 + k], k = EGM, lottery, distribution solve, K reduction + search, whole search
 * (microseconds, workgroup 0's clock), EGM cycles, matvecs, evaluations.  Returns the
 * calibrations written (<= n_cal).  Host-only. */
int32_t aiy_ge_last_profile(aiy_handle* h, double* out, int32_t n_cal);
/* Per-evaluation log of the last device-resident search: out[(c * 32 + e) * 6 + k], k = r,
   (K_s - K_d) / K_d, EGM cycles, matvecs, loose flag, microseconds (measurement hook). */
int32_t aiy_ge_last_eval_log(aiy_handle* h, double* out, int32_t n_cal);

/* Launches of the last device-resident search (1 + its rebalancing relaunches) and how many
 * cluster stops happened inside a distribution solve (that solve resumes from its iterate in
 * the next launch).  Host-only. */
int32_t aiy_ge_last_rounds(aiy_handle* h, int32_t* launches, int32_t* mid_solve_stops);
/* Calibrations of the last aiy_ge_stationary call whose distribution solves ran on the asset
 * grid alone (AIY_OPT_HIST_IID; each cluster of the device-resident search reports what it
 * decided from its P); 0 when that call ran the host-driven loop.  Host-only. */
int32_t aiy_ge_last_iid_cells(aiy_handle* h, int32_t* cells);

/* Resident-histogram launch statistics (measurement hook): kernel milliseconds summed over
 * the device-resident distribution-iteration launches since the last reset (HIP events on
 * their stream) and their number.  reset != 0 zeroes the counters.  Host-only. */
int32_t aiy_hist_launch_stats(aiy_handle* h, double* ms_sum, int64_t* launches, int32_t reset);

/* ------------- perfect-foresight transition paths (build-defined) ------------- */

/* A batch of stationary households on a price path of T + 1 periods: the device arrays of
 * aiy_stationary_model, the path prices and the policy of the last period. */
typedef struct {
  int32_t n_cal, S, n_a, T;
  const double* a_grid;  /* [n_cal][n_a]  device                                          */
  const double* P;       /* [n_cal][S][S] device                                          */
  const double* lab;     /* [n_cal][S]    device                                          */
  const double* beta;    /* [n_cal]       device                                          */
  const double* crra;    /* [n_cal]       device                                          */
  const double* R;       /* [n_cal][T+1]  device: gross return of every period            */
  const double* w;       /* [n_cal][T+1]  device: wage of every period                    */
  const double* m_term;  /* [n_cal][S][n_a+1] device: policy of period T                  */
  const double* c_term;  /* [n_cal][S][n_a+1] device                                      */
} aiy_transition_model;

/* Device scratch both transition calls need (caller-owned `work`; the two calls use
 * disjoint parts of it), -1 for bad sizes (T < 1, n_a < 2, S outside 1..AIY_MAX_STATES).
 * Host-only. */
int64_t aiy_transition_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T);

/* Backward sweep: for u = T .. 1, (m_{u-1}, c_{u-1}) = one aiy_egm_step (n_M = 1) from
 * (m_u, c_u) with R[u], w[u] as next-period prices; lo[t], wlo[t] = aiy_hist_lottery of
 * (m_t, c_t) at R[t], w[t] for t = 0 .. T-1, taken from the step's own interpolation
 * (bit-identical to chaining the two entry points).  One launch per period, enqueued back
 * to back.
 *   lo / wlo: [T][n_cal][S][n_a] (caller-owned, device); m0_out / c0_out: [n_cal][S][n_a+1]
 *   or both NULL.  Asynchronous. */
int32_t aiy_transition_backward(aiy_handle* h, const aiy_transition_model* model, void* work, int32_t* lo,
                                double* wlo, double* m0_out, double* c0_out, aiy_stream stream);

/* Forward sweep: mass_{t+1} = lottery step of mass_t with (lo[t], wlo[t]) mixed by P, in pull
 * form (no atomics; deterministic), t = 0 .. T-1, one launch per period.
 *   mass [n_cal][S][n_a] device: in mass_0, out mass_T
 *   Ks_out HOST [n_cal][T+1]: Ks[t] = sum mass_t a_grid
 *   C_out  HOST [n_cal][T] or NULL: C[t] = sum mass_t (R[t] a + w[t] lab - a'), a' the
 *          lottery's savings wlo a[lo] + (1 - wlo) a[lo + 1]; needs R, w (device
 *          [n_cal][T+1]) and lab, which may be NULL with it.
 * Returns AIY_ERR_UNSUPPORTED, with nothing pushed and Ks_out, C_out and mass untouched, if
 * any row of lo is not non-decreasing or leaves [0, n_a - 2].  BLOCKING. */
int32_t aiy_transition_forward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                               const int32_t* lo, const double* wlo, const double* P, const double* a_grid,
                               const double* R, const double* w, const double* lab, void* work, double* mass,
                               double* Ks_out, double* C_out, aiy_stream stream);

/* aiy_transition_forward, which also keeps the marginal over assets of every period's mass:
 *   marg_out DEVICE [T+1][n_cal][n_a] (caller-owned): marg_out[t][cal][j] = sum over s, in
 *            ascending s, of mass_t[cal][s][j], t = 0 .. T -- one more launch per period, on the
 *            buffer that period's step just wrote (S times smaller than keeping the masses).
 * mass, Ks_out and C_out have the bits aiy_transition_forward gives; the row check, the
 * argument checks and the blocking are its own, and a failed row check leaves marg_out
 * untouched too.  `work` is aiy_transition_work_bytes', unchanged. */
int32_t aiy_transition_forward_marginals(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                         const int32_t* lo, const double* wlo, const double* P,
                                         const double* a_grid, const double* R, const double* w, const double* lab,
                                         void* work, double* mass, double* Ks_out, double* C_out, double* marg_out,
                                         aiy_stream stream);

/* aiy_transition_forward, which also keeps every period's mass:
 *   mass_path_out DEVICE [T+1][n_cal][S][n_a] (caller-owned): mass_0 and the buffer every period's
 *                 step just wrote, by device-to-device copies enqueued behind the launches (8 S
 *                 bytes per node and period; 4.05 GB at 24 x 7 x 10 000 nodes and T = 300).
 * No kernel differs: mass, Ks_out and C_out have the bits of the plain sweep; the row check, the
 * argument checks and the blocking are its own, and a failed row check leaves mass_path_out
 * untouched too.  `work` is aiy_transition_work_bytes', unchanged. */
int32_t aiy_transition_forward_masses(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                      const int32_t* lo, const double* wlo, const double* P,
                                      const double* a_grid, const double* R, const double* w, const double* lab,
                                      void* work, double* mass, double* Ks_out, double* C_out,
                                      double* mass_path_out, aiy_stream stream);

/* Device scratch of aiy_transition_forward_any: the regions of aiy_transition_work_bytes, then the
 * second window array ([T][n_cal][S][n_a + 1] int32) and the check's counters; -1 for the same
 * bad sizes.  A work space of this size also serves aiy_transition_backward.  Host-only. */
int64_t aiy_transition_any_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T);

/* aiy_transition_forward[_marginals] for lotteries whose rows need not be non-decreasing
 * (DESIGN.md §4r).  Per row, with the prefix maximum and the suffix minimum of lo, the sources
 * with lo = d lie in a window [jlo[d], jhi[d]); the pull of column d walks the windows of d and
 * d - 1 in ascending j and adds a source where lo says so -- the order of the push form's two
 * scattered adds, no atomics, deterministic.  On a lottery whose rows are all non-decreasing
 * mass, Ks_out, C_out and marg_out have the bits aiy_transition_forward_marginals gives.
 *   marg_out        DEVICE [T+1][n_cal][n_a] or NULL
 *   rows_turned_out HOST, one int32, or NULL: the rows (of the T n_cal S) with a decreasing pair
 *   work            DEVICE, aiy_transition_any_work_bytes(n_cal, S, n_a, T)
 * Returns AIY_ERR_UNSUPPORTED, with nothing pushed and mass, Ks_out, C_out and marg_out
 * untouched, if an entry of lo leaves [0, n_a - 2] or if a row is too disordered: its windows
 * together hold more than 4 (n_a + 1) sources (a sorted row: n_a).  aiy_last_error names which.
 * The argument checks are aiy_transition_forward's and run before any launch.  BLOCKING. */
int32_t aiy_transition_forward_any(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                   const int32_t* lo, const double* wlo, const double* P, const double* a_grid,
                                   const double* R, const double* w, const double* lab, void* work, double* mass,
                                   double* Ks_out, double* C_out, double* marg_out, int32_t* rows_turned_out,
                                   aiy_stream stream);

/* ---------- cohorts on the forward sweep: mobility (build-defined) ---------- */

#define AIY_MAX_COHORTS 16   /* G: masses one aiy_cohort_forward call carries */
#define AIY_MAX_CLASSES 32   /* Q: wealth classes of the occupancy            */

/* Device scratch of aiy_cohort_forward (caller-owned `work`): the inverse index of the n_lot
 * lottery periods, the ping-pong partner of the G cohorts, the blocks' partial sums of
 * min(n_lot, 7) + 1 periods and the class edges; -1 for bad sizes (n_lot < 1, G outside
 * 1..AIY_MAX_COHORTS, Q outside 1..AIY_MAX_CLASSES, S and n_a as aiy_transition_work_bytes).
 * A multiple of 256.  Host-only. */
int64_t aiy_cohort_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t n_lot, int32_t G, int32_t Q);

/* Forward sweep of G cohorts -- masses that share the lottery, e.g. the restrictions of one
 * distribution to G groups of households -- over T periods: every cohort takes
 * aiy_transition_forward's step, and its mass, K_out and C_out have the bits that call gives on
 * the cohort alone, whatever G, the cohort's place and the other cohorts are.  One launch per
 * period carries all cohorts: the index and the weights are read once per period.
 *   lo / wlo [n_lot][n_cal][S][n_a] device; n_lot = T: period t steps with lottery t; n_lot = 1:
 *            every period steps with the one lottery (a steady state)
 *   edges    HOST [n_cal][Q+1]: class q of calibration cal holds the nodes
 *            [edges[q], edges[q+1]); non-decreasing, edges[0] = 0, edges[Q] = n_a; repeated
 *            values (empty classes) are allowed
 *   mass     DEVICE [G][n_cal][S][n_a] (each cohort the [n_cal][S][n_a] of
 *            aiy_transition_forward): in period 0, out period T
 *   K_out    HOST [n_cal][G][T+1]: K_g[t] = sum mass_g,t a_grid
 *   C_out    HOST [n_cal][G][T] or NULL (then R, w, lab may be NULL): aiy_transition_forward's C
 *   occ_out  HOST [n_cal][G][T+1][Q]: the cohort's mass on the nodes of class q in period t
 *   inc_out  HOST [n_cal][G][T+1][S] or NULL: the cohort's mass in income state s in period t
 * occ and inc are sums without atomics whose order depends on (S, n_a, edges) only (DESIGN.md
 * §4s); period 0 reports the cohorts as given.
 * Bad sizes (also n_lot not 1 or T), bad edges or a null required buffer: AIY_ERR_ARG before any
 * launch.  A row of lo that is not non-decreasing or leaves [0, n_a - 2]: AIY_ERR_UNSUPPORTED.
 * Either way mass and every output stay untouched.  BLOCKING. */
int32_t aiy_cohort_forward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_lot,
                           int32_t G, int32_t Q, const int32_t* lo, const double* wlo, const double* P,
                           const double* a_grid, const double* R, const double* w, const double* lab,
                           const int32_t* edges, void* work, double* mass, double* K_out, double* C_out,
                           double* occ_out, double* inc_out, aiy_stream stream);

/* ------- sequence-space Jacobian of the household block (build-defined) ------- */

/* The device stages of the fake-news algorithm at a steady state; the backward sweeps are
 * aiy_transition_backward's over T + 2 periods.  All buffers are caller-owned device memory and
 * every call is ordered on `stream`. */

/* Device scratch of the three calls below for a Jacobian of T rows (the inverse index of
 * T + 1 lottery periods, the expectation recursion's two mixed vectors and the contraction's
 * partials), -1 for bad sizes (T < 1, n_a < 2, S outside 1..AIY_MAX_STATES).  Host-only. */
int64_t aiy_jacobian_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T);

/* Fan-out step: out[t] = lottery step of the ONE distribution `mass` with (lo[t], wlo[t]) mixed
 * by P, for every period t < n_t (n_t <= T + 1, T the size `work` was asked for) in one launch;
 * each out[t] has the bits of aiy_transition_forward with T = 1 on that period.
 *   lo / wlo: [n_t][n_cal][S][n_a]; mass: [n_cal][S][n_a] (read only); out: [n_t][n_cal][S][n_a]
 * Returns AIY_ERR_UNSUPPORTED, with nothing written to out, if any row of lo is not
 * non-decreasing or leaves [0, n_a - 2].  Blocks on `stream` for that check; the step itself
 * is asynchronous. */
int32_t aiy_jacobian_fanout(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_t,
                            const int32_t* lo, const double* wlo, const double* P, const double* mass,
                            void* work, double* out, aiy_stream stream);

/* shocked[i] = (shocked[i] - ghost[i]) / step for i < n: the distribution responses, formed
 * element by element before anything is summed.  Asynchronous. */
int32_t aiy_jacobian_diff(aiy_handle* h, int64_t n, double* shocked, const double* ghost, double step,
                          aiy_stream stream);

/* Expectation vectors of the lottery (lo, wlo) [n_cal][S][n_a]: E_0[s][j] = a_grid[j],
 * E_{k+1}[s][j] = wlo G[s][lo] + (1 - wlo) G[s][lo + 1], G[s][d] = sum_{s'} P[s, s'] E_k[s'][d]
 * in ascending s' (the transpose of the lottery step), k = 0 .. T - 2; one launch per k.
 *   E_out: [T][n_cal][S][n_a]
 * The lottery passes aiy_jacobian_fanout's row check first (AIY_ERR_UNSUPPORTED, nothing
 * written; blocks on `stream` for it). */
int32_t aiy_jacobian_expectation(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                 const int32_t* lo, const double* wlo, const double* P, const double* a_grid,
                                 void* work, double* E_out, aiy_stream stream);

/* Fake-news contraction on the f64 matrix instruction:
 *   F_out[cal][t][c]         = sum_{s, j} E[t][cal][s][j] dD_R[c][cal][s][j]
 *   F_out[cal][t][T + 1 + c] = sum_{s, j} E[t][cal][s][j] dD_w[c][cal][s][j],  t < T, c <= T,
 * one pass over E for both.  The long index (s, j) is summed in chunks of a fixed length,
 * the chunks in ascending order: the bits depend on neither the device nor the batch.
 *   E: [T][n_cal][S][n_a]; dD_R / dD_w: [T+1][n_cal][S][n_a]; F_out: DEVICE [n_cal][T][2(T+1)]
 * Asynchronous. */
int32_t aiy_jacobian_contract(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, const double* E,
                              const double* dD_R, const double* dD_w, void* work, double* F_out,
                              aiy_stream stream);

/* ------- aggregate risk with linearised policies (build-defined) ------- */

/* The savings policy a lottery stands for, out = wlo a[lo] + (1 - wlo) a[lo + 1] element by
 * element (a = the calibration's row of a_grid [n_cal][n_a]), for the n_t periods of a lottery.
 *   lo / wlo / out: [n_t][n_cal][S][n_a]
 * lo is read as held to [0, n_a - 2].  Asynchronous. */
int32_t aiy_lottery_mean(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t n_t, const int32_t* lo,
                         const double* wlo, const double* a_grid, double* out, aiy_stream stream);

/* Young lotteries of n_p periods from linearised policies, on the f64 matrix instruction:
 *   a'[p][cal][s][j] = a_star[cal][s][j] + sum_k op[k][cal][s][j] X[cal][p][k],  k < 2 (T + 1),
 * op[k] = dA_R[k] for k <= T and dA_w[k - T - 1] after it; k ascends, the sum is added to
 * a_star last, a' is clamped to [a_0, a_{n_a - 1}] of the calibration's grid, and
 *   lo = clip(upper_bound(a, a') - 1, 0, n_a - 2),  wlo = clip((a[lo+1] - a') / (a[lo+1] - a[lo]), 0, 1).
 * A period's lottery has the same bits whatever n_p, its place among the periods and the batch.
 *   a_star: [n_cal][S][n_a]; dA_R / dA_w: [T+1][n_cal][S][n_a]; X: [n_cal][n_p][2(T+1)];
 *   lo_out / wlo_out: [n_p][n_cal][S][n_a], the lottery aiy_transition_forward takes
 * AIY_ERR_ARG, nothing written, for T < 1, n_p < 1, bad sizes or a null buffer.  Asynchronous. */
int32_t aiy_aggregate_lotteries(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_p,
                                const double* a_star, const double* dA_R, const double* dA_w, const double* X,
                                const double* a_grid, int32_t* lo_out, double* wlo_out, aiy_stream stream);

/* ------------------- wealth-distribution statistics ------------------- */

/* HARK 0.12 get_lorenz_shares(data, weights, percentiles) and get_percentiles(...) of a
 * DEVICE array (the notebook's sim_wealth, Aiyagari-HARK.py:311-316): n doubles `data`,
 * optional device `weights` (NULL: unit weights), n_p <= 256 HOST percentiles in (0, 1).
 * lorenz_out / pctl_out: HOST [n_p] (either may be NULL).  Scratch is handle-owned.
 * BLOCKING (synchronises `stream`). */
int32_t aiy_wealth_stats(aiy_handle* h, const double* data, const double* weights, int64_t n,
                         const double* pctiles, int32_t n_p, double* lorenz_out, double* pctl_out,
                         aiy_stream stream);

/* ------- wealth statistics of histogram distributions (build-defined) ------- */

/* Statistics of distributions over the ascending asset grid (no sort): for the marginal g[n_a]
 * of one distribution, cw = cumsum(g), cd = cumsum(a g), F = cw / cw[-1], L = cd / cd[-1];
 * Lorenz shares np.interp(p, F, L) and percentiles interp1d(F, a, bounds_error=False)(p) (HARK
 * 0.12 get_lorenz_shares / get_percentiles with weights = g, presorted; NaN for p < F[0]), and
 * gini = 1 - sum_j (F[j] - F[j-1]) (L[j] + L[j-1]), F[-1] = L[-1] = 0. */

/* Device scratch of aiy_dist_stats for n_dist distributions of n_a nodes (cw and cd of every
 * distribution, then the results), -1 for n_dist < 1 or n_a < 2.  Host-only. */
int64_t aiy_dist_stats_work_bytes(int32_t n_dist, int32_t n_a);

/* g[d][j] = sum over s, in ascending s, of mass[d][s][j]: the marginals of a stack.
 *   mass: DEVICE [n_dist][S][n_a]; g: DEVICE [n_dist][n_a].  No atomics.  Asynchronous. */
int32_t aiy_dist_marginal(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, const double* mass, double* g,
                          aiy_stream stream);

/* The statistics of a stack of marginals in one launch, one workgroup per distribution; every
 * sum order depends on n_a only, so a distribution has the same bits alone and in any stack.
 *   g           DEVICE [n_dist][n_a]
 *   a_grid      DEVICE [n_grid][n_a]; distribution d uses grid d % n_grid (a [T+1][n_cal] stack
 *               addresses its calibration's grid with n_grid = n_cal)
 *   pctiles     HOST [n_p], in (0, 1), n_p <= 256; may be NULL with n_p = 0
 *   work        DEVICE, aiy_dist_stats_work_bytes(n_dist, n_a)
 *   lorenz_out / pctl_out  HOST [n_dist][n_p] (either may be NULL)
 *   summary_out HOST [n_dist][4]: total = cw[-1], mean = cd[-1] / cw[-1], gini,
 *               bottom_share = g[0] / cw[-1] (may be NULL)
 * AIY_ERR_ARG for a percentile outside (0, 1), AIY_ERR_UNSUPPORTED for n_p > 256, both before
 * any device work.  BLOCKING (synchronises `stream`). */
int32_t aiy_dist_stats(aiy_handle* h, int32_t n_dist, int32_t n_grid, int32_t n_a, const double* g,
                       const double* a_grid, const double* pctiles, int32_t n_p, void* work, double* lorenz_out,
                       double* pctl_out, double* summary_out, aiy_stream stream);

/* ------- statistics of any household variable (build-defined) ------- */

/* The variables of a node (s, j) of a period with lottery (lo, wlo) and prices (R, w), a' the
 * lottery's savings wlo a[lo] + (1 - wlo) a[lo + 1] (lo read as held to [0, n_a - 2]):
 *   consumption  (R a_j + w lab_s) - a'        (c_t[s][j] of the welfare section below)
 *   income       (R - 1) a_j + w lab_s
 *   earnings     w lab_s
 *   cash         R a_j + w lab_s
 *   saving       a' - a_j
 *   wealth       a_j
 * each with the operations of the expression as written (the NumPy expressions' bits). */
#define AIY_VAR_CONSUMPTION 1
#define AIY_VAR_INCOME 2
#define AIY_VAR_EARNINGS 4
#define AIY_VAR_CASH 8
#define AIY_VAR_SAVING 16
#define AIY_VAR_WEALTH 32
#define AIY_VAR_MAX_MOMENTS 8

/* Device scratch of aiy_var_merge and aiy_var_moments for n_dist distributions (the check's flag
 * and the moments of every distribution), -1 for n_dist < 1, n_a < 2, S outside
 * 1..AIY_MAX_STATES or S n_a >= 2^31.  Host-only. */
int64_t aiy_var_work_bytes(int32_t n_dist, int32_t S, int32_t n_a);

/* The variables named by the bit mask `which` (AIY_VAR_*), element by element, no atomics:
 *   lo / wlo  [n_t][n_cal][S][n_a] (may be NULL unless consumption or saving is asked for)
 *   R / w     DEVICE, period t of calibration cal at [cal * ld_price + t], ld_price >= n_t
 *   a_grid    [n_cal][n_a]; lab [n_cal][S]
 *   out       DEVICE: the variables asked for in ascending bit order, each [n_t][n_cal][S][n_a]
 * Asynchronous. */
int32_t aiy_household_variables(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t n_t,
                                const int32_t* lo, const double* wlo, const double* R, const double* w,
                                int32_t ld_price, const double* a_grid, const double* lab, int32_t which,
                                double* out, aiy_stream stream);

/* Orders every distribution of a stack whose S rows are each nondecreasing: an S-way merge.
 *   key / weight               DEVICE [n_dist][S][n_a]
 *   key_sorted / weight_sorted DEVICE [n_dist][S n_a]: the order of
 *                              np.argsort(key.reshape(-1), kind="stable"), by key, ties by (s, j)
 *   rank_out                   DEVICE int32 [n_dist][S][n_a] or NULL: the place of (s, j), j plus,
 *                              for every other row s', its entries with key <= y (s' < s) or
 *                              key < y (s' > s)
 *   work                       DEVICE, aiy_var_work_bytes(n_dist, S, n_a)
 * Every output element is a copy of an input element: the same bits in every run, alone or in a
 * stack.  No atomics, no sort.  A first pass checks that every row is nondecreasing and free of
 * NaN; AIY_ERR_UNSUPPORTED with nothing written if one is not.  AIY_ERR_ARG for bad sizes or a
 * null buffer, before any launch.  Blocks for the check's flag; the merge itself is enqueued. */
int32_t aiy_var_merge(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, const double* key,
                      const double* weight, void* work, double* key_sorted, double* weight_sorted,
                      int32_t* rank_out, aiy_stream stream);

/* Weighted moments of n_v <= AIY_VAR_MAX_MOMENTS variables on one weight stack, one launch, two
 * passes (means, then centred products; not sum w y^2 - m^2); the rows need not be monotone.
 *   vars   HOST array of n_v DEVICE pointers, each [n_dist][S][n_a]; weight DEVICE, the same shape
 *   work   DEVICE, aiy_var_work_bytes(n_dist, S, n_a)
 *   out    HOST [n_dist][1 + n_v + n_v n_v]: sum w, the means m_u = sum w y_u / sum w, then
 *          sum w (y_u - m_u)(y_v - m_v) / sum w at [1 + n_v + u n_v + v]
 * Sum order: a row (d, s) in contiguous chunks of ceil(n_a / 256) nodes reduced as
 * aiy_dist_stats reduces its Gini terms, then the rows in ascending s.  BLOCKING. */
int32_t aiy_var_moments(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, int32_t n_v,
                        const double* const* vars, const double* weight, void* work, double* out,
                        aiy_stream stream);

/* ---- welfare: values on the histogram and consumption equivalents (build-defined) ---- */

/* The exact expected discounted utility of the discretised economy.  The histogram is a Markov
 * chain on (s, a_j): a household at node (s, j) of period t consumes
 *   c_t[s][j] = R_t a_j + w_t lab_s - (wlo a[lo] + (1 - wlo) a[lo + 1])
 * (the term aiy_transition_forward sums into C_out), moves to lo / lo + 1 with weights
 * wlo / 1 - wlo and draws s' from P[s, .], so
 *   V_t[s][j]     = u(c_t[s][j]) + beta (wlo G_{t+1}[s][lo] + (1 - wlo) G_{t+1}[s][lo + 1])
 *   G_{t+1}[s][d] = sum over s', ascending, of P[s, s'] V_{t+1}[s'][d]
 *   u(c) = log c for CRRA = 1, c^(1 - CRRA) / (1 - CRRA) otherwise (HARK's CRRAutility, no -1).
 * The recursion is the transpose of the forward lottery step, hence, to rounding,
 *   sum mass_0 V_0 = sum_{t<T} beta^t sum mass_t u(c_t) + beta^T sum mass_T V_T.
 * c = 0 gives u = -inf and c < 0 gives NaN: a non-finite V, never a fault or a device-side error.
 * The sum order of G depends on S only and nothing else is summed: a calibration has the same
 * bits alone and in any batch.  lab, beta, crra: device, as in aiy_transition_model. */

/* Device scratch of the two value calls below: two [n_cal][S][n_a] buffers for G and the
 * convergence slots; -1 for n_a < 2 or S outside 1..AIY_MAX_STATES.  Host-only. */
int64_t aiy_value_work_bytes(int32_t n_cal, int32_t S, int32_t n_a);

/* V_t for t = T-1 .. 0 from V_term = V_T on the lotteries and prices of a path: one launch mixes
 * V_term into G, then one fused launch per period (u(c), the gather from G_{t+1}, V_t, and G_t
 * mixed by P through LDS), enqueued back to back.
 *   lo / wlo   [T][n_cal][S][n_a]; R / w [n_cal][T+1]; V_term [n_cal][S][n_a]
 *   V0_out     [n_cal][S][n_a]: V_0
 *   V_path_out [T][n_cal][S][n_a] or NULL: every V_t (V_path_out[0] has the bits of V0_out)
 * Null pointers and T < 1 give AIY_ERR_ARG before any launch.  A lottery index outside
 * [0, n_a - 2] is read as the nearest one inside.  Asynchronous. */
int32_t aiy_value_backward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, const int32_t* lo,
                           const double* wlo, const double* P, const double* a_grid, const double* R,
                           const double* w, const double* lab, const double* beta, const double* crra,
                           const double* V_term, void* work, double* V0_out, double* V_path_out,
                           aiy_stream stream);

/* The steady value V = u(c) + beta Lambda V of the one lottery (lo, wlo) [n_cal][S][n_a] at the
 * prices R, w [n_cal]: the same step iterated from the V given.  A calibration stops once
 *   max |V_new - V| <= tol (1 - beta) / beta max |V_new|,
 * which bounds |V - V*| by tol max |V| (contraction of modulus beta); both maxima come out of the
 * step's launch into per-calibration slots, polled every `chunk` steps (chunk <= 0: 32), and a
 * calibration that has stopped is skipped on device.  tol < 1e-13 is refused (AIY_ERR_ARG):
 * rounding alone moves V by more per step.
 *   beta_host HOST [n_cal]: the values of beta; V [n_cal][S][n_a] in: the start, out: the value
 *   iters_out / dist_out HOST [n_cal]: steps run and the last max |V_new - V|; a calibration
 *   still running at max_iter has iters_out == max_iter (nothing is raised).  BLOCKING. */
int32_t aiy_value_stationary(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const int32_t* lo,
                             const double* wlo, const double* P, const double* a_grid, const double* R,
                             const double* w, const double* lab, const double* beta, const double* crra,
                             const double* beta_host, double tol, int32_t max_iter, int32_t chunk, double* V,
                             void* work, int32_t* iters_out, double* dist_out, aiy_stream stream);

/* W_out[c][s] = sum_j mass[c][s][j] V[c][s][j] (HOST [n_cal][S]; mass, V device): one workgroup
 * per row, in aiy_dist_stats' order -- contiguous chunks of ceil(n_a / 256) nodes summed
 * sequentially, then lanes and waves in a fixed order that depends on n_a only.  BLOCKING. */
int32_t aiy_value_reduce(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const double* mass,
                         const double* V, double* W_out, aiy_stream stream);

/* Consumption equivalent of every node, g_out[i] for i < n_cal * per (calibration i / per):
 *   g = (V_new / V_base)^(1 / (1 - CRRA)) - 1 for CRRA != 1, exp((1 - beta)(V_new - V_base)) - 1
 * for CRRA = 1: the uniform proportional change of consumption in every period and state that
 * takes a household from V_base to V_new.  Elementwise.  Asynchronous. */
int32_t aiy_consumption_equivalent(aiy_handle* h, int32_t n_cal, int64_t per, const double* V_new,
                                   const double* V_base, const double* beta, const double* crra, double* g_out,
                                   aiy_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* AIYAGARI_H */
