// The BiCGSTAB distribution solve of one calibration's cluster (build-defined row E2,
// Krylov mode) as a device function: hist_krylov.hip runs one solve per launch,
// ge_resident.hip many solves per launch inside its device-resident GE search.
// See hist_krylov.hip for the algorithm.
// A lottery that is not "monotone, of ours" stops the cluster with error 2 before the first
// matvec, in both forms and from every entry: the pull form needs every row non-decreasing
// inside the grid; the push form needs every own entry of a workgroup inside the grid and inside
// the bracket [lo(j0), lo(j1 - 1)] of its row's end columns (neighbours that swap order inside
// the bracket are harmless to a push and run).
#pragma once

#include "common.h"
#include "hist_cluster.h"

namespace aiy {

constexpr int kHkStall = 256;   // matvecs without a 10 % residual gain that count as a stall
constexpr double kHkStopSentinel = 1e300;   // rebalancing stop request on the max|r| partial
// Destinations covered by more than two spans (the borrowing constraint, the top of the grid:
// up to kHcCand covering workgroups) are summed by a whole wave, one candidate per lane, instead
// of a serial per-lane loop whose dependent slab loads put the owning workgroup ~2 us behind the
// others every matvec (tools/hist_phases.py at G = 32: its gather 4.2 vs 1.6-2.4 us).  Up to
// kHkHeavy such (column, state) entries per workgroup; more fall back to the per-lane loop.
constexpr int kHkHeavy = 31;
// only destinations with more than kHkWaveCn covering spans take a wave-parallel entry; the
// others (3 .. kHkWaveCn spans: the destinations of the lowest workgroup's range that several
// neighbours' dissaving sources reach, often hundreds of them) load their extra candidates 2
// and 3 for every state at once, one round trip instead of one per state (Table II sweep
// 60.5 -> 57.9 ms against kHkWaveCn = 2, gpurun_out r07a abt2)
#ifndef AIY_HK_WAVE_CN
#define AIY_HK_WAVE_CN 6
#endif
constexpr int kHkWaveCn = AIY_HK_WAVE_CN;
static_assert(kHcCand <= 32, "covering-span index and count packed in 5 + 6 bits");
// covering info of one (column, state): first candidate (5 bits), count (6 bits), heavy-entry
// index (5 bits; kHkHeavy = none)
__device__ __forceinline__ unsigned short hk_cinfo(int cf, int cn, int hi) {
  return (unsigned short)(cf | (cn << 5) | (hi << 11));
}
__device__ __forceinline__ int hk_cf(int ci) { return ci & 31; }
__device__ __forceinline__ int hk_cn(int ci) { return (ci >> 5) & 63; }
__device__ __forceinline__ int hk_hi(int ci) { return ci >> 11; }

// a wave-uniform double kept in SGPRs (the solve's scalars: otherwise VGPR pairs that the
// pipelined form spilled to scratch inside its loop)
__device__ __forceinline__ double hk_uni(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// shadow residual: a fixed pseudo-random value in [-1, 1) per point index q = s n_a + j
__device__ __forceinline__ double hk_rhat(unsigned q) {
  unsigned h = q * 0x9E3779B1u + 0x7F4A7C15u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return (double)(int)h * (1.0 / 2147483648.0);
}

// Phase timing (diagnostic builds, -DAIY_DIAG_PHASES=<block>: that block and the next 9,
// i.e. one calibration's cluster at Table II size): time since the previous
// mark is added to slot k: 0 push, 1 publish, 2 matvec barrier, 3 gather + mix,
// 4 reductions (partials, publish, barrier, read), 5 vector updates
#ifdef AIY_DIAG_PHASES
#define HK_PH(k)                                                        \
  do {                                                                  \
    if (tid == 0 && blockIdx.x >= AIY_DIAG_PHASES && blockIdx.x < AIY_DIAG_PHASES + 10) { \
      const unsigned long long tn = __builtin_amdgcn_s_memrealtime();   \
      if ((k) >= 0) ph[(k)] += tn - tq;                                 \
      tq = tn;                                                          \
    }                                                                   \
  } while (0)
#define HK_PH_REPORT(mv)                                                                                           \
  do {                                                                                                             \
    if (tid == 0 && blockIdx.x >= AIY_DIAG_PHASES && blockIdx.x < AIY_DIAG_PHASES + 10 && (mv) > 0)                \
      printf("[bicg phases] block %d G=%d nj=%d matvecs=%d us/matvec: push %.2f publish %.2f barrier %.2f "        \
             "gather+mix %.2f reduce %.2f vector %.2f\n",                                                          \
             (int)blockIdx.x, G, j1 - j0, (mv), ph[0] * 0.01 / (mv), ph[1] * 0.01 / (mv), ph[2] * 0.01 / (mv),     \
             ph[3] * 0.01 / (mv), ph[4] * 0.01 / (mv), ph[5] * 0.01 / (mv));                                       \
  } while (0)
#else
#define HK_PH(k) \
  do {           \
  } while (0)
#define HK_PH_REPORT(mv) \
  do {                   \
  } while (0)
#endif

template <int SMAX, int KC, int TH>
struct HkShared {
  double* Tacc;                    // span buffer (cap doubles); for SMAX <= 8 then v
  int* s_base;                     // [SMAX]
  int (*s_pub)[2];                 // [2 SMAX][2]
  int* s_tot;
  HcCand (*s_cand)[kHcCand];       // [SMAX][kHcCand]
  int* s_ncand;                    // [SMAX]
  unsigned short* s_cinfo;         // [KC SMAX TH]
  double* s_P;                     // [SMAX SMAX]
  double (*s_part)[TH / kWave];    // [kHcRed]
  double* s_res;                   // [kHcRed]
  int* s_flag;
  int* s_stop;
  int* s_ex;                       // [SMAX][2] pull form: exported prefix / suffix of the own sources
  int* s_nheavy;                   // heavy (column, state) entries of this workgroup
  int* s_wcnt;                     // [TH / kWave] per-wave counts while numbering them
  int (*s_heavy)[4];               // [kHkHeavy] (k, s, tid, cf | cn << 8)
  double* s_hval;                  // [kHkHeavy] their wave sums
  int* s_rok;                      // reduction riding on a matvec barrier: granules read in time
};

// One calibration's BiCGSTAB distribution solve by the workgroups of its cluster (this
// workgroup: w of G, own columns [j0, j1)); shared by hist_bicg_kernel (one solve per
// launch) and the device-resident GE search (ge_resident.hip, many solves per launch).
// (pointers typed global: hk_solve_isolated receives them as plain arguments, where the
// compiler could not infer their address space and would use flat accesses)
struct HkArgs {
  int G, S, n_a, cap, w, j0, j1;
  gptr<const int> LO;          // [S][n_a] lottery of the calibration (index)
  gptr<const double> WL;       // [S][n_a] lottery weight on lo
  gptr<double> X;              // [S][n_a] in: start, out: T x (own columns)
  gptr<double> Pg;             // [S][n_a] p scratch rows
  gptr<double> Vg;             // v block of this workgroup in HBM (SMAX > 8)
  gptr<double> slab_cl;        // [G][2][cap]
  gptr<int> span_cl;           // [G][SMAX][4]
  gptr<unsigned> ctr;          // cluster barrier counter
  gptr<unsigned long long> gran;   // [2][G][kHcRedRec] reduction granules
  gptr<const double> Pc;       // [S][S]
  double tol;
  int max_iter;
  gptr<unsigned> err;
  // rebalancing (ge_resident.hip): stop at the next iteration once *stop_ctr >= stop_at
  // (nullptr: never); the solve then returns -(2 + matvecs) with X a valid iterate
  gptr<const unsigned> stop_ctr;
  unsigned stop_at;
  // pull form of the matvec (PULL = true, hist_pull.h's lottery pull with the vectors kept in
  // registers): the matvec input staged in Qg, the inverse lottery in Ainv
  gptr<double> Qg;             // [S][n_a]
  gptr<int> Ainv;              // [S][n_a + 1]
  bool lottery_fresh;          // LO / WL written in this launch by other workgroups (sc1 loads)
  // hk_solve_isolated: the LDS address of the caller's dynamic shared memory (hk_lds_addr).
  // Declared in the callee, a non-kernel function, it is found through the module's dynamic-LDS
  // table, and the compiler reloads that word from memory in front of almost every LDS access
  // (228 scalar loads in the two-column loop, each with a wait that drains the LDS queue)
  unsigned dyn_lds;
};

template <class T>
using lptr = __attribute__((address_space(3))) T*;
// the 32-bit LDS address of a __shared__ object, opaque to the compiler: handed on plainly,
// interprocedural constant propagation puts the dynamic-LDS symbol back into the callee
__device__ __forceinline__ unsigned hk_lds_addr(double* p) {
  unsigned a = (unsigned)(size_t)(lptr<double>)p;
  asm volatile("" : "+s"(a));
  return a;
}

// Returns the matvecs of the solve, or -1 when the cluster stops (error word set: a
// timeout, a span that does not fit, too many covering workgroups), or -(2 + matvecs) when
// a rebalancing stop was requested (X holds the current iterate; a later solve restarts
// from it).  nb / ne: the
// cluster barriers / reductions passed so far in this launch (counted on).
//
// IID (push form): the calibration's income is i.i.d. -- every row of P is the same vector pi, bit
// for bit (the caller's test) -- so T x = pi (x) (M mu) for any x, with mu[j] = sum_s x[s][j] and
// M = sum_s pi_s Push_s on the asset grid alone.  The solve then runs on mu: ONE unknown per column
// instead of S.  The lottery push, the spans, the publish and the cluster exchange are the general
// form's (state s pushes pi_s mu[j]); the gather sums the states (no P mix); r, p, v, t, x and u of
// a column stay in registers at one and at two columns per thread (no Pg / X traffic inside the
// loop, no v in LDS), and so does its lottery.  X is the interface as before: in, the start, read
// as mu0[j] = sum_s X[s][j]; out, pi_s (M mu)[j], also at a rebalancing stop (pi_s mu[j]).  The loop
// runs at tol / max_s pi_s: max|M mu - mu| max pi < tol is the full vector's max|T x - x| < tol.
template <int SMAX, int KC, int TH, bool PULL = false, bool FUSEA = false, int SC = 0, bool IID = false>
__device__ __forceinline__ int hk_solve(const HkArgs& r, const HkShared<SMAX, KC, TH>& L, unsigned& nb,
                                        unsigned& ne) {
  constexpr bool kVlds = SMAX <= 8;
  static_assert(!IID || (!PULL && SMAX <= 8), "the asset-grid solve: push form, S <= 8");
  constexpr int NV = IID ? 1 : SMAX;   // unknowns per column
#ifdef AIY_DIAG_PHASES
  unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, tq = 0;
#endif
  double* Tacc = L.Tacc;
  int* s_base = L.s_base;
  int (*s_pub)[2] = L.s_pub;
  HcCand (*s_cand)[kHcCand] = L.s_cand;
  int* s_ncand = L.s_ncand;
  unsigned short* s_cinfo = L.s_cinfo;
  double* s_P = L.s_P;
  double (*s_part)[TH / kWave] = L.s_part;
  double* s_res = L.s_res;
  int& s_flag = *L.s_flag;
  int& s_stop = *L.s_stop;
  int& s_tot = *L.s_tot;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wid = tid / kWave;
  // SC > 0: the state count at compile time (the resident search's Table II kernels, S == SMAX:
  // no per-state branches or clamps); 0: r.S
  static_assert(SC >= 0 && SC <= SMAX, "compile-time state count within SMAX");
  const int G = r.G, S = SC > 0 ? SC : r.S, n_a = r.n_a, cap = r.cap;
  const int w = r.w;
  const int j0 = r.j0;
  const int j1 = r.j1;
  unsigned* ctr = (unsigned*)r.ctr;
  unsigned long long* gran = (unsigned long long*)r.gran;
  const int* LO = (const int*)r.LO;
  const double* WL = (const double*)r.WL;
  double* X = (double*)r.X;   // x: the iterate, own columns read-modify-written
  double* slab_cl = (double*)r.slab_cl;
  const double* __restrict__ Pc = (const double*)r.Pc;
  int* span_cl = (int*)r.span_cl;
  unsigned* err = (unsigned*)r.err;

  // ---- setup (as hist_cluster_kernel): P, own spans, covering candidates ----
  for (int q = tid; q < SMAX * SMAX; q += TH) {
    const int s = q / SMAX, sp = q - s * SMAX;
    s_P[q] = (s < S && sp < S) ? Pc[s * S + sp] : 0.0;
  }
  auto barrier = [&]() -> bool {
    ++nb;
    return hc_barrier(err, ctr, (unsigned)G * nb, &s_flag);
  };
  // pull form: the inverse lottery of the own destinations, staged in LDS (Tacc's space)
  const int n_own = j1 - j0, aspan = n_own + 2;
  int* s_A = reinterpret_cast<int*>(Tacc);
  int* s_ex = L.s_ex;
  int* Ainv = (int*)r.Ainv;
  double* Qg = (double*)r.Qg;
  if constexpr (PULL) {
    const int n1 = n_a + 1;
    unsigned bad = 0u;
    // a lottery written in this launch (the resident GE search): every workgroup's entries are
    // in memory before the neighbour's column j0 - 1 is read
    if (r.lottery_fresh) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (!barrier()) return -1;
    }
    for (int q = tid; q < S * n_own; q += TH) {
      const int s = q / n_own, j = j0 + (q - s * n_own);
      const int l = hc_lo_at(LO, n_a, r.lottery_fresh, s, j);
      const int lp = j > 0 ? hc_lo_at(LO, n_a, r.lottery_fresh, s, j - 1) : -1;
      // only a monotone lottery inside the grid is scattered (anything else: error 2, the
      // caller falls back); the loops never index outside the row
      const bool ok = l >= 0 && l <= n_a - 2 && lp >= -1 && lp <= l;
      if (!ok) {
        bad = 2u;
        continue;
      }
      for (int d = lp + 1; d <= l; ++d)
        __hip_atomic_store(to_global(&Ainv[(size_t)s * n1 + d]), j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (j == n_a - 1)
        for (int d = l + 1; d <= n_a; ++d)
          __hip_atomic_store(to_global(&Ainv[(size_t)s * n1 + d]), n_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (S * aspan * (int)sizeof(int) > cap * (int)sizeof(double)) bad = 2u;
    if (bad) __hip_atomic_store(to_global(err), bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hc_exported(LO, n_a, r.lottery_fresh, S, j0, j1, s_ex);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!barrier()) return -1;
    if (hc_failed(err, &s_stop)) return -1;
    for (int q = tid; q < S * aspan; q += TH) {   // A(d) for d in [j0 - 1, j1] (A(-1) = 0)
      const int s = q / aspan, d = j0 - 1 + (q - s * aspan);
      s_A[q] = d < 0 ? 0 : __hip_atomic_load(to_global(&Ainv[(size_t)s * n1 + d]), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
  if (!PULL && tid == 0) {
    int tot = 0;
    unsigned bad = 0;
    for (int s = 0; s < S; ++s) {
      const int f = LO[(size_t)s * n_a + j0];
      const int l = LO[(size_t)s * n_a + j1 - 1] - f + 2;
      if (l < 2 || f < 0 || f + l > n_a) bad = 2u;
      const int ll = l > 0 ? l : 0;
      s_base[s] = tot - f;
      s_pub[2 * s][0] = tot;
      s_pub[2 * s][1] = tot + max(0, min(ll, j0 - f));
      s_pub[2 * s + 1][0] = tot + min(ll, max(0, j1 - f));
      s_pub[2 * s + 1][1] = tot + ll;
      int* sp = &span_cl[((size_t)w * SMAX + s) * 4];
      __hip_atomic_store(to_global(&sp[0]), f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(to_global(&sp[1]), ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(to_global(&sp[2]), tot - f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tot += ll;
    }
    s_tot = tot;
    *L.s_nheavy = 0;
    if (tot > cap) bad = 2u;
    if (bad) __hip_atomic_store(to_global(err), bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (!PULL) {
  // every own entry, not only the two end columns (as hist_cluster_kernel): inside the grid
  // and inside [lo(j0), lo(j1 - 1)] of its row, or error 2 -- no push leaves its row's span
  if (!hc_own_in_bracket<KC, TH>(LO, S, n_a, j0, j1)) {
    __hip_atomic_store(to_global(err), 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (!barrier()) return -1;
  if (hc_failed(err, &s_stop)) return -1;
  if (tid < S) {
    const int s = tid;
    int n = 0, bad = 0;
    for (int w2 = 0; w2 < G; ++w2) {
      const int* sp = &span_cl[((size_t)w2 * SMAX + s) * 4];
      const int f = __hip_atomic_load(to_global(&sp[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int l = __hip_atomic_load(to_global(&sp[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (f < j1 && f + l > j0) {
        const int base = __hip_atomic_load(to_global(&sp[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n < kHcCand) s_cand[s][n] = HcCand{w2, f, l, base};
        else bad = 1;
        ++n;
      }
    }
    s_ncand[s] = n < kHcCand ? n : kHcCand;
    if (bad) {
      __hip_atomic_store(to_global(err), 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  const int total = s_tot;
  for (int q = tid; q < total; q += TH) Tacc[q] = 0.0;
  if (!barrier()) return -1;
  if (hc_failed(err, &s_stop)) return -1;
  }   // !PULL setup
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    if (PULL) break;
    const int d = j0 + tid + k * TH;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      int cf = 0, cn = 0;
      if (s < S && d < j1) {
        const int nc = s_ncand[s];
        for (int c = 0; c < nc; ++c) {
          const HcCand cd = s_cand[s][c];
          if (d >= cd.first && d < cd.first + cd.len) {
            if (cn == 0) cf = c;
            ++cn;
          }
        }
      }
      // a heavy destination: a wave-parallel entry, numbered in (k, s, thread) order so that
      // which destinations get the kHkHeavy entries (and so the summation order of the
      // others) is the same in every run
      const bool heavy = cn > kHkWaveCn;
      const unsigned long long bm = __ballot(heavy);
      if (lane == 0) L.s_wcnt[wid] = __popcll(bm);
      __syncthreads();
      int base = *L.s_nheavy;
      for (int q = 0; q < wid; ++q) base += L.s_wcnt[q];
      int tot = 0;
      for (int q = 0; q < TH / kWave; ++q) tot += L.s_wcnt[q];
      const int e = base + __popcll(bm & ((1ull << lane) - 1ull));
      int hi = kHkHeavy;
      if (heavy && e < kHkHeavy) {
        hi = e;
        L.s_heavy[e][0] = k;
        L.s_heavy[e][1] = s;
        L.s_heavy[e][2] = tid;
        L.s_heavy[e][3] = cf | (cn << 8);
      }
      __syncthreads();   // every wave read s_nheavy and s_wcnt before they change
      if (tid == 0) *L.s_nheavy = base + tot;   // (thread 0: wave 0, base = the running total)
      s_cinfo[(k * SMAX + s) * TH + tid] = hk_cinfo(cf, cn, hi);
    }
  }
  // lottery in registers with one column per thread at <= 8 waves (256 VGPRs); with two columns
  // per thread, or 16 waves (128 VGPRs), the registers hold the Krylov vectors
  // (the asset-grid solve: always, its vectors are one value per column)
  constexpr bool kLoReg = SMAX <= 8 && (KC == 1 || IID) && TH <= 512;
  int dreg[KC][kLoReg ? SMAX : 1];
  double wreg[KC][kLoReg ? SMAX : 1];
  if constexpr (kLoReg) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int j = j0 + tid + k * TH;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        const bool ok = s < S && j < j1;
        dreg[k][s] = ok ? LO[(size_t)s * n_a + j] : -1;
        wreg[k][s] = ok ? WL[(size_t)s * n_a + j] : 0.0;
      }
    }
  }
  const int v_base = lane < S ? s_base[lane] : 0;
  const int v_plo = lane < 2 * S ? s_pub[lane][0] : 0;
  const int v_phi = lane < 2 * S ? s_pub[lane][1] : 0;
  // IID: pi = P's (common) row in SGPRs
  double pi[IID ? SMAX : 1];
  if constexpr (IID) {
#pragma unroll
    for (int s = 0; s < SMAX; ++s) pi[s] = hk_uni(s_P[s]);
  }
  // the column index is re-materialised per phase through an empty asm: otherwise the
  // compiler hoists every point's address, hash and predicate out of the loop and keeps
  // them live across the gathers (hundreds of VGPRs of spills)
  const int jbase = j0 + tid;
  auto col = [&]() {
    int c = jbase;
    asm volatile("" : "+v"(c));
    return c;
  };

  // ---- the matvec pieces ----
  // push q's own sources into the LDS spans (np.add.at(T[s], lo, wlo q) and lo + 1)
  auto push = [&](const double (&q)[KC][NV]) {
    // lottery rows in groups whose loads (L2) are all in flight before the first atomic
    constexpr int PR = SMAX <= 8 ? SMAX : 4;
    const int jc = col();   // lottery addresses formed here, not hoisted (they spilled)
#pragma unroll
    for (int s0 = 0; s0 < SMAX; s0 += PR) {
      if (s0 < S) {
        int dd[KC][PR];
        double ww[KC][PR];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const int j = jc + k * TH;
#pragma unroll
          for (int u = 0; u < PR; ++u) {
            const int s = s0 + u;
            if constexpr (kLoReg) {
              dd[k][u] = s < SMAX ? dreg[k][s < SMAX ? s : 0] : -1;
              ww[k][u] = s < SMAX ? wreg[k][s < SMAX ? s : 0] : 0.0;
            } else {
              // unconditional loads at a clamped index (no exec-masked branch per load)
              const bool ok = s < S && j < j1;
              const int q = min(s, S - 1) * n_a + min(j, n_a - 1);
              const int dv = LO[q];
              const double wv = WL[q];
              dd[k][u] = ok ? dv : -1;
              ww[k][u] = ok ? wv : 0.0;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const bool act = j0 + tid + k * TH < j1;
#pragma unroll
          for (int u = 0; u < PR; ++u) {
            const int s = s0 + u;
            if (s < S) {   // wave-uniform
              const int d = dd[k][u];
              double qs;
              if constexpr (IID) qs = pi[s] * q[k][0];        // state s's share of the column's mass
              else qs = q[k][s];
              const double vlo = ww[k][u] * qs;          // np.add.at(T[s], lo, wlo q)
              const double vhi = (1.0 - ww[k][u]) * qs;  // np.add.at(T[s], lo + 1, (1 - wlo) q)
              const int ilo = __builtin_amdgcn_readlane(v_base, s) + d, ihi = ilo + 1;
              const int d0 = __builtin_amdgcn_readfirstlane(d);
              if (__all(act && d == d0)) {   // the whole wave on one destination (borrowing constraint)
                const double tl = wave_sum_lane63(vlo), th = wave_sum_lane63(vhi);
                if (lane == kWave - 1) {
                  atomicAdd(&Tacc[ilo], tl);
                  if (th != 0.0) atomicAdd(&Tacc[ihi], th);
                }
              } else if (act) {
                if (vlo != 0.0) atomicAdd(&Tacc[ilo], vlo);
                if (vhi != 0.0) atomicAdd(&Tacc[ihi], vhi);
              }
            }
          }
        }
      }
    }
    __syncthreads();
  };
  // publish the foreign parts of the spans write-through to slab `par`, re-zero them
  auto publish = [&](int par) {
    double* slab = slab_cl + ((size_t)w * 2 + par) * cap;
    for (int rr = 0; rr < 2 * S; ++rr) {
      const int lo = __builtin_amdgcn_readlane(v_plo, rr), hi = __builtin_amdgcn_readlane(v_phi, rr);
      for (int q = lo + tid; q < hi; q += TH) {
        store_f64_agent(&slab[q], Tacc[q]);
        Tacc[q] = 0.0;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  // gather the own destinations (ascending covering workgroup) and mix: Tq[k][s'] =
  // sum_s P[s, s'] T_s[d]
  // (IID: out[k][0] = sum_s T_s[d], s ascending, no mix)
  auto gather_mix = [&](int par, double (&out)[KC][NV]) {
    constexpr int GR = 4;
    double T[KC][SMAX];
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int s = 0; s < SMAX; ++s) T[k][s] = 0.0;
    bool more = false;
#pragma unroll
    for (int s0 = 0; s0 < SMAX; s0 += GR) {
      if (s0 < S) {
        double v0[KC][GR], v1[KC][GR];
        int oq[KC][GR];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const int d = j0 + tid + k * TH;
#pragma unroll
          for (int q = 0; q < GR; ++q) {
            const int s = s0 + q;
            v0[k][q] = 0.0;
            v1[k][q] = 0.0;
            oq[k][q] = -1;
            if (s < S) {
              const int ci = s_cinfo[(k * SMAX + s) * TH + tid], cf = hk_cf(ci), cn = hk_cn(ci);
              if (cn >= 1) {
                const HcCand c = s_cand[s][cf];
                if (c.w != w) v0[k][q] = load_f64_agent(&slab_cl[((size_t)c.w * 2 + par) * cap + c.base + d]);
                else oq[k][q] = c.base + d;
              }
              if (cn >= 2) {
                const HcCand c = s_cand[s][cf + 1];
                if (c.w != w) v1[k][q] = load_f64_agent(&slab_cl[((size_t)c.w * 2 + par) * cap + c.base + d]);
                else oq[k][q] = c.base + d;
              }
              more = more || (cn > 2 && hk_hi(ci) == kHkHeavy);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
          for (int q = 0; q < GR; ++q)
            if (oq[k][q] >= 0) {
              T[k][s0 + q] = Tacc[oq[k][q]];
              Tacc[oq[k][q]] = 0.0;
            }
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
          for (int q = 0; q < GR; ++q) T[k][s0 + q] = (v0[k][q] + v1[k][q]) + T[k][s0 + q];
      }
    }
    // heavy destinations (more than two covering spans): one wave per entry, candidate 2 + lane
    // in lane order, summed by the wave's fixed DPP tree; the owner adds the sum
    const int nh = min(*L.s_nheavy, kHkHeavy);   // block-uniform
    if (nh > 0) {
      // every entry of this wave loaded before the first sum (one round trip, not one per entry)
      constexpr int NW = TH / kWave, EPW = (kHkHeavy + NW - 1) / NW;
      double hx[EPW];
#pragma unroll
      for (int i = 0; i < EPW; ++i) {
        const int e = wid + i * NW;
        hx[i] = 0.0;
        if (e < nh) {   // wave-uniform
          const int ek = L.s_heavy[e][0], es = L.s_heavy[e][1], et = L.s_heavy[e][2], ec = L.s_heavy[e][3];
          const int c = 2 + lane;
          if (c < (ec >> 8)) hx[i] = hc_take(s_cand[es][(ec & 255) + c], w, j0 + et + ek * TH, par, cap, slab_cl, Tacc);
        }
      }
#pragma unroll
      for (int i = 0; i < EPW; ++i) {
        const int e = wid + i * NW;
        if (e < nh) {
          const double sum = wave_sum_lane63(hx[i]);
          if (lane == kWave - 1) L.s_hval[e] = sum;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
          if (s < S) {
            const int ci = s_cinfo[(k * SMAX + s) * TH + tid];
            if (hk_hi(ci) < kHkHeavy) T[k][s] += L.s_hval[hk_hi(ci)];
          }
    }
    if (__any(more)) {   // destinations with more than two covering spans and no wave entry
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const int d = j0 + tid + k * TH;
        double e2[SMAX], e3[SMAX];   // candidates 2 and 3 of every state, all in flight
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          e2[s] = 0.0;
          e3[s] = 0.0;
          if (s < S) {
            const int ci = s_cinfo[(k * SMAX + s) * TH + tid], cf = hk_cf(ci), cn = hk_cn(ci);
            if (cn > 2 && hk_hi(ci) == kHkHeavy) {
              e2[s] = hc_take(s_cand[s][cf + 2], w, d, par, cap, slab_cl, Tacc);
              if (cn > 3) e3[s] = hc_take(s_cand[s][cf + 3], w, d, par, cap, slab_cl, Tacc);
            }
          }
        }
#pragma unroll
        for (int s = 0; s < SMAX; ++s) T[k][s] += e2[s] + e3[s];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          if (s < S) {
            const int ci = s_cinfo[(k * SMAX + s) * TH + tid], cf = hk_cf(ci), cn = hk_cn(ci);
            if (hk_hi(ci) < kHkHeavy) continue;
            for (int c0 = 4; c0 < cn; c0 += 4) {   // (more than four spans and no wave entry: rare)
              double x[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int c = c0 + u;
                x[u] = 0.0;
                if (c < cn) x[u] = hc_take(s_cand[s][cf + c], w, d, par, cap, slab_cl, Tacc);
              }
              T[k][s] += ((x[0] + x[1]) + x[2]) + x[3];
            }
          }
        }
      }
    }
    if constexpr (IID) {
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        double acc = T[k][0];
#pragma unroll
        for (int s = 1; s < SMAX; ++s) acc += T[k][s];   // (rows past S are 0.0)
        out[k][0] = acc;
      }
    } else {
#pragma unroll
    for (int sp = 0; sp < SMAX; ++sp) {
      double pc[SMAX];
      asm volatile("" ::: "memory");   // one column of P at a time (else all of P is hoisted)
#pragma unroll
      for (int s = 0; s < SMAX; ++s) pc[s] = s_P[s * SMAX + sp];
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < SMAX; ++s) acc += pc[s] * T[k][s];
        out[k][sp] = acc;
      }
    }
    }   // !IID
  };
  // pull form: q of the own points staged in Qg (the exported entries write-through), one
  // cluster barrier, then every own destination pulls its sources (hist_pull.h)
  auto stage_q = [&](const double (&q)[KC][SMAX]) {
    const int jc = col();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int j = jc + k * TH;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < S && j < j1) {
          double* p = Qg + (size_t)s * n_a + j;
          if (j < s_ex[2 * s] || j >= s_ex[2 * s + 1]) store_f64_agent(p, q[k][s]);
          else *p = q[k][s];
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  auto w_at = [&](int s, int j) -> double {
    const double* p = WL + (size_t)s * n_a + j;
    return r.lottery_fresh ? load_f64_agent(p) : *p;
  };
  auto q_at = [&](int s, int j) -> double { return load_f64_agent(Qg + (size_t)s * n_a + j); };
  auto pull_mix = [&](double (&out)[KC][SMAX]) {
    const int jc = col();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      asm volatile("" ::: "memory");   // one column's loads at a time (else both are hoisted: spills)
      const int d = jc + k * TH;
      const bool valid = d < j1;
      double T[SMAX];
#pragma unroll
      for (int s = 0; s < SMAX; ++s) T[s] = 0.0;
      constexpr int GRP = SMAX <= 8 ? (KC == 1 ? (SMAX + 1) / 2 : 2) : 4;
#pragma unroll
      for (int s0 = 0; s0 < SMAX; s0 += GRP) {
        if (s0 >= S) break;   // wave-uniform
        asm volatile("" ::: "memory");
        int a0[GRP], a1[GRP], a2[GRP];
        double wv[GRP][4], qv[GRP][4];
#pragma unroll
        for (int u = 0; u < GRP; ++u) {
          const int sc = min(s0 + u, S - 1);
          const int* As = s_A + sc * aspan - (j0 - 1);
          // (clamped into the row: the loops below never leave it)
          a0[u] = valid ? min(max(As[d - 1], 0), n_a) : 0;
          a1[u] = valid ? min(max(As[d], a0[u]), n_a) : 0;
          a2[u] = valid ? min(max(As[d + 1], a1[u]), n_a) : 0;
          const int i0 = min(a1[u], n_a - 1), i1 = min(a1[u] + 1, n_a - 1);
          const int i2 = min(a0[u], n_a - 1), i3 = min(a0[u] + 1, n_a - 1);
          wv[u][0] = w_at(sc, i0); qv[u][0] = q_at(sc, i0);
          wv[u][1] = w_at(sc, i1); qv[u][1] = q_at(sc, i1);
          wv[u][2] = w_at(sc, i2); qv[u][2] = q_at(sc, i2);
          wv[u][3] = w_at(sc, i3); qv[u][3] = q_at(sc, i3);
        }
#pragma unroll
        for (int u = 0; u < GRP; ++u) {
          const int sr = s0 + u;
          if (sr < S) {   // wave-uniform
            const int n1c = a2[u] - a1[u], n0c = a1[u] - a0[u];
            const bool heavy = valid && (n1c + n0c) > kWave;
            double acc = 0.0;
            if (valid && !heavy) {
              if (n1c > 0) acc += wv[u][0] * qv[u][0];                    // np.add.at(T, lo, w q), ascending j
              if (n1c > 1) acc += wv[u][1] * qv[u][1];
              for (int j = a1[u] + 2; j < a2[u]; ++j) acc += w_at(sr, j) * q_at(sr, j);
              if (n0c > 0) acc += (1.0 - wv[u][2]) * qv[u][2];            // np.add.at(T, lo + 1, (1 - w) q)
              if (n0c > 1) acc += (1.0 - wv[u][3]) * qv[u][3];
              for (int j = a0[u] + 2; j < a1[u]; ++j) acc += (1.0 - w_at(sr, j)) * q_at(sr, j);
            }
            unsigned long long hm = __ballot(heavy);
            while (hm) {   // a destination with many sources: its whole wave, fixed order
              const int h = __builtin_ctzll(hm);
              hm &= hm - 1ull;
              const int b0 = __builtin_amdgcn_readlane(a0[u], h), b1 = __builtin_amdgcn_readlane(a1[u], h),
                        b2 = __builtin_amdgcn_readlane(a2[u], h);
              double pa = 0.0, pb = 0.0;
              for (int j = b1 + lane; j < b2; j += kWave) pa += w_at(sr, j) * q_at(sr, j);
              for (int j = b0 + lane; j < b1; j += kWave) pb += (1.0 - w_at(sr, j)) * q_at(sr, j);
              const double ta = wave_sum_lane63(pa), tb = wave_sum_lane63(pb);
              const double tot = __shfl(ta, kWave - 1, kWave) + __shfl(tb, kWave - 1, kWave);
              if (lane == h) acc = tot;
            }
            T[sr] = acc;
          }
        }
      }
#pragma unroll
      for (int sp = 0; sp < SMAX; ++sp) {
        double pc[SMAX];
        asm volatile("" ::: "memory");   // one column of P at a time
#pragma unroll
        for (int s = 0; s < SMAX; ++s) pc[s] = s_P[s * SMAX + sp];
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < SMAX; ++s) acc += pc[s] * T[s];
        out[k][sp] = acc;
      }
    }
  };
  // one matvec: out = T q (the cluster exchange in the middle)
  auto matvec = [&](const double (&q)[KC][NV], double (&out)[KC][NV]) -> bool {
    if constexpr (PULL) {
      HK_PH(5);
      stage_q(q);
      HK_PH(1);
      if (!barrier()) return false;
      HK_PH(2);
      pull_mix(out);
      HK_PH(3);
      return true;
    }
    HK_PH(5);
    push(q);
    HK_PH(0);
    const int par = (int)((nb + 1) & 1);
    publish(par);
    HK_PH(1);
    if (!barrier()) return false;
    HK_PH(2);
    gather_mix(par, out);
    HK_PH(3);
    return true;
  };
  // cluster-wide reduction of nv per-thread partials into s_res (hist_cluster.h's protocol);
  // prefetch(): loads the step after the reduction needs, in flight across the sweep.
  // hc_reduce's steps written out: through hc_reduce, with prefetch handed on as its hook, the
  // two-column push kernel (hist_bicg_kernel<8, 2, 512, false>) spilled 4 bytes per lane more
  auto reduce = [&](double (&vals)[kHcRed], int nv, unsigned kmax, auto&& prefetch) -> bool {
    HK_PH(5);
    hc_wave_parts(vals, nv, kmax, s_part);
    __syncthreads();
    ++ne;
    const unsigned long long tag = hc_red_tag(ne);
    unsigned long long* slot = hc_red_slot(gran, G, ne);
    hc_store_granules<TH>(slot, w, tag, nv, kmax, s_part);
    prefetch();
    if (wid == 0) hc_sweep(slot, G, tag, nv, kmax, s_res, &s_flag, err);
    __syncthreads();
    HK_PH(4);
    return s_flag != 0;
  };
  // one matvec out = T q whose cluster barrier also carries a reduction of nv values computed
  // before it (pipelined BiCGSTAB): the granules are stored before the publish's store drain,
  // so every workgroup's are in memory once the barrier has passed; the last wave reads them
  // while the other waves gather, and s_res is valid on return
  // do_push(): the push of the matvec input (ends with a workgroup barrier)
  auto matvec_rp = [&](auto&& do_push, double (&out)[KC][NV], const double* vals, int nv, unsigned kmax) -> bool {
    HK_PH(5);
    hc_wave_parts(vals, nv, kmax, s_part);
    do_push();   // ends with a workgroup barrier: s_part complete
    HK_PH(0);
    ++ne;
    const unsigned long long tag = hc_red_tag(ne);
    unsigned long long* slot = hc_red_slot(gran, G, ne);
    hc_store_granules<TH>(slot, w, tag, nv, kmax, s_part);
    const int par = (int)((nb + 1) & 1);
    publish(par);   // every thread's s_waitcnt vmcnt(0): slabs and granules drained
    HK_PH(1);
    if (!barrier()) return false;
    HK_PH(2);
    // the sweep by the last wave: with one column per thread its lanes own no columns whenever
    // a workgroup has <= TH - 64 of them (G >= 23 at N_a = 10 000), so it overlaps the gather
    if (wid == TH / kWave - 1) hc_sweep(slot, G, tag, nv, kmax, s_res, L.s_rok, err);
    gather_mix(par, out);
    __syncthreads();
    HK_PH(3);
    return *L.s_rok != 0;
  };
  auto matvec_r = [&](const double (&q)[KC][NV], double (&out)[KC][NV], const double* vals, int nv,
                      unsigned kmax) -> bool { return matvec_rp([&] { push(q); }, out, vals, nv, kmax); };
  if constexpr (IID) {
    int mv = 0;                 // matvecs
    auto col_act = [&](int jc, bool (&act)[KC]) {   // (as the general loop's below)
#pragma unroll
      for (int k = 0; k < KC; ++k) act[k] = jc + k * TH < j1;
    };
    // ---- BiCGSTAB on (I - M) mu = 0: the general loop below with one unknown per column, every
    //      vector in registers; the same stopping, stall, restart and breakdown rules ----
    // TWIN of the general loop: the stop poll, the convergence / max_iter tests, the stall rule
    // (kHkStall, 0.9 best), the breakdown tests on alpha, omega, beta and rho and the rescale to the
    // start's total are copied from it line for line.  A change to any of them there is made here
    // too (tests/test_gpu_iid_cells.py holds the two to each other only within the search bounds).
    double pimax = 0.0;
#pragma unroll
    for (int s = 0; s < SMAX; ++s)
      if (s < S) pimax = fmax(pimax, pi[s]);
    const double tol = r.tol / pimax;
    double xv[KC][1], rv[KC][1], pv[KC][1], tv[KC][1], vv[KC], uv[KC];
    double part[kHcRed];
    bool restart = true, first = true;
    double rho = 0.0, total0 = 0.0;
    bool act[KC];
    double pu = 0.0;   // FUSEA: this thread's part of <u, p>
    unsigned seed = 0;
    auto rh_at = [&](int jc, int k) { return hk_rhat((unsigned)(jc + k * TH) + seed * 0x5BD1E995u); };
    double best = __builtin_inf();
    int mv_best = 0;
    // X[s][j] = pi_s m[j] of the own columns
    auto store_x = [&](int jc, const double (&m)[KC]) {
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (jc + k * TH < j1) {
#pragma unroll
          for (int s = 0; s < SMAX; ++s)
            if (s < S) X[(size_t)s * n_a + jc + k * TH] = pi[s] * m[k];
        }
    };
    {   // mu0[j] = sum_s X[s][j], s ascending
      const int jc = col();
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        double xs[SMAX];
#pragma unroll
        for (int s = 0; s < SMAX; ++s) xs[s] = X[min(s, S - 1) * n_a + min(jc + k * TH, n_a - 1)];
        double acc = xs[0];
#pragma unroll
        for (int s = 1; s < SMAX; ++s)
          if (s < S) acc += xs[s];
        xv[k][0] = jc + k * TH < j1 ? acc : 0.0;
      }
    }
    HK_PH(-1);
    while (true) {
      if (restart) {
        // true residual of mu: tv = M mu, rv = M mu - mu
        if (!matvec(xv, tv)) return -1;
        ++mv;
        const int jc = col();
        col_act(jc, act);
        double rr = 0.0, rm = 0.0, xs = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          rv[k][0] = tv[k][0] - xv[k][0];
          if (act[k]) {
            rr += rh_at(jc, k) * rv[k][0];
            rm = nan_max(rm, fabs(rv[k][0]));
            xs += xv[k][0];
          }
        }
        part[0] = rr;
        part[1] = rm;
        part[2] = xs;
        if (!reduce(part, 3, 2u, [] {})) return -1;
        rho = s_res[0];
        if (mv == 1) total0 = s_res[2];   // the starting mass's total
        if (s_res[1] < tol || mv >= r.max_iter) {   // converged: pi (x) M mu, rescaled to the start's total
          const double scale = total0 / s_res[2];
          double m[KC];
#pragma unroll
          for (int k = 0; k < KC; ++k) m[k] = mv == 1 ? tv[k][0] : tv[k][0] * scale;
          store_x(jc, m);
          break;
        }
        double pun = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          pv[k][0] = rv[k][0];
          uv[k] = 0.0;
          if constexpr (FUSEA) {   // u = rh - M^T rh of the own columns (their own lottery only)
            if (act[k]) {
              double tr = 0.0;
#pragma unroll
              for (int s = 0; s < SMAX; ++s)
                if (s < S) {
                  const unsigned q = (unsigned)dreg[k][s] + seed * 0x5BD1E995u;
                  tr += pi[s] * (wreg[k][s] * hk_rhat(q) + (1.0 - wreg[k][s]) * hk_rhat(q + 1u));
                }
              uv[k] = rh_at(jc, k) - tr;
              pun += uv[k] * pv[k][0];
            }
          }
        }
        pu = pun;
        restart = false;
        first = true;
      }
      // rebalancing stop request, polled every 8th iteration (see the general loop)
      if (r.stop_ctr != nullptr && tid == 0 && ((mv >> 1) & 7) == 0)
        s_stop = __hip_atomic_load((const unsigned*)r.stop_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= r.stop_at;
      int jc = col();
      col_act(jc, act);
      if constexpr (FUSEA) {   // <u, p> = <rh, v> and max|r| ride on the matvec's barrier
        double rm = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (act[k]) rm = nan_max(rm, fabs(rv[k][0]));
        part[0] = pu;
        part[1] = (r.stop_ctr != nullptr && tid == 0 && s_stop) ? kHkStopSentinel : rm;
        if (!matvec_r(pv, tv, part, 2, 2u)) return -1;
        ++mv;
#pragma unroll
        for (int k = 0; k < KC; ++k) vv[k] = pv[k][0] - tv[k][0];
      } else {
        if (!matvec(pv, tv)) return -1;
        ++mv;
        jc = col();
        col_act(jc, act);
        double rvv = 0.0, rm = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          vv[k] = pv[k][0] - tv[k][0];
          if (act[k]) {
            rvv += rh_at(jc, k) * vv[k];
            rm = nan_max(rm, fabs(rv[k][0]));
          }
        }
        part[0] = rvv;
        part[1] = (r.stop_ctr != nullptr && tid == 0 && s_stop) ? kHkStopSentinel : rm;
        if (!reduce(part, 2, 2u, [] {})) return -1;
      }
      if (s_res[1] >= kHkStopSentinel) {   // every workgroup reads the same max: X = pi (x) mu, a valid iterate
        double m[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k) m[k] = xv[k][0];
        store_x(col(), m);
        return -(2 + mv);
      }
      if ((!first && s_res[1] < tol) || mv >= r.max_iter) {   // recursive residual converged: verify
        restart = true;
        continue;
      }
      if (first || s_res[1] < 0.9 * best) {
        best = first ? __builtin_inf() : s_res[1];
        mv_best = mv;
      } else if (mv - mv_best > kHkStall) {   // stagnation: the next shadow residual
        ++seed;
        best = __builtin_inf();
        restart = true;
        continue;
      }
      first = false;
      const double alpha = rho / s_res[0];
      if (!(fabs(alpha) < 1e300)) {   // breakdown or NaN: restart from the true residual
        restart = true;
        continue;
      }
      // x += alpha p; s = r - alpha v (in rv); t = s - M s (in tv)
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        xv[k][0] += alpha * pv[k][0];
        rv[k][0] -= alpha * vv[k];
      }
      if (!matvec(rv, tv)) return -1;
      ++mv;
      jc = col();
      col_act(jc, act);
      double ts = 0.0, tt = 0.0, rs = 0.0, rt = 0.0, sm = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        tv[k][0] = rv[k][0] - tv[k][0];
        if (act[k]) {
          const double h = rh_at(jc, k);
          ts += tv[k][0] * rv[k][0];
          tt += tv[k][0] * tv[k][0];
          rs += h * rv[k][0];
          rt += h * tv[k][0];
          sm = nan_max(sm, fabs(rv[k][0]));
        }
      }
      part[0] = ts;
      part[1] = tt;
      part[2] = rs;
      part[3] = rt;
      part[4] = sm;
      if (!reduce(part, 5, 16u, [] {})) return -1;
      double omega = (s_res[4] < tol) ? 0.0 : s_res[0] / s_res[1];
      if (!(fabs(omega) < 1e300)) omega = 0.0;
      if (omega == 0.0) {   // s already below tol (x + alpha p is the answer), or <t, t> = 0: verify
        restart = true;
        continue;
      }
      const double rho2 = s_res[2] - omega * s_res[3];
      const double beta = (rho2 / rho) * (alpha / omega);
      rho = rho2;
      // x += omega s; r = s - omega t; p = r + beta (p - omega v)
      double pun = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        xv[k][0] += omega * rv[k][0];
        rv[k][0] = rv[k][0] - omega * tv[k][0];
        pv[k][0] = rv[k][0] + beta * (pv[k][0] - omega * vv[k]);
        if constexpr (FUSEA) pun += uv[k] * pv[k][0];
      }
      pu = pun;
      if (!(fabs(beta) < 1e300) || rho == 0.0) restart = true;
    }
    HK_PH_REPORT(mv);
    return mv;
  } else {
  // ---- BiCGSTAB ----
  // (TWIN: the IID block above repeats this loop's stop poll, convergence, stall, breakdown and
  // rescale rules for one unknown per column; change them in both places)
  // registers: r (then s), p, and the matvec result; v waits in LDS (behind the spans) and
  // p in the HBM scratch row across the second matvec, whose gather needs the registers
  double rv[KC][SMAX], pv[KC][SMAX], tv[KC][SMAX];
  // v: in LDS behind the spans when it fits (SMAX <= 8), else a per-workgroup HBM block of
  // the same [KC][SMAX][TH] layout (behind the p rows of the scratch)
  double* Vl = kVlds ? Tacc + cap : (double*)r.Vg;
  double* Pg = (double*)r.Pg;
  auto vidx = [&](int k, int s) { return (k * SMAX + s) * TH + tid; };
  double part[kHcRed];
  const double tol = r.tol;
  int mv = 0;                 // matvecs
  bool restart = true, first = true;
  double rho = 0.0, total0 = 0.0;
  auto own = [&](int jc, int k, int s) { return s < S && jc + k * TH < j1; };
  // In the iteration's phases a thread's column is active or not as a whole: one predicate (one
  // exec region) per column around its guarded points, not one per point; the per-thread partial
  // sums keep their (column, state) order, and an inactive column's entries stay 0.0
  auto col_act = [&](int jc, bool (&act)[KC]) {
#pragma unroll
    for (int k = 0; k < KC; ++k) act[k] = jc + k * TH < j1;
  };
  bool act[KC];
  unsigned seed = 0;   // shadow-residual choice; a stagnating solve restarts with the next one
  auto rh_at = [&](int jc, int k, int s) { return hk_rhat((unsigned)(s * n_a + jc + k * TH) + seed * 0x5BD1E995u); };
  double best = __builtin_inf();   // best recursive max|r| since the last restart, and when
  int mv_best = 0;
  auto gidx = [&](int jc, int k, int s) { return (size_t)s * n_a + jc + k * TH; };
  // FUSEA (one column per thread, the resident search): alpha's reduction rides on the first
  // matvec's cluster barrier.  <rh, v> = <rh, A p> = <A^T rh, p> with A = I - T, and
  // u = A^T rh is fixed for a solve (a new shadow residual recomputes it): its own points sit in
  // the Qg rows, and <u, p> is formed when p is, before the matvec.  One cluster reduction per
  // iteration instead of two; the same recurrence otherwise.
  //   (T^T y)[s][j] = sum_s' P[s, s'] (wlo y[s'][lo] + (1 - wlo) y[s'][lo + 1])
  double* Ug = (double*)r.Qg;
  double pu = 0.0;   // this thread's part of <u, p>
  auto make_u = [&]() {   // u of the own points -> Ug; pu = <u, p> with p = r
    if constexpr (FUSEA) {
      const int jc = col();
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          if (own(jc, k, s)) {
            int d;
            double wl;
            if constexpr (kLoReg) {
              d = dreg[k][s];
              wl = wreg[k][s];
            } else {   // (two columns per thread: the own lottery from L2, once per solve)
              d = LO[gidx(jc, k, s)];
              wl = WL[gidx(jc, k, s)];
            }
            double tr = 0.0;
            for (int sp = 0; sp < S; ++sp) {
              const unsigned q = (unsigned)(sp * n_a + d) + seed * 0x5BD1E995u;
              tr += s_P[s * SMAX + sp] * (wl * hk_rhat(q) + (1.0 - wl) * hk_rhat(q + 1u));
            }
            const double u = rh_at(jc, k, s) - tr;
            Ug[gidx(jc, k, s)] = u;
            acc += u * pv[k][s];
          }
        }
      pu = acc;
    }
  };
  // FUSEA with two columns per thread: u of the own points is read back when the new p is formed
  // (AIY_FUSEA_KC2 = 1: prefetched with x and p across the second reduction; 2: loaded after it,
  // beside the new p, so it holds no registers across the reduction)
#ifndef AIY_FUSEA_KC2
#define AIY_FUSEA_KC2 0
#endif
  constexpr bool kUqPre = KC == 1 || AIY_FUSEA_KC2 == 1;
  HK_PH(-1);
  while (true) {
    if (restart) {
      // true residual of x: pv = x, tv = T x, rv = T x - x
      int jc = col();
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          const double xv = X[min(s, S - 1) * n_a + min(jc + k * TH, n_a - 1)];
          pv[k][s] = own(jc, k, s) ? xv : 0.0;
        }
      if (!matvec(pv, tv)) return -1;
      ++mv;
      jc = col();
      double rr = 0.0, rm = 0.0, xs = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          rv[k][s] = tv[k][s] - pv[k][s];
          if (own(jc, k, s)) {
            rr += rh_at(jc, k, s) * rv[k][s];
            rm = nan_max(rm, fabs(rv[k][s]));
            xs += pv[k][s];
          }
        }
      part[0] = rr;
      part[1] = rm;
      part[2] = xs;
      if (!reduce(part, 3, 2u, [] {})) return -1;
      rho = s_res[0];
      if (mv == 1) total0 = s_res[2];   // the starting mass's total
      if (s_res[1] < tol || mv >= r.max_iter) {   // converged (np.max(...) < tol: NaN never is)
        // T x rescaled to the start's total: the residual test cannot see the scale of x,
        // and near a breakdown (huge alpha) rounding can move sum(x) away from it; T
        // preserves totals, as the plain iteration does
        const double scale = total0 / s_res[2];
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
          for (int s = 0; s < SMAX; ++s)
            if (own(jc, k, s)) X[gidx(jc, k, s)] = mv == 1 ? tv[k][s] : tv[k][s] * scale;
        break;
      }
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) pv[k][s] = rv[k][s];
      make_u();
      restart = false;
      first = true;
    }
    // v = p - T p (to LDS); alpha = rho / <rh, v>; the previous step's max|r| rides along.
    // r waits in v's slot during this matvec (only p and the result stay in registers)
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int s = 0; s < SMAX; ++s) Vl[vidx(k, s)] = rv[k][s];
    // rebalancing stop request: polled every 8th iteration by thread 0 into LDS (the matvec's
    // barriers make it visible; the partial below carries it to every workgroup).  mv grows by
    // 2 per iteration and is odd after a restart's true-residual matvec, so the iteration
    // number is mv >> 1
    if (r.stop_ctr != nullptr && tid == 0 && ((mv >> 1) & 7) == 0)
      s_stop = __hip_atomic_load((const unsigned*)r.stop_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= r.stop_at;
    double xq[KC][SMAX];   // x of the own points, for x += alpha p
    int jc;
    if constexpr (FUSEA) {
      // <u, p> and max|r| ride on this matvec's barrier (the stop request as a sentinel on the
      // max, which no residual of a mass vector reaches); x's loads in flight across it (one
      // column per thread; with two, x is loaded after the matvec: its registers are full)
      jc = col();
      col_act(jc, act);
      double rm = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        if (act[k]) {
#pragma unroll
          for (int s = 0; s < SMAX; ++s)
            if (s < S) rm = nan_max(rm, fabs(Vl[vidx(k, s)]));
        }
        if constexpr (KC == 1) {
#pragma unroll
          for (int s = 0; s < SMAX; ++s) xq[k][s] = X[min(s, S - 1) * n_a + min(jc + k * TH, n_a - 1)];
        }
      }
      part[0] = pu;
      part[1] = (r.stop_ctr != nullptr && tid == 0 && s_stop) ? kHkStopSentinel : rm;
      if (!matvec_r(pv, tv, part, 2, 2u)) return -1;
      ++mv;
      jc = col();
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          const double v = pv[k][s] - tv[k][s];
          rv[k][s] = Vl[vidx(k, s)];
          Vl[vidx(k, s)] = v;
          if constexpr (KC > 1) xq[k][s] = X[min(s, S - 1) * n_a + min(jc + k * TH, n_a - 1)];
        }
    } else {
      if (!matvec(pv, tv)) return -1;
      ++mv;
      jc = col();
      col_act(jc, act);
      double rvv = 0.0, rm = 0.0;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          tv[k][s] = pv[k][s] - tv[k][s];   // v
          rv[k][s] = Vl[vidx(k, s)];
          Vl[vidx(k, s)] = tv[k][s];
        }
        if (act[k]) {
#pragma unroll
          for (int s = 0; s < SMAX; ++s)
            if (s < S) {
              rvv += rh_at(jc, k, s) * tv[k][s];
              rm = nan_max(rm, fabs(rv[k][s]));
            }
        }
      }
      part[0] = rvv;
      // the stop request rides on the max|r| partial as a sentinel no residual of a mass vector
      // reaches (the cluster max is the same in every workgroup)
      part[1] = (r.stop_ctr != nullptr && tid == 0 && s_stop) ? kHkStopSentinel : rm;
      if (!reduce(part, 2, 2u, [&] {
            const int jq = col();
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
              for (int s = 0; s < SMAX; ++s) xq[k][s] = X[min(s, S - 1) * n_a + min(jq + k * TH, n_a - 1)];
          }))
        return -1;
    }
    if (s_res[1] >= kHkStopSentinel) return -(2 + mv);   // every workgroup reads the same max
    if ((!first && s_res[1] < tol) || mv >= r.max_iter) {   // recursive residual converged: verify
      restart = true;
      continue;
    }
    // stagnation (BiCGSTAB can stall for a particular shadow residual: one Table II cell
    // sat at max|r| ~ 6e-5 with the first hash): no 10 % gain in kHkStall matvecs ->
    // restart from the true residual with the next shadow residual
    if (first || s_res[1] < 0.9 * best) {
      best = first ? __builtin_inf() : s_res[1];
      mv_best = mv;
    } else if (mv - mv_best > kHkStall) {
      ++seed;
      best = __builtin_inf();
      restart = true;
      continue;
    }
    first = false;
    const double alpha = rho / s_res[0];
    if (!(fabs(alpha) < 1e300)) {   // breakdown (<rh, v> = 0) or NaN: restart from the true residual
      restart = true;
      continue;
    }
    // x += alpha p; p -> HBM scratch; s = r - alpha v (in rv); t = s - T s (in tv)
    jc = col();
    col_act(jc, act);
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      if (act[k]) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
          if (s < S) {
            const int g = s * n_a + jc + k * TH;
            X[g] = xq[k][s] + alpha * pv[k][s];
            Pg[g] = pv[k][s];
          }
      }
#pragma unroll
      for (int s = 0; s < SMAX; ++s) rv[k][s] -= alpha * Vl[vidx(k, s)];
    }
    if (!matvec(rv, tv)) return -1;
    ++mv;
    jc = col();
    col_act(jc, act);
    double ts = 0.0, tt = 0.0, rs = 0.0, rt = 0.0, sm = 0.0;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
#pragma unroll
      for (int s = 0; s < SMAX; ++s) tv[k][s] = rv[k][s] - tv[k][s];
      if (act[k]) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
          if (s < S) {
            const double h = rh_at(jc, k, s);
            ts += tv[k][s] * rv[k][s];
            tt += tv[k][s] * tv[k][s];
            rs += h * rv[k][s];
            rt += h * tv[k][s];
            sm = nan_max(sm, fabs(rv[k][s]));
          }
      }
    }
    part[0] = ts;
    part[1] = tt;
    part[2] = rs;
    part[3] = rt;
    part[4] = sm;
    double pq[KC][SMAX];   // x and p of the own points, for x += omega s and the new p
    double uq[FUSEA && kUqPre ? KC : 1][SMAX];   // FUSEA: u of the own points, for <u, p> of the new p
    if (!reduce(part, 5, 16u, [&] {
          const int jq = col();
#pragma unroll
          for (int k = 0; k < KC; ++k)
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
              const int g = min(s, S - 1) * n_a + min(jq + k * TH, n_a - 1);
              xq[k][s] = X[g];
              pq[k][s] = Pg[g];
              if constexpr (FUSEA && kUqPre) uq[k][s] = Ug[g];
            }
        }))
      return -1;
    double omega = (s_res[4] < tol) ? 0.0 : s_res[0] / s_res[1];
    if (!(fabs(omega) < 1e300)) omega = 0.0;
    if (omega == 0.0) {   // s already below tol (x + alpha p is the answer), or <t, t> = 0: verify
      restart = true;
      continue;
    }
    const double rho2 = s_res[2] - omega * s_res[3];
    const double beta = (rho2 / rho) * (alpha / omega);
    rho = rho2;
    // x += omega s; r = s - omega t; p = r + beta (p - omega v)
    jc = col();
    col_act(jc, act);
    double pun = 0.0;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      if (act[k]) {
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
          if (s < S) X[s * n_a + jc + k * TH] = xq[k][s] + omega * rv[k][s];
      }
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        const double pold = (act[k] && s < S) ? pq[k][s] : 0.0;
        rv[k][s] = rv[k][s] - omega * tv[k][s];
        pv[k][s] = rv[k][s] + beta * (pold - omega * Vl[vidx(k, s)]);
      }
      if constexpr (FUSEA && kUqPre) {
        if (act[k]) {
#pragma unroll
          for (int s = 0; s < SMAX; ++s)
            if (s < S) pun += uq[k][s] * pv[k][s];
        }
      }
    }
    if constexpr (FUSEA && !kUqPre) {   // u read back beside the new p (every load before the first use)
      double ul[KC][SMAX];
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) ul[k][s] = Ug[min(s, S - 1) * n_a + min(jc + k * TH, n_a - 1)];
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
          if (own(jc, k, s)) pun += ul[k][s] * pv[k][s];
    }
    pu = pun;
    if (!(fabs(beta) < 1e300) || rho == 0.0) restart = true;
  }
  HK_PH_REPORT(mv);
  return mv;
  }   // !IID
}

// The arguments of a non-kernel function arrive in VGPRs, where the compiler must take them for
// per-lane values: every address built from them is vector arithmetic (a v_mul_lo_u32 per row
// index, a 64-bit vector add per access), every `s < S` an exec-mask region, and the pointers
// hold ~30 VGPRs that the Krylov vectors then spill around.  They are the same in every lane:
// read into SGPRs once at entry.
__device__ __forceinline__ int hk_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
template <class T>
__device__ __forceinline__ gptr<T> hk_uni(gptr<T> p) {
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return (gptr<T>)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ HkArgs hk_uniform_args(const HkArgs& a) {
  HkArgs u;
  u.G = hk_uni(a.G); u.S = hk_uni(a.S); u.n_a = hk_uni(a.n_a); u.cap = hk_uni(a.cap);
  u.w = hk_uni(a.w); u.j0 = hk_uni(a.j0); u.j1 = hk_uni(a.j1);
  u.LO = hk_uni(a.LO); u.WL = hk_uni(a.WL); u.X = hk_uni(a.X); u.Pg = hk_uni(a.Pg); u.Vg = hk_uni(a.Vg);
  u.slab_cl = hk_uni(a.slab_cl); u.span_cl = hk_uni(a.span_cl); u.ctr = hk_uni(a.ctr); u.gran = hk_uni(a.gran);
  u.Pc = hk_uni(a.Pc);
  u.tol = hk_uni(a.tol);
  u.max_iter = hk_uni(a.max_iter);
  u.err = hk_uni(a.err);
  u.stop_ctr = hk_uni(a.stop_ctr);
  u.stop_at = (unsigned)hk_uni((int)a.stop_at);
  u.Qg = hk_uni(a.Qg); u.Ainv = hk_uni(a.Ainv);
  u.lottery_fresh = hk_uni((int)a.lottery_fresh) != 0;
  u.dyn_lds = (unsigned)hk_uni((int)a.dyn_lds);
  return u;
}

// hk_solve as its own (not inlined) function with its LDS declared here: a caller that
// carries a lot of live state of its own (ge_resident.hip's search loop) would otherwise
// force the solve's registers into scratch; the call costs a few register saves per
// solve.  The span buffer / v share the caller's dynamic LDS (HkArgs::dyn_lds).
// Its LDS arrays are one object per (SMAX, KC, TH): the general and the asset-grid (IID) solve of
// one kernel are two functions, each with its own register allocation, that never run at the
// same time and share it (declared inside, each brought its own: +20 KB at two columns per
// thread, taken from the span buffer).
template <int SMAX, int KC, int TH>
struct HkIsoLds {
  int s_base[SMAX];
  int s_pub[2 * SMAX][2];
  int s_tot;
  HcCand s_cand[SMAX][kHcCand];
  int s_ncand[SMAX];
  unsigned short s_cinfo[KC * SMAX * TH];
  double s_P[SMAX * SMAX];
  double s_part[kHcRed][TH / kWave];
  double s_res[kHcRed];
  int s_flag, s_stop;
  int s_ex[2 * SMAX];
  int s_nheavy, s_heavy[kHkHeavy][4], s_rok, s_wcnt[TH / kWave];
  double s_hval[kHkHeavy];
};
template <int SMAX, int KC, int TH>
__shared__ HkIsoLds<SMAX, KC, TH> hk_iso_lds;
template <int SMAX, int KC, int TH, bool PULL = false, bool FUSEA = false, int SC = 0, bool IID = false>
__device__ __noinline__ int hk_solve_isolated(HkArgs a, unsigned* nb_io, unsigned* ne_io);
// the same body inlined into the caller (the pull form spilled more as a separate function)
template <int SMAX, int KC, int TH, bool PULL = false, bool FUSEA = false, int SC = 0>
__device__ __forceinline__ int hk_solve_inlined(HkArgs a, unsigned* nb_io, unsigned* ne_io) {
  extern __shared__ double hk_dyn_in[];
  __shared__ int s_base[SMAX];
  __shared__ int s_pub[2 * SMAX][2];
  __shared__ int s_tot;
  __shared__ HcCand s_cand[SMAX][kHcCand];
  __shared__ int s_ncand[SMAX];
  __shared__ unsigned short s_cinfo[PULL ? 1 : KC * SMAX * TH];
  __shared__ double s_P[SMAX * SMAX];
  __shared__ double s_part[kHcRed][TH / kWave];
  __shared__ double s_res[kHcRed];
  __shared__ int s_flag, s_stop;
  __shared__ int s_ex[2 * SMAX];
  __shared__ int s_nheavy, s_heavy[kHkHeavy][4], s_rok, s_wcnt[TH / kWave];
  __shared__ double s_hval[kHkHeavy];
  HkShared<SMAX, KC, TH> L{hk_dyn_in, s_base, s_pub, &s_tot, s_cand, s_ncand, s_cinfo, s_P, s_part, s_res,
                                 &s_flag, &s_stop, s_ex, &s_nheavy, s_wcnt, s_heavy, s_hval, &s_rok};
  unsigned nb = *nb_io, ne = *ne_io;
  const int mv = hk_solve<SMAX, KC, TH, PULL, FUSEA, SC>(a, L, nb, ne);
  *nb_io = nb;
  *ne_io = ne;
  return mv;
}
template <int SMAX, int KC, int TH, bool PULL, bool FUSEA, int SC, bool IID>
__device__ __noinline__ int hk_solve_isolated(HkArgs a, unsigned* nb_io, unsigned* ne_io) {
  // the caller's dynamic LDS by address (wave-uniform, one SGPR), typed LDS so that every access
  // stays a ds_ instruction
  double* hk_dyn = (double*)(lptr<double>)(size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)a.dyn_lds);
  HkIsoLds<SMAX, KC, TH>& S_ = hk_iso_lds<SMAX, KC, TH>;
  HkShared<SMAX, KC, TH> L{hk_dyn, S_.s_base, S_.s_pub, &S_.s_tot, S_.s_cand, S_.s_ncand, S_.s_cinfo, S_.s_P,
                           S_.s_part, S_.s_res, &S_.s_flag, &S_.s_stop, S_.s_ex, &S_.s_nheavy, S_.s_wcnt,
                           S_.s_heavy, S_.s_hval, &S_.s_rok};
  unsigned nb = *nb_io, ne = *ne_io;
  const int mv = hk_solve<SMAX, KC, TH, PULL, FUSEA, SC, IID>(hk_uniform_args(a), L, nb, ne);
  *nb_io = nb;
  *ne_io = ne;
  return mv;
}

}  // namespace aiy
