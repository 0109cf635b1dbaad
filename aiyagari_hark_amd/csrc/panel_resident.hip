// Persistent ("resident") Monte Carlo panel: a whole block of periods of
// Market.make_history in ONE launch (same per-period
// semantics as sim_period_kernel in panel.hip).
//
// Geometry: one workgroup of TH threads per CU (grid <= CU count, all resident; checked
// by the cooperative launch), each owning a contiguous, even-aligned slice of the
// agents.  When the slice fits (<= ~16k agents per CU, i.e. ~4M agents on MI355X) its
// assets and labour states live in LDS for the whole launch, so per period the agents
// cost no HBM traffic at all; otherwise they stream from HBM (same code).
//
// One period, per workgroup:
//   1. lookups: every lane carries NA agents (i = base + k TH + lane: consecutive lanes,
//      consecutive agents) through m = R a + W l, c = cFunc[4 l + 2 Mrkv + 1](m, M)
//      (merged-table lookup, panel_common.h), a = m - c in lock step, so a whole slice is
//      in flight in one or two passes; partial sum of a in fixed order;
//   2. publish: lane 0 stores the workgroup partial as two tagged 8-byte granules;
//   3. next period's labour draws (Philox + inverse CDF, AS:1253-1254) do not depend on
//      prices, so they run while the partials travel;
//   4. wave 0 sweeps every workgroup's granules (relaxed agent-scope loads, s_sleep,
//      wall-clock timeout), sums them in fixed order and runs calc_R_and_W
//      (AS:1867-1894) -- every workgroup computes the same prices, no broadcast hop.
// Granule slots alternate by period parity and are tagged with the period index
// within the launch; they are zeroed by a memset ahead of each launch.  Partial sums
// are combined in fixed order, so histories are reproducible run to run (they differ
// from the per-period kernel's only in the summation order of the mean, ~1e-16
// relative).
#include "common.h"
#include "internal.h"
#include "panel_common.h"

#include <algorithm>

namespace aiy {

typedef double st_d2 __attribute__((ext_vector_type(2)));

constexpr int kResMaxBlocks = 256;             // granule sweep: 8 granules per lane of one wave
constexpr int kResGranPerLane = 2 * kResMaxBlocks / kWave;
constexpr int kResMaxM = 64;                   // aggregate-M nodes staged in LDS
constexpr size_t kResLdsBudget = 150 * 1024;   // dynamic LDS per workgroup
constexpr size_t kResHdrMaxBytes = 32 * 1024;  // row-header table in LDS
constexpr unsigned long long kResTimeoutTicks = 400000000ull;  // 4 s of the 100 MHz wall clock
constexpr size_t kResGranBytes = sizeof(unsigned long long) * 2 * 2 * kResMaxBlocks;
constexpr size_t kResSyncBytes = kResGranBytes + 16;          // + timeout word, padded to 16 B

// Labour states of period t for the slice (in place: lab(t-1) -> lab(t)).  Each thread
// draws kDrawGroup agent pairs at once: their Philox chains are independent, so they
// overlap instead of running back to back (the draw sits on the critical path of the
// workgroup that publishes last).
// Thread `vt` of `nvt` drawing threads takes agent pairs vt, vt + nvt, ..., G at a time.
constexpr int kDrawGroup = 4;
struct Slice {   // a workgroup's agents: their labour states, the local index of the first, their number
  uint8_t* L; long long start; int cnt;
};
template <int G>
__device__ __forceinline__ void draw_slice(const ResRun& r, long long offset, const Slice& sl, int t,
                                           const double* s_cdf, int n_lab, int vt, int nvt) {
  uint8_t* const L = sl.L;
  const long long start = sl.start;
  const int cnt = sl.cnt;
  const unsigned ctr0 = (r.ge_iter << 20) | (unsigned)t;
  const double* u = r.u ? r.u + (size_t)(t - r.t0) * r.u_ld + start : nullptr;
  const int nthr = nvt;
  for (int q0 = vt; 2 * q0 < cnt; q0 += G * nthr) {
    double u0[G], u1[G];
    int l0[G], l1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {   // the pair's labour states first (one 2-byte load), in flight across Philox
      const int i = 2 * (q0 + g * nthr);
      if (i + 1 < cnt) {
        const unsigned v = *reinterpret_cast<const unsigned short*>(L + i);
        l0[g] = (int)(v & 0xffu);
        l1[g] = (int)(v >> 8);
      } else {
        l0[g] = i < cnt ? L[i] : 0;
        l1[g] = 0;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int i = 2 * (q0 + g * nthr);
      if (u) {
        u0[g] = i < cnt ? u[i] : 0.0;
        u1[g] = i + 1 < cnt ? u[i + 1] : 0.0;
      } else {
#ifdef AIY_DIAG_NO_PHILOX
        u0[g] = 0.37 + 1e-9 * (double)(i & 1023); u1[g] = 0.41 + 1e-9 * (double)(i & 1023);   // diagnostic build only
#else
        philox_uniform2(ctr0, (uint64_t)((offset + start + i) >> 1), r.seed, 0u, u0[g], u1[g]);
#endif
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int i = 2 * (q0 + g * nthr);
      const int n0 = draw_labour(s_cdf, n_lab, l0[g], u0[g]);
      if (i + 1 < cnt) {
        const int n1 = draw_labour(s_cdf, n_lab, l1[g], u1[g]);
        *reinterpret_cast<unsigned short*>(L + i) = (unsigned short)(n0 | (n1 << 8));
      } else if (i < cnt) {
        L[i] = (uint8_t)n0;
      }
    }
  }
}


// Dynamic LDS: [cell headers (16-aligned)] [a: chunk doubles] [lab: chunk bytes]
__host__ __device__ inline size_t res_hdr_bytes(int n_cells) {
  return ((size_t)n_cells * sizeof(CellHdr) + 15) / 16 * 16;
}

// SHARD: the instantiation that takes the sharded flags (kResSharded, kResPrices, kResDrawNext,
// the agent offset of the shard); the single-rank streaming instantiations carry none of that
// code (the flags are kResDraw0, the offset 0: VERDICT r5 weak 4, 1 003 -> 1 045 us per period
// at configs[3] once the single-rank kernel carried them, gpurun_out/r08a_c3ab).  The
// LDS-resident form runs the SHARD instantiation for every launch (launch_resident).
template <int TH, int NA, bool IN_LDS, bool QUAD, bool SHARD>
__global__ __launch_bounds__(TH) void sim_resident_kernel(PanelDev P, ResRun r, aiy_market mk) {
  const int flags = SHARD ? r.flags : kResDraw0;
  const long long offset = SHARD ? r.offset : 0;
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  __shared__ double s_cdf[kLdsLab * kLdsLab];
  __shared__ double s_lvl[kLdsLab];
  __shared__ double s_Mg[kResMaxM];   // Mgrid: the period's M bracket search stays in LDS
  __shared__ double s_red[TH / kWave];
  __shared__ double s_price[4];   // Mnow, Rnow, Wnow, Mrkv
  __shared__ int s_abort;         // sweep timeout
#ifdef AIY_DIAG_PHASES
  __shared__ unsigned long long s_wdiag[TH / kWave];   // per-wave cycles inside tab_policy
  if (threadIdx.x < TH / kWave) s_wdiag[threadIdx.x] = 0;
#endif

  const int tid = threadIdx.x;
  const int nthr = TH;
  const int nb = gridDim.x;
  const int n_M = P.n_M, n_lab = P.n_lab, n_J = P.tab.g.n_J, n_cells = P.tab.g.n_cells;
  const long long start = (long long)blockIdx.x * r.chunk;
  const int cnt = (int)std::max(0LL, std::min(r.chunk, r.n - start));
  CellHdr* hdr = reinterpret_cast<CellHdr*>(s_dyn);   // [cell]
  double* A;
  uint8_t* L;
  if constexpr (IN_LDS) {
    A = reinterpret_cast<double*>(s_dyn + res_hdr_bytes(n_cells));
    L = reinterpret_cast<uint8_t*>(A + r.chunk);
  } else {
    A = r.a + start;
    L = r.lab + start;
  }

  for (int q = tid; q < n_lab * n_lab; q += nthr) s_cdf[q] = P.lab_cdf[q];
  for (int q = tid; q < n_lab; q += nthr) s_lvl[q] = P.lab_level[q];
  for (int q = tid; q < n_M; q += nthr) s_Mg[q] = P.M_grid[q];
  for (int q = tid; q < n_cells; q += nthr) hdr[q] = cell_header(P.tab, q);
  if constexpr (IN_LDS) {
    for (int i = tid; i < cnt; i += nthr) {
      A[i] = r.a[start + i];
      L[i] = r.lab[start + i];
    }
  }
  if (tid == 0) {
    if (flags & kResPrices) {   // period t0 - 1's mill from the all-reduced sum (AS:1867-1894)
      const Prices q = calc_prices(mk, P.mrkv_hist[r.t0 - 1], load_f64_agent(&r.sow[6]) / (double)r.n_total);
      s_price[0] = q.Mnow;
      s_price[1] = q.Rnow;
      s_price[2] = q.Wnow;
      s_price[3] = (double)q.Mrkv;
      if (blockIdx.x == 0) {   // sow and the history, as period_price_kernel (sow[6] is rewritten only
        // after every workgroup has read it: at this period's end, behind the granule sweep)
        store_f64_agent(&r.sow[0], q.Mnow);
        store_f64_agent(&r.sow[1], q.Aprev);
        store_f64_agent(&r.sow[2], (double)q.Mrkv);
        store_f64_agent(&r.sow[3], q.Rnow);
        store_f64_agent(&r.sow[4], q.Wnow);
        store_f64_agent(&r.sow[5], 0.0);
        store_f64_agent(&r.sow[7], (double)r.t0);
        if (r.hist_A) r.hist_A[r.t0 - 1] = q.Aprev;
        if (r.hist_M) r.hist_M[r.t0 - 1] = q.Mnow;
      }
    } else {
      s_price[0] = load_f64_agent(&r.sow[0]);
      s_price[1] = load_f64_agent(&r.sow[3]);
      s_price[2] = load_f64_agent(&r.sow[4]);
      s_price[3] = load_f64_agent(&r.sow[2]);
    }
  }
  __syncthreads();
  if (flags & kResDraw0) draw_slice<kDrawGroup>(r, offset, Slice{L, start, cnt}, r.t0, s_cdf, n_lab, tid, TH);
  __syncthreads();   // period t0's labour draws complete
  const bool sharded = SHARD && (flags & kResSharded) != 0;

  Prices last{};
#ifdef AIY_DIAG_PHASES
  unsigned long long ph[5] = {0, 0, 0, 0, 0}, tq = 0;
#define AIY_PH(k) do { if (tid == 0) { const unsigned long long tn = __builtin_amdgcn_s_memrealtime(); if (k) ph[k - 1] += tn - tq; tq = tn; } } while (0)
#else
#define AIY_PH(k) do {} while (0)
#endif
  for (int p = 0; p < r.n_periods; ++p) {
    const int t = r.t0 + p;
    const double Mnow = s_price[0], Rnow = s_price[1], Wnow = s_price[2];
    const int Mrkv = (int)s_price[3];
    int jc;
    double alpha;
    m_bracket(s_Mg, n_M, Mnow, jc, alpha);
    const int mrkv_next = P.mrkv_hist[t];   // read-only history: issued early, used by the sweep
    AIY_PH(0);

    // ---- 1. agents: lookups, a = m - c, partial sum ----
    double local = 0.0;
    constexpr bool kPairs = !IN_LDS && NA % 2 == 0;
    for (int base = 0; base < cnt; base += TH * NA) {
      double m[NA];
      int ln[NA], cell[NA];
      // agent of slot k: consecutive lanes take consecutive agents (i = base + k TH + tid), except
      // the streaming form: agent PAIRS per lane (i = base + 2 (k/2 TH + tid) + k%2), so the
      // assets move as 16-byte loads / stores and the labour states as 2-byte ones
      if constexpr (kPairs) {
#pragma unroll
        for (int kp = 0; kp < NA / 2; ++kp) {
          const int i = base + 2 * (kp * TH + tid);
          double a0, a1;
          int q0, q1;
          if (i + 1 < cnt) {
            // the agent stream carries the nontemporal hint (keeps the policy table in L2:
            // 1 035 -> 1 002 us per period at 1e8 agents, gpurun_out/r05q)
            const st_d2 avv = __builtin_nontemporal_load(reinterpret_cast<const st_d2*>(A + i));
            const double2 av = make_double2(avv.x, avv.y);
            const unsigned lv = *reinterpret_cast<const unsigned short*>(L + i);
            a0 = av.x; a1 = av.y; q0 = (int)(lv & 0xffu); q1 = (int)(lv >> 8);
          } else {   // tail lanes: dummy work on the last agent
            const int ic = i < cnt ? i : cnt - 1;
            a0 = a1 = A[ic];
            q0 = q1 = L[ic];
          }
          ln[2 * kp] = q0;
          ln[2 * kp + 1] = q1;
          m[2 * kp] = Rnow * a0 + Wnow * (s_lvl[q0] * 1.0);                              // AS:1283
          m[2 * kp + 1] = Rnow * a1 + Wnow * (s_lvl[q1] * 1.0);
          cell[2 * kp] = (2 * q0 + Mrkv) * n_J + jc;                                     // employed (Urate = 0)
          cell[2 * kp + 1] = (2 * q1 + Mrkv) * n_J + jc;
        }
      } else
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const int i0 = base + k * TH + tid;
        const int i = i0 < cnt ? i0 : cnt - 1;                                            // tail lanes: dummy work
        ln[k] = L[i];
        m[k] = Rnow * A[i] + Wnow * (s_lvl[ln[k]] * 1.0);                                 // AS:1283
        cell[k] = (2 * ln[k] + Mrkv) * n_J + jc;                                          // employed (Urate = 0)
      }
#ifdef AIY_DIAG_NO_LOOKUP
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const int i = base + k * TH + tid;
        if (i < cnt) { A[i] = 0.9 * m[k]; local += 0.9 * m[k]; }   // diagnostic build only
      }
      continue;
#endif
      double c[NA];
#ifdef AIY_DIAG_PHASES
      const unsigned long long w0 = __builtin_amdgcn_s_memtime();
#endif
      tab_policy<NA, QUAD>(P.tab, cell, hdr, cell, m, alpha, n_M > 1, c);                       // AS:1326-1408
#ifdef AIY_DIAG_PHASES
      if ((tid & (kWave - 1)) == 0) {
        const unsigned long long w1 = __builtin_amdgcn_s_memtime();
        atomicAdd(&s_wdiag[tid / kWave], (unsigned long long)(w1 - w0));
      }
#endif
      if constexpr (kPairs) {
#pragma unroll
        for (int kp = 0; kp < NA / 2; ++kp) {
          const int i = base + 2 * (kp * TH + tid);
          const double an0 = m[2 * kp] - c[2 * kp], an1 = m[2 * kp + 1] - c[2 * kp + 1];   // AS:1415
          if (i + 1 < cnt) {
            st_d2 o;
            o.x = an0;
            o.y = an1;
            __builtin_nontemporal_store(o, reinterpret_cast<st_d2*>(A + i));
            local += an0;
            local += an1;
          } else if (i < cnt) {
            A[i] = an0;
            local += an0;
          }
        }
      } else
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const int i = base + k * TH + tid;
        if (i < cnt) {
          const double an = m[k] - c[k];                                                  // AS:1415
          A[i] = an;
          local += an;
        }
      }
    }

    // ---- 2. publish the workgroup partial as two tagged granules ----
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o, kWave);
    if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = local;
    __syncthreads();
    AIY_PH(1);
    const unsigned e = r.ep0 + (unsigned)p + 1;
    unsigned long long* gslot = r.gran + (size_t)(e & 1) * 2 * nb;
    if (tid == 0) {
      double sb = 0.0;
      for (int w = 0; w < nthr / kWave; ++w) sb += s_red[w];
      const unsigned long long bits = (unsigned long long)__double_as_longlong(sb);
      __hip_atomic_store(to_global(&gslot[2 * blockIdx.x]), ((unsigned long long)e << 32) | (bits >> 32), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(to_global(&gslot[2 * blockIdx.x + 1]), ((unsigned long long)e << 32) | (bits & 0xffffffffull),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- 3. next period's labour draws overlap the exchange (waves 1..; wave 0 sweeps) ----
    if (p + 1 < r.n_periods || (flags & kResDrawNext)) {   // waves 1.. share every pair
      if (tid >= kWave) draw_slice<kDrawGroup + 1>(r, offset, Slice{L, start, cnt}, t + 1, s_cdf, n_lab, tid - kWave, TH - kWave);
    }
    AIY_PH(2);
    // ---- 4. wave 0 sweeps every workgroup's granules, sums in fixed order, prices (sharded:
    //      workgroup 0 leaves the shard's sum for the all-reduce) ----
    if (tid < kWave && (!sharded || blockIdx.x == 0)) {
      unsigned long long gv[kResGranPerLane];
      const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
      int ok = 1;
      for (;;) {
        bool all = true;
#pragma unroll
        for (int k = 0; k < kResGranPerLane; ++k) {
          const int gi = tid * kResGranPerLane + k;
          if (gi < 2 * nb) {
            gv[k] = __hip_atomic_load(to_global(&gslot[gi]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            all = all && (unsigned)(gv[k] >> 32) == e;
          } else {
            gv[k] = 0;
          }
        }
        if (__all(all)) break;
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t_start > kResTimeoutTicks) { ok = 0; break; }
      }
      AIY_PH(3);
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < kResGranPerLane; k += 2) {
        const unsigned long long bits = ((gv[k] & 0xffffffffull) << 32) | (gv[k + 1] & 0xffffffffull);
        acc += __longlong_as_double((long long)bits);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
      if (tid == 0 && sharded) {
        if (!ok) __hip_atomic_store(to_global(r.tmo), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_abort = ok ? 0 : 1;
        store_f64_agent(&r.sow[6], acc);
      } else if (tid == 0) {
        if (!ok) __hip_atomic_store(to_global(r.tmo), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_abort = ok ? 0 : 1;
        last = calc_prices(mk, mrkv_next, acc / (double)r.n);   // np.mean(np.array(aNow))
        s_price[0] = last.Mnow;
        s_price[1] = last.Rnow;
        s_price[2] = last.Wnow;
        s_price[3] = (double)last.Mrkv;
        if (blockIdx.x == 0) {
          if (r.hist_A) r.hist_A[t] = last.Aprev;
          if (r.hist_M) r.hist_M[t] = last.Mnow;
        }
      }
    }
    __syncthreads();
    if ((!sharded || blockIdx.x == 0) && s_abort) return;   // sweep timeout: the host reports it (tmo word)
    AIY_PH(4);
  }
  if constexpr (IN_LDS) {
    for (int i = tid; i < cnt; i += nthr) {
      r.a[start + i] = A[i];
      r.lab[start + i] = L[i];
    }
  }
#ifdef AIY_DIAG_PHASES
  if (tid == 0 && (blockIdx.x == 0 || blockIdx.x == nb / 2 || blockIdx.x == nb - 1))
  {
    printf("[phases] block %d/%d cnt %d: lookup %.2f publish %.2f sweep %.2f prices+draws %.2f us/period\n", blockIdx.x, nb,
           cnt, ph[0] * 0.01 / r.n_periods, ph[1] * 0.01 / r.n_periods, ph[2] * 0.01 / r.n_periods,
           ph[3] * 0.01 / r.n_periods);
    if (blockIdx.x == 0) {
      for (int w = 0; w < TH / kWave; ++w)
        printf("[phases] block 0 wave %d: tab_policy %.0f cycles/period\n", w, (double)s_wdiag[w] / r.n_periods);
      printf("[phases] search-loop wave trips (all blocks) %u\n", diag_search_iters);
    }
  }
#endif
  if (blockIdx.x == 0 && tid == 0 && r.n_periods > 0 && !sharded) {
    r.sow[0] = last.Mnow;
    r.sow[1] = last.Aprev;
    r.sow[2] = (double)last.Mrkv;
    r.sow[3] = last.Rnow;
    r.sow[4] = last.Wnow;
    r.sow[5] = 0.0;
    r.sow[7] = (double)(r.t0 + r.n_periods);
  }
}

// Workgroup shape (threads per workgroup, agents per lane per pass, record loads) by
// shape id (AIY_OPT_RESIDENT_SHAPE, AIY_OPT_RESIDENT_SHAPE_STREAM): 0 -> 512 x 8 quad-cooperative (default: a ~4k-agent slice in ONE pass,
// 256 VGPRs), 1 -> 1024 x 4 quad-cooperative, 2 -> 512 x 8 per-lane record loads.
struct ResShape {
  int id, th, na;
};
static ResShape res_shape(int id) {
  switch (id) {
    case 1: return ResShape{1, 1024, 4};
    case 2: return ResShape{2, 512, 8};
    default: return ResShape{0, 512, 8};
  }
}

struct ResGeometry {
  int nb = 0;
  long long chunk = 0;
  bool in_lds = false;
  size_t lds = 0;
};

static ResGeometry res_geometry(aiy_handle* h, long long n, int n_cells, const ResShape& sh) {
  ResGeometry G;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 1) cus = 1;
  const long long want = (n + sh.th - 1) / sh.th;      // >= one agent per lane
  G.nb = (int)std::max(1LL, std::min<long long>(std::min(cus, kResMaxBlocks), want));
  G.chunk = (n + G.nb - 1) / G.nb;
  G.chunk += G.chunk & 1;                              // even: Philox pairs never straddle workgroups
  G.nb = (int)((n + G.chunk - 1) / G.chunk);
  const size_t hdr = res_hdr_bytes(n_cells);
  const size_t agents = (size_t)G.chunk * (sizeof(double) + 1);
  G.in_lds = !h->res_stream && hdr + agents <= kResLdsBudget;
  G.lds = G.in_lds ? (hdr + agents + 15) / 16 * 16 : hdr;
  return G;
}

bool resident_supported(const PanelDev& P) {
  return res_hdr_bytes(P.tab.g.n_cells) <= kResHdrMaxBytes && P.n_M <= kResMaxM;
}

// Every instantiation once: [shape][form].
enum { kFormStream, kFormStreamShard, kFormLds };
#define AIY_RES_FORMS(TH, NA, QUAD)                                                    \
  {reinterpret_cast<const void*>(sim_resident_kernel<TH, NA, false, QUAD, false>),     \
   reinterpret_cast<const void*>(sim_resident_kernel<TH, NA, false, QUAD, true>),      \
   reinterpret_cast<const void*>(sim_resident_kernel<TH, NA, true, QUAD, true>)}
static const void* const kResKernels[3][3] = {AIY_RES_FORMS(512, 8, true), AIY_RES_FORMS(1024, 4, true),
                                              AIY_RES_FORMS(512, 8, false)};
#undef AIY_RES_FORMS

// Launch the resident kernel for periods [r.t0, r.t0 + r.n_periods).
int32_t launch_resident(aiy_handle* h, const PanelDev& P, const aiy_market& mk, ResRun r, hipStream_t st) {
  if (!resident_supported(P)) return fail(h, AIY_ERR_UNSUPPORTED, "resident panel: header table too large");
  if (!resident_aligned(r.a, r.lab))
    return fail(h, AIY_ERR_ARG, "resident panel: assets must be 16-byte and labour states 2-byte aligned");
  ResShape sh = res_shape(h->res_shape);
  ResGeometry G = res_geometry(h, r.n, P.tab.g.n_cells, sh);
  if (!G.in_lds && h->res_shape_stream >= 0 && h->res_shape_stream != sh.id) {
    // the HBM-streaming form has its own shape (default 1024 x 4: 4 waves per SIMD hide the
    // streamed agents' latency better, 1 150 vs 1 504 us per period at 1e8 agents,
    // profiles/r05h_panel_shapes.jsonl)
    const ResShape ss = res_shape(h->res_shape_stream);
    const ResGeometry Gs = res_geometry(h, r.n, P.tab.g.n_cells, ss);
    if (!Gs.in_lds) {
      sh = ss;
      G = Gs;
    }
  }
  const int32_t rc = h->res_sync.reserve(h, kResSyncBytes);
  if (rc) return rc;
  AIY_HIP(h, h->res_timer.ensure());
  if (!h->res_attr_set) {   // LDS beyond the 64 KiB default, on this handle's device
    for (auto& shape : kResKernels)
      for (const void* k : shape)
        AIY_HIP(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kResLdsBudget));
    h->res_attr_set = true;
  }
  r.chunk = G.chunk;
  r.gran = h->res_sync.as<unsigned long long>();
  r.tmo = reinterpret_cast<unsigned*>(h->res_sync.as<char>() + kResGranBytes);
  if (r.n_total <= 0) r.n_total = r.n;
  // granule tags unique over the handle's launches: the slots need zeroing only when the tag
  // counter starts over (the first launch, or after 2^31 periods)
  if (h->res_epoch == 0 || h->res_epoch > 0x7fffffffu) {
    AIY_HIP(h, hipMemsetAsync(h->res_sync.get(), 0, kResSyncBytes, st));
    h->res_epoch = 0;
  } else if (!(r.flags & kResKeepTmo)) {
    AIY_HIP(h, hipMemsetAsync(r.tmo, 0, sizeof(unsigned), st));
  }
  r.ep0 = h->res_epoch;
  h->res_epoch += (unsigned)r.n_periods + 1u;
  PanelDev Pc = P;
  aiy_market mkc = mk;
  void* args[] = {&Pc, &r, &mkc};
  const bool shard = r.flags != kResDraw0 || r.offset != 0;   // any non-single-rank launch
  // the LDS-resident form always takes the runtime-flag instantiation: its folded single-rank
  // twin spilled more (124 vs 68 B per lane) and ran configs[1]'s periods at 16.8-16.9 against
  // 15.8-15.9 us (A/B on one box, gpurun_out/s7a_ablegs_*); the streaming form is the reverse
  // (1 004 vs 1 045 us per period at configs[3], r08b_c3ab)
  const void* fn = kResKernels[sh.id][G.in_lds ? kFormLds : shard ? kFormStreamShard : kFormStream];
  // Co-residency of the grid (one workgroup per CU, nb <= CU count) is checked here once
  // against the occupancy query; a plain launch then has the same residency as a
  // cooperative one without its per-launch host cost (MI355X_MICROARCH.md, coop-launch),
  // and the in-kernel sweep is bounded by a wall-clock timeout either way.
  if (fn != h->res_occ_fn || G.lds != h->res_occ_lds) {   // the occupancy query once per shape
    hipError_t e = hipSuccess;   // (the dynamic-LDS limit of every form is raised above, once)
    const Admit adm = admit_launch(fn, sh.th, G.lds, false, &e);
    if (adm == Admit::query_error)
      return fail(h, AIY_ERR_HIP, "hipOccupancyMaxActiveBlocksPerMultiprocessor failed: %s", hipGetErrorString(e));
    if (adm != Admit::fits) return fail(h, AIY_ERR_UNSUPPORTED, "resident panel: workgroup does not fit a CU");
    h->res_occ_fn = fn;
    h->res_occ_lds = G.lds;
  }
  // HIP events bracket the single-rank launches (aiy_panel_launch_stats); the sharded per-period
  // launches are timed by the caller's clock
  const bool timed = !(r.flags & kResSharded);
  if (timed) AIY_HIP(h, h->res_timer.begin(st));
  AIY_HIP(h, hipLaunchKernel(fn, dim3(G.nb), dim3(sh.th), args, G.lds, st));
  if (timed) AIY_HIP(h, h->res_timer.end(st));
  h->res_periods += r.n_periods;
  return AIY_OK;
}

// Timeout word of the last resident launch (0 = fine).  Synchronises `st`.
int32_t resident_status(aiy_handle* h, hipStream_t st, bool timed) {
  if (!h->res_sync.get()) return AIY_OK;
  unsigned tmo = 0;
  AIY_HIP(h, hipMemcpyAsync(&tmo, h->res_sync.as<char>() + kResGranBytes, sizeof(unsigned),
                            hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  if (timed) h->res_timer.collect();
  if (tmo) return fail(h, AIY_ERR_STATE, "resident panel: partial-sum exchange timed out (workgroups not co-resident?)");
  return AIY_OK;
}

}  // namespace aiy

// Launch statistics of the persistent panel (bench.py): kernel milliseconds summed over
// the resident launches since the last reset, their number and the periods they ran.
extern "C" int32_t aiy_panel_launch_stats(aiy_handle* h, double* ms_sum, int64_t* launches, int64_t* periods,
                                          int32_t reset) {
  if (!h) return AIY_ERR_ARG;
  h->res_timer.read(ms_sum, launches, reset != 0);
  if (periods) *periods = h->res_periods;
  if (reset) h->res_periods = 0;
  return AIY_OK;
}
