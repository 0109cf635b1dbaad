// Shared pieces of the kernels in which a calibration's cluster of workgroups works on one
// stationary distribution (hist_resident.hip: plain / Aitken iteration; hist_krylov.hip:
// BiCGSTAB, push form hist_bicg.h and pull form hist_pull.h; ge_resident.hip: the whole GE
// search): the per-calibration cluster run description, the covering-span record, the
// cluster barriers, wave sums, the cluster reduction (hc_reduce and its pieces: the one
// definition every BiCGSTAB solve and the GE search run) and the pull forms' exported
// prefix / suffix search.
#pragma once

#include <algorithm>

#include "common.h"
#include "hist_scratch.h"

namespace aiy {

constexpr int kHcMaxG = 128;                       // workgroups per calibration cluster
constexpr int kHcCand = 32;                        // covering workgroups per (row, workgroup)
constexpr int kHcRows = 8;                         // rows whose push loads are in flight together
// rows whose gather loads are in flight together: all (S <= 8) for one column per thread
template <int SMAX, int KC, int TH>
struct HcGather {
  static constexpr int kRows = SMAX == 8 ? 8 : 4;
};
constexpr size_t kHcLdsTotal = 160 * 1024;         // per CU
constexpr unsigned long long kHcTimeoutTicks = 200000000ull;   // 2 s of the 100 MHz clock
constexpr int kHcRed = 8;                          // values per cluster reduction (at most)
static_assert(2 * kHcRed <= kHcRedRec, "two granules per value of a reduction");

struct HcRun {
  int n_cal, cal0, S, n_a, G, nj, cap;   // cap: doubles of the span buffer / one slab
  int cw;                 // pull form: columns of one matvec chunk (hist_pull_plan)
  const int* lo;          // [n_cal][S][n_a]
  const double* wlo;      // [n_cal][S][n_a]
  const double* P;        // [n_cal][S][S]
  double* mass;           // [n_cal][S][n_a] in: start, out: final
  double* slab;           // [launch cals][G][2][cap]
  int* span;              // [launch cals][G][SMAX][4] (first, len, left base, right base)
  unsigned* ctr;          // [launch cals][kHcCtrStride]
  double* dist;           // [launch cals][2][G][4]: sup-norm change, Aitken dot products, valid
  double* dbuf;           // [n_cal][S][n_a] stored differences for the Aitken step (accel > 0);
                          // pull form (hist_pull.h): [n_cal][4][S][n_a] BiCGSTAB vectors r, p, v, t
  int* ainv;              // pull form: [n_cal][S][n_a + 1] inverse lottery
  int accel;              // Aitken extrapolation period E (0: plain iteration = the oracle's)
  int* iters_out;         // [n_cal]
  unsigned* err;          // 0 ok, 1 timeout, 2 span overflow / not monotone, 3 candidate overflow
  double tol;
  const double* tolv;     // [n_cal] per-calibration tolerance (device) or null: tol
  int max_iter;
};

struct HcCand {
  int w, first, len, base;   // destination d of the covering span sits at slab/LDS index base + d
};

// Cluster barrier: lane 0 adds one to the cluster counter (after the caller's drained sc1
// stores) and waits until it reaches `target`.  False on timeout (error word set).
__device__ __forceinline__ bool hc_barrier(unsigned* err, unsigned* ctr, unsigned target, int* s_flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(to_global(ctr), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 1;
    while (__hip_atomic_load(to_global(ctr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kHcTimeoutTicks) {
        __hip_atomic_store(to_global(err), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    *s_flag = ok;
  }
  __syncthreads();
  return *s_flag != 0;
}
__device__ __forceinline__ bool hc_barrier(const HcRun& r, unsigned* ctr, unsigned target, int* s_flag) {
  return hc_barrier(r.err, ctr, target, s_flag);
}

// Cluster barrier that also counts the workgroups whose `flag` is set: lane 0 adds
// (1 | flag << 32) to the 64-bit word of the barrier's parity (low half: arrivals, high
// half: cumulative flags of that parity; a workgroup can run at most one barrier ahead, so
// the other parity's word takes its early add) and waits for `target` arrivals (G times
// the barriers of this parity so far).  *nc_out: the flag count of this parity after every
// workgroup's add.  False on timeout (error word set).
__device__ __forceinline__ bool hc_barrier_count(unsigned* err, unsigned long long* cw, unsigned target,
                                                 unsigned flag, unsigned* nc_out, int* s_flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long v = __hip_atomic_fetch_add(to_global(cw), 1ull | ((unsigned long long)flag << 32), __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT) +
                           (1ull | ((unsigned long long)flag << 32));
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 1;
    while ((unsigned)v < target) {
      __builtin_amdgcn_s_sleep(1);
      v = __hip_atomic_load(to_global(cw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kHcTimeoutTicks) {
        __hip_atomic_store(to_global(err), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    *nc_out = (unsigned)(v >> 32);
    *s_flag = ok;
  }
  __syncthreads();
  return *s_flag != 0;
}

// One covering span's value at destination d: the own span from LDS (read once by the
// column's owner, then re-zeroed for the next push), a foreign one from its published slab.
__device__ __forceinline__ double hc_take(const HcCand& c, int w, int d, int par, int cap, const double* slab_cl,
                                          double* Tacc) {
  const int q = c.base + d;
  // two destinations (added at the use): one shared register would make the LDS read
  // wait for every earlier slab load in flight (write-after-write on the register)
  double vg = 0.0, vl = 0.0;
  if (c.w == w) {
    vl = Tacc[q];
    Tacc[q] = 0.0;
  } else {
    vg = load_f64_agent(&slab_cl[((size_t)c.w * 2 + par) * cap + q]);
  }
  return vg + vl;
}

// Sum over the 64 lanes (DPP: row shifts, then row broadcasts), valid in lane 63.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_add_src(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROWS, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double wave_sum_lane63(double v) {
  v += dpp_add_src<0x111, 0xF>(v);   // row_shr:1
  v += dpp_add_src<0x112, 0xF>(v);   // row_shr:2
  v += dpp_add_src<0x114, 0xF>(v);   // row_shr:4
  v += dpp_add_src<0x118, 0xF>(v);   // row_shr:8   (lane 15 of every row: the row's sum)
  v += dpp_add_src<0x142, 0xA>(v);   // row_bcast:15 into rows 1, 3
  v += dpp_add_src<0x143, 0xC>(v);   // row_bcast:31 into rows 2, 3
  return v;
}

// Whether the cluster's error word is set: thread 0 reads it, every thread gets the answer.
// Called behind a cluster barrier, so every workgroup of the cluster gets the same one.
__device__ __forceinline__ bool hc_failed(const unsigned* err, int* s_stop) {
  if (threadIdx.x == 0) *s_stop = __hip_atomic_load(to_global(err), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  __syncthreads();
  return *s_stop != 0;
}

// Push forms: whether every own lottery entry of this workgroup (columns [j0, j1), thread t owns
// j0 + t + k TH, k < KC) lies inside the grid and inside the bracket [lo(j0), lo(j1 - 1)] of its
// row's end columns, for which the spans are laid out: an entry beyond it would add into another
// row's span or behind the span buffer.  Once per solve, before the first cluster barrier.  Eight
// rows' loads are issued before the first compare (indices clamped to the last own column and the
// last state: the same entries again, no predicate), the flags combined without branches.
template <int KC, int TH>
__device__ __forceinline__ bool hc_own_in_bracket(const int* LO, int S, int n_a, int j0, int j1) {
  constexpr int R = 8;
  int bad = 0;
  for (int s0 = 0; s0 < S; s0 += R) {
    int l[R][KC], f[R], fl[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int* Ls = LO + (size_t)min(s0 + u, S - 1) * n_a;
      f[u] = Ls[j0];
      fl[u] = Ls[j1 - 1];
#pragma unroll
      for (int k = 0; k < KC; ++k) l[u][k] = Ls[min(j0 + (int)threadIdx.x + k * TH, j1 - 1)];
    }
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int k = 0; k < KC; ++k)
        bad |= (int)(l[u][k] < f[u]) | (int)(l[u][k] > fl[u]) | (int)(l[u][k] < 0) | (int)(l[u][k] > n_a - 2);
  }
  return bad == 0;
}

// ---- cluster reduction ----
// Cluster-wide reduction of nv <= kHcRed per-thread values (bit v of kmax: nan_max, else sum),
// fixed order at every level, so every workgroup gets the same s_res: lanes by
// wave_sum_lane63 / wave_nan_max, waves ascending, then workgroups lane and lane + 64 and the
// wave sum over lanes.  The workgroup's values travel as tagged 8-byte granules ({epoch, 32
// data bits}, two per double, sc1 stores; MI355X_MICROARCH.md hand-off R2): the data is its
// own flag, so there is no counter barrier and no store drain -- one wave re-reads the
// cluster's granules until every tag carries this reduction's epoch.  Epochs count up from 1
// within a launch (the host zeroes the granules before each launch) and every user of a
// launch counts on the same `ne`; slots alternate by epoch parity, and a workgroup stores
// epoch e + 1 only after its sweep of epoch e, so when a slot is rewritten (epoch e + 2, after
// a sweep that saw every workgroup's e + 1) every workgroup has read it.
__device__ __forceinline__ unsigned long long hc_red_tag(unsigned ne) { return (unsigned long long)ne << 32; }
__device__ __forceinline__ unsigned long long* hc_red_slot(unsigned long long* gran, int G, unsigned ne) {
  return gran + (size_t)(ne & 1) * G * kHcRedRec;
}
// the workgroup's wave partials of nv values into s_part (visible after the next barrier)
template <int NWS>
__device__ __forceinline__ void hc_wave_parts(const double* vals, int nv, unsigned kmax, double (*s_part)[NWS]) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int v = 0; v < kHcRed; ++v) {
    if (v < nv) {
      const double x = (kmax >> v) & 1u ? wave_nan_max(vals[v]) : wave_sum_lane63(vals[v]);
      if (lane == kWave - 1) s_part[v][wid] = x;
    }
  }
}
// threads < nv: workgroup w's values (its TH / kWave waves in ascending order) as two tagged
// granules each
template <int TH, int NWS>
__device__ __forceinline__ void hc_store_granules(unsigned long long* slot, int w, unsigned long long tag, int nv,
                                                  unsigned kmax, double (*s_part)[NWS]) {
  const int tid = threadIdx.x;
  if (tid < nv) {
    const int v = tid;
    double x = s_part[v][0];
    for (int q = 1; q < TH / kWave; ++q) x = (kmax >> v) & 1u ? nan_max(x, s_part[v][q]) : x + s_part[v][q];
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    unsigned long long* g = slot + (size_t)w * kHcRedRec + 2 * v;
    __hip_atomic_store(to_global(g), tag | (b >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(to_global(g + 1), tag | (b & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// ONE wave: the granules of the cluster's G <= kHcMaxG workgroups (lanes read workgroups lane
// and lane + 64, until every tag carries this epoch), fixed-order sums into s_res; *s_ok = 0
// on timeout (error word set)
__device__ __forceinline__ void hc_sweep(const unsigned long long* slot, int G, unsigned long long tag, int nv,
                                         unsigned kmax, double* s_res, int* s_ok, unsigned* err) {
  static_assert(kHcMaxG <= 2 * kWave, "two workgroups per lane of the sweeping wave");
  const int lane = threadIdx.x & (kWave - 1);
  double xa[kHcRed], xb[kHcRed];
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  bool ok;
  do {   // every granule load of a pass in flight before the tag test
    ok = true;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int w2 = lane + u * kWave;
#pragma unroll
      for (int v = 0; v < kHcRed; ++v) {
        double x = 0.0;
        if (v < nv && w2 < G) {
          const unsigned long long* g = slot + (size_t)w2 * kHcRedRec + 2 * v;
          const unsigned long long hi = __hip_atomic_load(to_global(g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const unsigned long long lo = __hip_atomic_load(to_global(g + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = ok && (hi & 0xffffffff00000000ull) == tag && (lo & 0xffffffff00000000ull) == tag;
          x = __longlong_as_double((long long)((hi << 32) | (lo & 0xffffffffull)));
        }
        if (u == 0) xa[v] = x;
        else xb[v] = x;
      }
    }
    if (__all(ok)) break;
    __builtin_amdgcn_s_sleep(1);
    if (__builtin_amdgcn_s_memrealtime() - t0 > kHcTimeoutTicks) {
      if (lane == 0) __hip_atomic_store(to_global(err), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
  } while (true);
  if (lane == 0) *s_ok = ok ? 1 : 0;
#pragma unroll
  for (int v = 0; v < kHcRed; ++v) {
    if (v < nv) {
      const bool mx = (kmax >> v) & 1u;
      const double y = mx ? wave_nan_max(nan_max(xa[v], xb[v])) : wave_sum_lane63(xa[v] + xb[v]);
      if (lane == kWave - 1) s_res[v] = y;
    }
  }
}
// The whole reduction by workgroup w of G (TH threads; NWS >= TH / kWave: the row length of
// s_part): s_res valid in every thread on return, false on timeout.  prefetch(): loads the
// step after the reduction needs, in flight across the sweep.
template <int TH, int NWS, typename Prefetch>
__device__ __forceinline__ bool hc_reduce(unsigned long long* gran, int G, int w, unsigned& ne, const double* vals,
                                          int nv, unsigned kmax, double (*s_part)[NWS], double* s_res, int* s_flag,
                                          unsigned* err, Prefetch&& prefetch) {
  static_assert(TH / kWave <= NWS, "a partial per wave");
  hc_wave_parts(vals, nv, kmax, s_part);
  __syncthreads();
  ++ne;
  const unsigned long long tag = hc_red_tag(ne);
  unsigned long long* slot = hc_red_slot(gran, G, ne);
  hc_store_granules<TH>(slot, w, tag, nv, kmax, s_part);
  prefetch();
  if (threadIdx.x / kWave == 0) hc_sweep(slot, G, tag, nv, kmax, s_res, s_flag, err);
  __syncthreads();
  return *s_flag != 0;
}

// ---- pull forms: the lottery of the own sources ----
// lottery index of source j of row s; fresh: written in this launch by other workgroups (sc1 load)
__device__ __forceinline__ int hc_lo_at(const int* LO, int n_a, bool fresh, int s, int j) {
  const int* p = LO + (size_t)s * n_a + j;
  return fresh ? __hip_atomic_load(to_global(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
// threads < S: the exported prefix [j0, s_ex[2 s]) (lo < j0) and suffix [s_ex[2 s + 1], j1)
// (lo + 1 >= j1) of row s's own sources [j0, j1), the ones other workgroups pull
__device__ __forceinline__ void hc_exported(const int* LO, int n_a, bool fresh, int S, int j0, int j1, int* s_ex) {
  if ((int)threadIdx.x < S) {
    const int s = threadIdx.x;
    int lo = j0, hi = j1;   // first own j with lo_j >= j0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (hc_lo_at(LO, n_a, fresh, s, mid) < j0) lo = mid + 1; else hi = mid;
    }
    s_ex[2 * s] = lo;
    int lo2 = j0, hi2 = j1;   // first own j with lo_j + 1 >= j1
    while (lo2 < hi2) {
      const int mid = (lo2 + hi2) >> 1;
      if (hc_lo_at(LO, n_a, fresh, s, mid) + 1 < j1) lo2 = mid + 1; else hi2 = mid;
    }
    s_ex[2 * s + 1] = lo2;
  }
}

// BiCGSTAB form of the cluster kernel (hist_krylov.hip) for (S, padded S, columns per
// thread) and its state count (*smax_k); nullptr when there is no instantiation
const void* hist_bicg_pick(int S, int smax, int kc, int* smax_k, bool pull = false);
// pull form (hist_pull.h) for S > 8: the kernel, and its dynamic LDS for n_own columns
const void* hist_pull_pick(int S);
// pull form: the column chunk of a matvec (fewest item rounds + mix passes whose LDS fits
// `budget`) and its dynamic LDS bytes; false when even one-column chunks do not fit
bool hist_pull_plan(int S, int n_own, size_t budget, int* cw, size_t* lds);
#ifdef AIY_HP_TH
constexpr int kHpTH = AIY_HP_TH;   // tuning builds only
#else
constexpr int kHpTH = 512;
#endif

// ---- host side of a resident cluster launch ----
// LDS of one CU as the resident kernel `fn` may use it: the total (the device's, at most
// kHcLdsTotal), the kernel's static part and the dynamic budget left (a multiple of 256,
// 1 KB kept free).  False when a query fails or the static part leaves under 4 KB.
struct HcLds { size_t total, stat, dyn; };
inline bool hc_lds_budget(int device, const void* fn, HcLds& b) {
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return false;
  int lds_dev = 0;
  if (hipDeviceGetAttribute(&lds_dev, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) != hipSuccess)
    return false;
  b.total = std::min<size_t>(kHcLdsTotal, (size_t)lds_dev);
  b.stat = fa.sharedSizeBytes;
  if (b.stat + 4096 >= b.total) return false;
  b.dyn = (b.total - b.stat - 1024) / 256 * 256;
  return true;
}

// Workgroups per calibration cluster and columns per workgroup: as many workgroups as the
// CUs shared among n_cal clusters allow, within [g_min, min(g_cap, kHcMaxG)], every one
// owning at least one of the n_a columns.  False when g_min workgroups cannot be had.
inline bool hc_cluster_split(int n_a, int g_min, int g_cap, int cus, int n_cal, int* G, int* nj) {
  if (g_min > kHcMaxG || g_min > cus) return false;
  int g = std::max(g_min, std::min(std::min(g_cap, kHcMaxG), cus / std::max(1, n_cal)));
  g = std::min(g, n_a);
  *nj = (n_a + g - 1) / g;
  *G = (n_a + *nj - 1) / *nj;
  return true;
}

}  // namespace aiy
