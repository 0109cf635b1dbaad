// Welfare on the histogram for gfx950: the exact expected discounted utility of
// the discretised economy -- the Markov chain on (s, a_j) that the Young lotteries define -- and
// consumption-equivalent gains between two such values.  A household at node (s, j) of period t
// consumes c = R_t a_j + w_t lab_s - (wlo a[lo] + (1 - wlo) a[lo + 1]) (the term
// aiy_transition_forward sums into C_out), moves to lo / lo + 1 with weights wlo / 1 - wlo and
// draws s' from P[s, .]:
//
//   V_t[s][j]    = u(c_t[s][j]) + beta (wlo G_{t+1}[s][lo] + (1 - wlo) G_{t+1}[s][lo + 1])
//   G_{t+1}[s][d] = sum over s', ascending, of P[s, s'] V_{t+1}[s'][d]
//   u(c) = log c (CRRA = 1), c^(1 - CRRA) / (1 - CRRA) otherwise; c = 0 gives -inf, c < 0 NaN.
//
// This is the transpose of the forward lottery step (the adjoint step of transition_common.h, as
// jac_expect_kernel, with a per-period lottery, a flow payoff and a discount), so sum mass_0 V_0
// equals the discounted sum of sum mass_t u(c_t) plus beta^T sum mass_T V_T to rounding.
//
//   value_step_kernel   tr_adjoint_values / tr_adjoint_mix (transition_common.h): a block owns
//                       (calibration, 64 columns, all states); wave w forms V[s] for s = w, w + 4,
//                       ... from the previous launch's G (tr_gather at lo, lo + 1), writes it, keeps
//                       it in LDS, and after a barrier mixes the block's own columns by P into the
//                       other G buffer (ping-pong): one launch per period, no separate mix launch,
//                       no atomics in the recursion.  MIX only mixes a given V into G (the terminal value);
//                       PATH is one period of a path; STEADY is one step of the value iteration
//                       with the one lottery: it also folds max |V_new - V| and max |V_new| into
//                       the calibration's slots (64-bit atomicMax on the bit pattern of a
//                       non-negative double, as the EGM solve keeps its distances -- a maximum does
//                       not depend on the order) and skips a calibration whose previous step met
//                       max |V_new - V| <= tol (1 - beta) / beta max |V_new|.
//   value_reduce_kernel W[cal][s] = sum_j mass V: a workgroup of 256 threads per row, thread k
//                       sums its row_chunk sequentially, the chunk totals are added by
//                       row_block_sum (transition_common.h, shared with dist_stats_kernel).
//   value_ce_kernel     the consumption equivalent of every node, element by element.
//
// Every sum order is a function of S (the mix) or n_a (the reduction) only: a calibration has the
// same bits alone and in any batch.  The gather index is clamped to [0, n_a - 2], so a lottery
// that is not one (never produced by the library) cannot make the kernel read outside G.
// Offsets are size_t throughout (24 x 300 x 7 x 10 000 > 2^31).
#include "common.h"
#include "egm_common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>
#include <vector>

namespace aiy {

constexpr int kValMix = 0, kValPath = 1, kValSteady = 2;
// Convergence slots of one calibration (unsigned long long): max |V_new - V| and max |V_new| of
// the steps k % 3 == 0, 1, 2, the sticky converged flag, the last step that ran.
constexpr int kValDist = 0, kValMax = 3, kValFlag = 6, kValLast = 7, kValSlots = 8;

struct ValArgs {
  int S, n_a, pstride;    // pstride: T + 1 on a path, 1 at the steady state
  const int* lo;          // [n_cal][S][n_a] the period's lottery
  const double* wlo;
  const double* P;        // [n_cal][S][S]
  const double* a_grid;   // [n_cal][n_a]
  const double* R;        // [n_cal][pstride]
  const double* w;
  const double* lab;      // [n_cal][S]
  const double* beta;     // [n_cal]
  const double* crra;     // [n_cal]
};

// The stopping rule of the value iteration, on the device and on the host: the contraction bound
// then gives |V - V*| <= tol max |V|.  A NaN distance (c <= 0 somewhere) stops the calibration.
__host__ __device__ inline bool val_converged(double d, double vm, double tol, double beta) {
  const double thr = tol * (1.0 - beta) / beta * vm;
  return !(d > thr);
}

// u(c); kind 1: log, 3 and 5: products and one division, 0: pow.  Wave-uniform kind.
__device__ __forceinline__ double val_utility(double c, int kind, double crra) {
  double u;
  if (kind == 1) {
    u = log(c);
  } else if (kind == 3) {
    u = 1.0 / (-2.0 * (c * c));
  } else if (kind == 5) {
    const double c2 = c * c;
    u = 1.0 / (-4.0 * (c2 * c2));
  } else {
    u = pow(c, 1.0 - crra) / (1.0 - crra);
  }
  if (!(c > 0.0)) u = c == 0.0 ? -__builtin_inf() : __builtin_nan("");
  return u;
}

__device__ __forceinline__ unsigned long long val_bits(double v) {   // v >= 0 or NaN
  return v != v ? 0x7FF8000000000000ull : (unsigned long long)__double_as_longlong(v);
}

// MIX:    G_out = P V_src.
// PATH:   V of period t from G_in; written to Va and Vb where they are given.
// STEADY: V = Va in place from G_in, step `iter` >= 1 of the iteration.
// PATH and STEADY write G_out of the V they formed unless G_out is NULL.
template <int MODE>
__global__ __launch_bounds__(kTrBlock) void value_step_kernel(ValArgs A, int t, const double* __restrict__ V_src,
                                                              const double* __restrict__ G_in, double* Va,
                                                              double* __restrict__ Vb, double* __restrict__ G_out,
                                                              int iter, unsigned long long* slots, double tol) {
  const int S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  const int cal = p.cal, wave = p.wave, lane = p.lane;
  __shared__ double El[kTrTile];   // V[s'] of the block's columns
  __shared__ double red[2][kTrWaves];
  __shared__ int s_skip;
  double beta = 0.0;
  if constexpr (MODE != kValMix) beta = A.beta[cal];
  if constexpr (MODE == kValSteady) {
    unsigned long long* sl = slots + (size_t)cal * kValSlots;
    if (iter >= 2) {   // every block of the calibration reads the same words of the previous launch
      if (threadIdx.x == 0) {
        const bool done = load_u64_agent(&sl[kValFlag]) != 0ull;
        const double d = __longlong_as_double((long long)load_u64_agent(&sl[kValDist + (iter - 1) % 3]));
        const double vm = __longlong_as_double((long long)load_u64_agent(&sl[kValMax + (iter - 1) % 3]));
        const bool skip = done || val_converged(d, vm, tol, beta);
        s_skip = skip ? 1 : 0;
        if (skip && !done && blockIdx.x == 0) store_u64_agent(&sl[kValFlag], 1ull);
      }
      __syncthreads();
      if (s_skip) return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the slots of the next step; this step ran
      store_u64_agent(&sl[kValDist + (iter + 1) % 3], 0ull);
      store_u64_agent(&sl[kValMax + (iter + 1) % 3], 0ull);
      store_u64_agent(&sl[kValLast], (unsigned long long)iter);
    }
  }
  double Rt = 0.0, wt = 0.0, crra = 0.0, aj = 0.0;
  int kind = 0;
  const double* ag = A.a_grid + (size_t)cal * n_a;
  if constexpr (MODE != kValMix) {
    Rt = A.R[(size_t)cal * A.pstride + t];
    wt = A.w[(size_t)cal * A.pstride + t];
    crra = A.crra[cal];
    kind = crra_kind(crra);
    aj = ag[p.active ? p.col : n_a - 1];
  }
  double dmax = 0.0, vmax = 0.0;
  tr_adjoint_values(p, S, n_a, El, [&](int s, size_t o) {
    if constexpr (MODE == kValMix) {
      return V_src[o];
    } else {
      int d = A.lo[o];
      d = d < 0 ? 0 : (d > n_a - 2 ? n_a - 2 : d);
      const double wl = A.wlo[o];
      const double c = (Rt * aj + wt * A.lab[p.rows + s]) - tr_gather(ag, d, wl);
      const double v = val_utility(c, kind, crra) + beta * tr_gather(G_in + (p.rows + s) * (size_t)n_a, d, wl);
      if constexpr (MODE == kValSteady) {
        dmax = nan_max(dmax, fabs(v - Va[o]));
        vmax = nan_max(vmax, fabs(v));
      }
      if (Va != nullptr) Va[o] = v;
      if constexpr (MODE == kValPath)
        if (Vb != nullptr) Vb[o] = v;
      return v;
    }
  });
  if constexpr (MODE == kValSteady) {
    dmax = wave_nan_max(dmax);
    vmax = wave_nan_max(vmax);
    if (lane == 0) {
      red[0][wave] = dmax;
      red[1][wave] = vmax;
    }
  }
  __syncthreads();
  if constexpr (MODE == kValSteady) {
    if (threadIdx.x == 0) {
      double d = red[0][0], m = red[1][0];
      for (int q = 1; q < kTrWaves; ++q) {
        d = nan_max(d, red[0][q]);
        m = nan_max(m, red[1][q]);
      }
      unsigned long long* sl = slots + (size_t)cal * kValSlots;
      atomicMax(&sl[kValDist + iter % 3], val_bits(d));
      atomicMax(&sl[kValMax + iter % 3], val_bits(m));
    }
  }
  if (G_out != nullptr) tr_adjoint_mix(p, S, n_a, A.P, El, G_out);   // (kernel argument: block-uniform)
}

// W[row] = sum_j mass[row][j] V[row][j], row = (cal, s).
__global__ __launch_bounds__(kTrBlock) void value_reduce_kernel(int n_a, const double* __restrict__ mass,
                                                                const double* __restrict__ V,
                                                                double* __restrict__ W) {
  const size_t row = blockIdx.x;
  const double* m = mass + row * n_a;
  const double* v = V + row * n_a;
  int j0, j1;
  row_chunk(n_a, threadIdx.x, j0, j1);
  double acc = 0.0;
  for (int j = j0; j < j1; ++j) acc += m[j] * v[j];
  __shared__ double s_wave[kTrWaves];
  const double tot = row_block_sum(acc, s_wave);
  if (threadIdx.x == 0) W[row] = tot;
}

__global__ __launch_bounds__(256) void value_ce_kernel(size_t n, size_t per, const double* __restrict__ V_new,
                                                       const double* __restrict__ V_base,
                                                       const double* __restrict__ beta,
                                                       const double* __restrict__ crra, double* __restrict__ g) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const size_t cal = i / per;
    const double gam = crra[cal];
    const double vn = V_new[i], vb = V_base[i];
    g[i] = gam == 1.0 ? exp((1.0 - beta[cal]) * (vn - vb)) - 1.0 : pow(vn / vb, 1.0 / (1.0 - gam)) - 1.0;
  }
}

// Work space (caller-owned): the two mixed values, then the convergence slots.
struct ValWork {
  double* g;
  unsigned long long* slots;
  size_t bytes, per;   // per: n_cal S n_a
  int nblk;
};

static ValWork val_work(Carve c, int n_cal, int S, int n_a) {
  ValWork L;
  L.per = (size_t)n_cal * S * n_a;
  L.nblk = tr_nblk(n_a);
  L.g = c.take<double>(2 * L.per);
  L.slots = c.take<unsigned long long>((size_t)n_cal * kValSlots);
  L.bytes = c.bytes();
  return L;
}

static void launch_mix(const ValArgs& A, int n_cal, int nblk, const double* V, double* G, hipStream_t st) {
  hipLaunchKernelGGL((value_step_kernel<kValMix>), dim3(nblk, n_cal), dim3(kTrBlock), 0, st, A, 0, V,
                     (const double*)nullptr, (double*)nullptr, (double*)nullptr, G, 0,
                     (unsigned long long*)nullptr, 0.0);
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_value_work_bytes(int32_t n_cal, int32_t S, int32_t n_a) {
  if (!tr_pull_sizes_ok(n_cal, S, n_a)) return -1;
  return (int64_t)val_work(Carve(), n_cal, S, n_a).bytes;
}

extern "C" int32_t aiy_value_backward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                      const int32_t* lo, const double* wlo, const double* P, const double* a_grid,
                                      const double* R, const double* w, const double* lab, const double* beta,
                                      const double* crra, const double* V_term, void* work, double* V0_out,
                                      double* V_path_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (T < 1) return fail(h, AIY_ERR_ARG, "T=%d must be >= 1", T);
  int32_t rc = tr_check(h, n_cal, S, n_a);
  if (rc) return rc;
  if (!lo || !wlo || !P || !a_grid || !R || !w || !lab || !beta || !crra) return fail(h, AIY_ERR_ARG, "null model array");
  if (!V_term || !work || !V0_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const ValWork L = val_work(Carve(work), n_cal, S, n_a);
  double* G = L.g;
  ValArgs A;
  A.S = S; A.n_a = n_a; A.pstride = T + 1;
  A.lo = lo; A.wlo = wlo; A.P = P; A.a_grid = a_grid; A.R = R; A.w = w; A.lab = lab; A.beta = beta; A.crra = crra;
  launch_mix(A, n_cal, L.nblk, V_term, G, st);
  int b = 0;   // the buffer that holds G_{t+1}
  for (int t = T - 1; t >= 0; --t, b ^= 1) {
    A.lo = lo + (size_t)t * L.per;
    A.wlo = wlo + (size_t)t * L.per;
    hipLaunchKernelGGL((value_step_kernel<kValPath>), dim3(L.nblk, n_cal), dim3(kTrBlock), 0, st, A, t,
                       (const double*)nullptr, (const double*)(G + (size_t)b * L.per), t == 0 ? V0_out : (double*)nullptr,
                       V_path_out ? V_path_out + (size_t)t * L.per : (double*)nullptr,
                       t > 0 ? G + (size_t)(b ^ 1) * L.per : (double*)nullptr, 0, (unsigned long long*)nullptr, 0.0);
  }
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_value_stationary(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const int32_t* lo,
                                        const double* wlo, const double* P, const double* a_grid, const double* R,
                                        const double* w, const double* lab, const double* beta, const double* crra,
                                        const double* beta_host, double tol, int32_t max_iter, int32_t chunk,
                                        double* V, void* work, int32_t* iters_out, double* dist_out,
                                        aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a);
  if (rc) return rc;
  if (!(tol >= 1e-13)) return fail(h, AIY_ERR_ARG, "tol=%g must be >= 1e-13 (rounding moves V by more per step)", tol);
  if (max_iter < 1) return fail(h, AIY_ERR_ARG, "max_iter=%d must be >= 1", max_iter);
  if (!lo || !wlo || !P || !a_grid || !R || !w || !lab || !beta || !crra || !beta_host)
    return fail(h, AIY_ERR_ARG, "null model array");
  if (!V || !work || !iters_out || !dist_out) return fail(h, AIY_ERR_ARG, "null buffer");
  if (chunk <= 0) chunk = 32;
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const ValWork L = val_work(Carve(work), n_cal, S, n_a);
  double* G = L.g;
  unsigned long long* slots = L.slots;
  const size_t n_slots = (size_t)n_cal * kValSlots;
  AIY_HIP(h, hipMemsetAsync(slots, 0, n_slots * sizeof(unsigned long long), st));
  ValArgs A;
  A.S = S; A.n_a = n_a; A.pstride = 1;
  A.lo = lo; A.wlo = wlo; A.P = P; A.a_grid = a_grid; A.R = R; A.w = w; A.lab = lab; A.beta = beta; A.crra = crra;
  launch_mix(A, n_cal, L.nblk, V, G, st);
  std::vector<unsigned long long> hs(n_slots);
  auto as_double = [](unsigned long long b) { double d; std::memcpy(&d, &b, sizeof(d)); return d; };
  int k = 0;
  while (true) {
    const int end = std::min(k + chunk, (int)max_iter);
    for (; k < end; ++k)   // step k + 1 reads G of buffer k & 1 and writes the other one
      hipLaunchKernelGGL((value_step_kernel<kValSteady>), dim3(L.nblk, n_cal), dim3(kTrBlock), 0, st, A, 0,
                         (const double*)nullptr, (const double*)(G + (size_t)(k & 1) * L.per), V, (double*)nullptr,
                         G + (size_t)((k + 1) & 1) * L.per, k + 1, slots, tol);
    AIY_CHECK_LAUNCH(h);
    AIY_HIP(h, hipMemcpyAsync(hs.data(), slots, n_slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    AIY_HIP(h, hipStreamSynchronize(st));
    bool all = true;
    for (int c = 0; c < n_cal; ++c) {
      const unsigned long long* sl = hs.data() + (size_t)c * kValSlots;
      const int last = (int)sl[kValLast];
      const double d = as_double(sl[kValDist + last % 3]), vm = as_double(sl[kValMax + last % 3]);
      iters_out[c] = last;
      dist_out[c] = d;
      all = all && (sl[kValFlag] != 0ull || val_converged(d, vm, tol, beta_host[c]));
    }
    if (all || k >= max_iter) break;
  }
  return AIY_OK;
}

extern "C" int32_t aiy_value_reduce(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, const double* mass,
                                    const double* V, double* W_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a);
  if (rc) return rc;
  if (!mass || !V || !W_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const size_t n_rows = (size_t)n_cal * S;
  rc = h->welf.reserve(h, n_rows * sizeof(double));
  if (rc) return rc;
  double* d_welf = h->welf.as<double>();
  hipLaunchKernelGGL(value_reduce_kernel, dim3((unsigned)n_rows), dim3(kTrBlock), 0, st, n_a, mass, V, d_welf);
  AIY_CHECK_LAUNCH(h);
  AIY_HIP(h, hipMemcpyAsync(W_out, d_welf, n_rows * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  return AIY_OK;
}

extern "C" int32_t aiy_consumption_equivalent(aiy_handle* h, int32_t n_cal, int64_t per, const double* V_new,
                                              const double* V_base, const double* beta, const double* crra,
                                              double* g_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (n_cal < 1 || per < 1) return fail(h, AIY_ERR_ARG, "bad sizes n_cal=%d per=%lld", n_cal, (long long)per);
  if (!V_new || !V_base || !beta || !crra || !g_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const size_t n = (size_t)n_cal * (size_t)per;
  const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 20);
  hipLaunchKernelGGL(value_ce_kernel, dim3(nb), dim3(256), 0, st, n, (size_t)per, V_new, V_base, beta, crra, g_out);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}
