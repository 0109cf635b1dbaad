// Sequence-space Jacobian of the household block at the steady state for
// gfx950: the device stages of the fake-news algorithm (Auclert, Bardoczy, Rognlie and Straub,
// 2021).  The backward sweeps are aiy_transition_backward's; this file adds
//
//   jac_fanout_kernel    out[t] = lottery step of ONE mass with (lo[t], wlo[t]) for every
//                        period t of a [T'][n_cal][S][n_a] lottery: the tr_pull and
//                        tr_mix_forward (transition_common.h) that tr_forward_kernel calls, so
//                        the same bits as aiy_transition_forward with T = 1 on that period, the
//                        period in blockIdx.z -- the periods do not depend on each other.
//   jac_diff_kernel      shocked <- (shocked - ghost) / h, element by element, before anything
//                        is summed.
//   jac_expect_kernel    E_{k+1}[s][j] = wlo G_k[s][lo] + (1 - wlo) G_k[s][lo + 1] with
//                        G_k[s][d] = sum_{s'} P[s, s'] E_k[s'][d] in ascending s': the adjoint
//                        step of transition_common.h (tr_adjoint_values, tr_adjoint_mix).  A
//                        block owns (calibration, 64 columns, all states), gathers from the
//                        previous launch's G, writes E_{k+1}, and mixes its own columns from LDS
//                        into G_{k+1} (ping-pong), so no separate mix launch and no atomics.
//   jac_contract_kernel  partial[cal][chunk][t][col] = sum over one chunk of the long index of
//                        E[t][cal][.] dD[col][cal][.], both inputs' columns in one pass over E,
//                        on v_mfma_f64_16x16x4_f64: a block owns a 64 x 64 tile of one chunk,
//                        stages 64 x 32 slabs of both operands through LDS (the long index is
//                        contiguous in both, so the global loads are coalesced along it) and
//                        each wave keeps 16 rows x 64 columns in four accumulators.
//   jac_sum_kernel       F = the chunks' partials added in chunk order.
//
// The chunk length is a constant, so the sums do not depend on the device or the batch.
// Offsets are size_t throughout (24 x 301 x 7 x 10 000 > 2^31).
#include "common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>

namespace aiy {

// ---------------------------------------------------------------------------------
// Fan-out step
// ---------------------------------------------------------------------------------
struct JacFan {
  int n_cal, S, n_a;
  const double* wlo;   // [T'][n_cal][S][n_a]
  const int* jb;       // [T'][n_cal][S][n_a + 1]
  const double* P;     // [n_cal][S][S]
};

__global__ __launch_bounds__(kTrBlock) void jac_fanout_kernel(JacFan A, const double* __restrict__ mass,
                                                              double* __restrict__ out) {
  const int t = blockIdx.z, S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  const size_t trow = ((size_t)t * A.n_cal + p.cal) * S;   // first row of (t, cal) in the [T'][n_cal][S][.] arrays
  __shared__ double Tl[kTrTile];   // T_s[d] of the block's columns
  double none = 0.0;               // (no consumption term)
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves)
    Tl[s * kTrCols + p.lane] =
        tr_pull<false>(A.jb + (trow + s) * (size_t)(n_a + 1), A.wlo + (trow + s) * (size_t)n_a,
                       mass + (p.rows + s) * (size_t)n_a, p.col, p.active, p.lane, nullptr, 0.0, 0.0, 0.0, none);
  __syncthreads();
  const double* Pc = A.P + p.rows * S;
#pragma unroll 1
  for (int sp = p.wave; sp < S; sp += kTrWaves) {
    const double acc = tr_mix_forward(Pc, Tl, S, sp, p.lane);
    if (p.active) out[(trow + sp) * (size_t)n_a + p.col] = acc;
  }
}

__global__ __launch_bounds__(256) void jac_diff_kernel(size_t n, double* __restrict__ shocked,
                                                       const double* __restrict__ ghost, double h) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    shocked[i] = (shocked[i] - ghost[i]) / h;
}

// ---------------------------------------------------------------------------------
// Expectation step
// ---------------------------------------------------------------------------------
struct JacExp {
  int S, n_a;
  const int* lo;          // [n_cal][S][n_a] the steady lottery (checked: in [0, n_a - 2])
  const double* wlo;
  const double* P;        // [n_cal][S][S]
  const double* a_grid;   // [n_cal][n_a]
};

// INIT: E_0 = a.  Else E_{k+1} from G_k (the row check keeps lo in [0, n_a - 2]).  Both write G of
// what they wrote to E.
template <bool INIT>
__global__ __launch_bounds__(kTrBlock) void jac_expect_kernel(JacExp A, const double* __restrict__ G_in,
                                                              double* __restrict__ E_out, double* __restrict__ G_out) {
  const int S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  __shared__ double El[kTrTile];   // E_{k+1}[s'] of the block's columns
  tr_adjoint_values(p, S, n_a, El, [&](int s, size_t o) {
    double e;
    if constexpr (INIT) e = A.a_grid[(size_t)p.cal * n_a + p.col];
    else e = tr_gather(G_in + (p.rows + s) * (size_t)n_a, A.lo[o], A.wlo[o]);
    E_out[o] = e;
    return e;
  });
  __syncthreads();
  tr_adjoint_mix(p, S, n_a, A.P, El, G_out);
}

// ---------------------------------------------------------------------------------
// Fake-news contraction
// ---------------------------------------------------------------------------------
constexpr int kJacChunk = 4096;        // long-index elements of one partial: a constant of the build
constexpr int kJacTile = 64;           // rows and columns of a block's output tile
constexpr int kJacKB = 32;             // long-index elements staged per step
constexpr int kJacLd = kJacKB + 2;     // LDS row pitch: 16 rows x 2 k land in 32 different 8-byte banks
constexpr int kJacBlock = 256;
constexpr int kJacPer = kJacTile * kJacKB / kJacBlock;   // slab elements per thread and operand

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct JacCon {
  int n_cal, T, n_col, nct, nchunk;
  size_t N;            // long index: S n_a
  const double* E;     // [T][n_cal][N]
  const double* D0;    // [n_col][n_cal][N] columns 0 .. n_col - 1
  const double* D1;    // [n_col][n_cal][N] columns n_col .. 2 n_col - 1
  double* part;        // [n_cal][nchunk][T][2 n_col]
};

__global__ __launch_bounds__(kJacBlock) void jac_contract_kernel(JacCon A) {
  const int C = 2 * A.n_col;
  const int t0 = (blockIdx.x / A.nct) * kJacTile, c0 = (blockIdx.x % A.nct) * kJacTile;
  const int chunk = blockIdx.y, cal = blockIdx.z;
  const size_t n0 = (size_t)chunk * kJacChunk;
  const size_t n1 = std::min(n0 + (size_t)kJacChunk, A.N);
  __shared__ double As[kJacTile * kJacLd];
  __shared__ double Bs[kJacTile * kJacLd];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  // staging: a thread holds element kk of the rows r8, r8 + 8, ... of both slabs.  T and the
  // column count are padded to the tile by guards: a row past the matrix reads row 0 (its
  // products reach only output rows / columns that are never stored), an element past the chunk
  // reads the chunk's last one and is staged times 0.0.  Every load is unconditional and in
  // bounds, so the 16 loads of a step are issued back to back (guarded by a select, the
  // compiler put each behind a branch with a wait of its own)
  const int kk = threadIdx.x & (kJacKB - 1), r8 = threadIdx.x / kJacKB;
  const double* ap[kJacPer];
  const double* bp[kJacPer];
#pragma unroll
  for (int i = 0; i < kJacPer; ++i) {
    const int t = t0 + r8 + (kJacBlock / kJacKB) * i;
    const int c = c0 + r8 + (kJacBlock / kJacKB) * i;
    const int tc = t < A.T ? t : 0, cc = c < C ? c : 0;
    ap[i] = A.E + ((size_t)tc * A.n_cal + cal) * A.N;
    bp[i] = (cc < A.n_col ? A.D0 + ((size_t)cc * A.n_cal + cal) * A.N
                          : A.D1 + ((size_t)(cc - A.n_col) * A.n_cal + cal) * A.N);
  }
  double ra[kJacPer], rb[kJacPer], keep;   // keep: applied when the slab is staged, not when it is loaded
  auto load = [&](size_t n) {
    const bool in = n + kk < n1;
    const size_t q = in ? n + kk : n1 - 1;   // always inside the row
    keep = in ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < kJacPer; ++i) {
      ra[i] = ap[i][q];
      rb[i] = bp[i][q];
    }
  };
  f64x4 acc[kJacTile / 16];
#pragma unroll
  for (int c = 0; c < kJacTile / 16; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
  // A operand: lane l holds A[row l & 15][k = l >> 4]; B operand: B[k = l >> 4][col l & 15]
  const int frag = (lane & 15) * kJacLd + (lane >> 4);
  load(n0);
  for (size_t n = n0; n < n1; n += kJacKB) {   // block-uniform
    __syncthreads();   // the previous step's readers are done with the slabs
#pragma unroll
    for (int i = 0; i < kJacPer; ++i) {
      const int r = r8 + (kJacBlock / kJacKB) * i;
      As[r * kJacLd + kk] = ra[i] * keep;
      Bs[r * kJacLd + kk] = rb[i] * keep;
    }
    __syncthreads();
    if (n + kJacKB < n1) load(n + kJacKB);   // the next slabs travel while this one is multiplied
#pragma unroll
    for (int k4 = 0; k4 < kJacKB; k4 += 4) {
      const double a = As[wave * 16 * kJacLd + frag + k4];
#pragma unroll
      for (int c = 0; c < kJacTile / 16; ++c) {
        const double b = Bs[c * 16 * kJacLd + frag + k4];
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
      }
    }
  }
  // C/D: col = lane & 15, row = (lane >> 4) + 4 reg
  double* out = A.part + ((size_t)cal * A.nchunk + chunk) * (size_t)A.T * C;
#pragma unroll
  for (int c = 0; c < kJacTile / 16; ++c) {
    const int col = c0 + 16 * c + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = t0 + 16 * wave + (lane >> 4) + 4 * reg;
      if (row < A.T && col < C) out[(size_t)row * C + col] = acc[c][reg];
    }
  }
}

// F[cal][t][col] = the chunks' partials in chunk order.
__global__ __launch_bounds__(256) void jac_sum_kernel(int n_cal, int nchunk, size_t per, const double* __restrict__ part,
                                                      double* __restrict__ F) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (size_t)n_cal * per) return;
  const size_t cal = q / per, e = q % per;
  const double* p = part + cal * nchunk * per + e;
  double v = 0.0;
  for (int k = 0; k < nchunk; ++k) v += p[(size_t)k * per];
  F[q] = v;
}

// ---------------------------------------------------------------------------------
// Work space (caller-owned): every region starts on a 256-byte boundary.
// ---------------------------------------------------------------------------------
struct JacWork {
  int *jb, *flag;       // jb: fan-out, T + 1 periods
  double *g, *part;     // g: G ping-pong
  size_t bytes, per;    // per: one period, n_cal S n_a
  int nchunk, nblk;
};

static bool jac_sizes_ok(int n_cal, int S, int n_a, int T) {
  if (!tr_pull_sizes_ok(n_cal, S, n_a) || T < 1 || T > 65534) return false;
  const long long nchunk = ((long long)S * n_a + kJacChunk - 1) / kJacChunk;
  const long long tiles = (long long)((T + kJacTile - 1) / kJacTile) * ((2 * (T + 1) + kJacTile - 1) / kJacTile);
  return nchunk <= 65535 && tiles <= 2147483647LL;
}

static JacWork jac_work(Carve c, int n_cal, int S, int n_a, int T) {
  JacWork L;
  L.per = (size_t)n_cal * S * n_a;
  L.nchunk = (int)(((size_t)S * n_a + kJacChunk - 1) / kJacChunk);
  L.nblk = tr_nblk(n_a);
  L.jb = c.take<int>((size_t)(T + 1) * n_cal * S * (n_a + 1));
  L.g = c.take<double>(2 * L.per);
  L.part = c.take<double>((size_t)n_cal * L.nchunk * T * 2 * (T + 1));
  L.flag = c.take<int>(256 / sizeof(int));
  L.bytes = c.bytes();
  return L;
}

// tr_check and the contraction's limits
static int32_t jac_check(aiy_handle* h, int n_cal, int S, int n_a, int T) {
  return tr_check(h, n_cal, S, n_a, true, T, jac_sizes_ok(n_cal, S, n_a, T));
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_jacobian_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t T) {
  if (!jac_sizes_ok(n_cal, S, n_a, T)) return -1;
  return (int64_t)jac_work(Carve(), n_cal, S, n_a, T).bytes;
}

extern "C" int32_t aiy_jacobian_fanout(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_t,
                                       const int32_t* lo, const double* wlo, const double* P, const double* mass,
                                       void* work, double* out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = jac_check(h, n_cal, S, n_a, T);
  if (rc) return rc;
  if (n_t < 1 || n_t > T + 1) return fail(h, AIY_ERR_ARG, "n_t=%d outside 1..T+1=%d", n_t, T + 1);
  if (!lo || !wlo || !P || !mass || !work || !out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const JacWork L = jac_work(Carve(work), n_cal, S, n_a, T);
  int* jb = L.jb;
  // inverse index of every period and the row check, before anything is written
  rc = tr_build_ranges(h, n_cal, S, n_a, n_t, lo, jb, L.flag, st);
  if (rc) return rc;
  JacFan A;
  A.n_cal = n_cal; A.S = S; A.n_a = n_a; A.wlo = wlo; A.jb = jb; A.P = P;
  hipLaunchKernelGGL(jac_fanout_kernel, dim3(L.nblk, n_cal, n_t), dim3(kTrBlock), 0, st, A, mass, out);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_jacobian_diff(aiy_handle* h, int64_t n, double* shocked, const double* ghost, double step,
                                     aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (n < 1) return fail(h, AIY_ERR_ARG, "n=%lld must be >= 1", (long long)n);
  if (!shocked || !ghost) return fail(h, AIY_ERR_ARG, "null buffer");
  if (!(step > 0.0)) return fail(h, AIY_ERR_ARG, "step must be > 0");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const unsigned nb = (unsigned)std::min<long long>(((long long)n + 255) / 256, 1 << 20);
  hipLaunchKernelGGL(jac_diff_kernel, dim3(nb), dim3(256), 0, st, (size_t)n, shocked, ghost, step);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_jacobian_expectation(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                            const int32_t* lo, const double* wlo, const double* P,
                                            const double* a_grid, void* work, double* E_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = jac_check(h, n_cal, S, n_a, T);
  if (rc) return rc;
  if (!lo || !wlo || !P || !a_grid || !work || !E_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const JacWork L = jac_work(Carve(work), n_cal, S, n_a, T);
  // the gather reads G at lo and lo + 1: the lottery passes the forward sweep's row check first
  rc = tr_build_ranges(h, n_cal, S, n_a, 1, lo, L.jb, L.flag, st);
  if (rc) return rc;
  double* G = L.g;
  JacExp A;
  A.S = S; A.n_a = n_a; A.lo = lo; A.wlo = wlo; A.P = P; A.a_grid = a_grid;
  const dim3 grid(L.nblk, n_cal);
  hipLaunchKernelGGL((jac_expect_kernel<true>), grid, dim3(kTrBlock), 0, st, A, (const double*)nullptr, E_out, G);
  for (int k = 0; k + 1 < T; ++k)   // E_{k+1} from G_k (buffer k & 1), G_{k+1} to the other one
    hipLaunchKernelGGL((jac_expect_kernel<false>), grid, dim3(kTrBlock), 0, st, A,
                       (const double*)(G + (size_t)(k & 1) * L.per), E_out + (size_t)(k + 1) * L.per,
                       G + (size_t)((k + 1) & 1) * L.per);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_jacobian_contract(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T,
                                         const double* E, const double* dD_R, const double* dD_w, void* work,
                                         double* F_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = jac_check(h, n_cal, S, n_a, T);
  if (rc) return rc;
  if (!E || !dD_R || !dD_w || !work || !F_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const JacWork L = jac_work(Carve(work), n_cal, S, n_a, T);
  JacCon A;
  A.n_cal = n_cal; A.T = T; A.n_col = T + 1; A.nchunk = L.nchunk;
  A.nct = (2 * A.n_col + kJacTile - 1) / kJacTile;
  A.N = (size_t)S * n_a;
  A.E = E; A.D0 = dD_R; A.D1 = dD_w;
  A.part = L.part;
  const unsigned tiles = (unsigned)((T + kJacTile - 1) / kJacTile) * (unsigned)A.nct;
  hipLaunchKernelGGL(jac_contract_kernel, dim3(tiles, L.nchunk, n_cal), dim3(kJacBlock), 0, st, A);
  const size_t per = (size_t)T * 2 * A.n_col;
  hipLaunchKernelGGL(jac_sum_kernel, dim3((unsigned)(((size_t)n_cal * per + 255) / 256)), dim3(256), 0, st, n_cal,
                     L.nchunk, per, (const double*)A.part, F_out);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}
