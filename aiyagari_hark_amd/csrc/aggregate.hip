// Aggregate risk to first order for gfx950: the savings policy of every
// simulated period is the steady one plus the linearised response to the expected price paths,
//
//   a'_p[s][j] = a*[s][j] + sum_k op[k][s][j] X[p][k],   k < 2 (T + 1),
//
// op = the policy derivatives dA_R[0..T] then dA_w[0..T] (lead u outermost, as the backward
// sweeps leave them), X[p] = the expected dR and dw at leads 0..T of period p.  This file adds
//
//   agg_mean_kernel     out = wlo a[lo] + (1 - wlo) a[lo + 1], element by element: the savings
//                       policy a lottery stands for (clipped to the grid as the lottery is).
//   agg_lottery_kernel  the product above on v_mfma_f64_16x16x4_f64 with the locate of
//                       oracle.stationary.savings_lottery as its epilogue.  A block owns 64
//                       points x 64 periods of one calibration; the periods are the rows of
//                       the matrix instruction and the points its columns, so a lane's results
//                       lie along the point index and the lottery is stored in 128-byte runs.
//                       Slabs of 32 k of both operands go through LDS in jac_contract_kernel's
//                       image (transition_jac.hip): the operand is read along its contiguous
//                       point index, X along k.
//
// An output element is one accumulator entry: its k ascend four to an instruction, nothing is
// split over k and nothing is atomic, the tail of k and the tile edges are padded (in-bounds
// loads, staged times 0 / never stored).  So a period's lottery does not depend on n_p, on the
// period's place in its tile or on the batch.  Offsets are size_t (24 x 301 x 70 000 > 2^31).
// Non-finite operands are not checked, as in jac_contract_kernel: a NaN sum passes both clamps and
// is stored as lo = 0, wlo = NaN, and a non-finite op or X at k = K2 - 1 reaches its tile's padded
// k (staged times 0) as NaN.
#include "common.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>

namespace aiy {

#ifndef AIY_AGG_PERIODS
#define AIY_AGG_PERIODS 64             // periods of a block's tile: the measured choice
#endif
constexpr int kAggTile = 64;           // points of a block's tile, and periods of one of its row tiles
constexpr int kAggPT = AIY_AGG_PERIODS / kAggTile;   // row tiles of 64 periods per block: a wave keeps 16 rows of each
static_assert(kAggPT >= 1 && kAggPT * kAggTile == AIY_AGG_PERIODS, "the period tile is a multiple of 64");
constexpr int kAggKB = 32;             // k staged per step
constexpr int kAggLd = kAggKB + 2;     // LDS row pitch: 16 rows x 2 k land in 32 different 8-byte banks
constexpr int kAggBlock = 256;
constexpr int kAggPer = kAggTile * kAggKB / kAggBlock;   // slab elements per thread and operand
constexpr int kAggMaxT = 1 << 20;

typedef double agg_f64x4 __attribute__((ext_vector_type(4)));

struct AggSyn {
  int n_cal, n_a, T, n_p, K2;   // K2 = 2 (T + 1)
  size_t N;                     // points of a calibration: S n_a
  const double* a_star;         // [n_cal][N]
  const double* dA_R;           // [T + 1][n_cal][N]
  const double* dA_w;
  const double* X;              // [n_cal][n_p][K2]
  const double* a_grid;         // [n_cal][n_a]
  int* lo;                      // [n_p][n_cal][N]
  double* wlo;
};

__global__ __launch_bounds__(kAggBlock) void agg_lottery_kernel(AggSyn A) {
  const size_t n0 = (size_t)blockIdx.x * kAggTile;
  const int p0 = blockIdx.y * (kAggTile * kAggPT), cal = blockIdx.z;
  const int K2 = A.K2, nT1 = A.T + 1;
  __shared__ double Xs[kAggPT * kAggTile * kAggLd];   // [period][k]
  __shared__ double Os[kAggTile * kAggLd];   // [point][k]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int lane = threadIdx.x & (kWave - 1);
  // staging.  X: a thread holds k = kk of the periods r8, r8 + 8, ...; the operand: point pl of
  // k = kq, kq + 4, ...  A period past n_p reads period 0 and a point past N point 0 (their
  // products reach only outputs that are never stored); a k past K2 reads k = K2 - 1 and is
  // staged times 0.0.  Every load is unconditional and in bounds.
  const int kk = threadIdx.x & (kAggKB - 1), r8 = threadIdx.x / kAggKB;
  const int pl = threadIdx.x & (kAggTile - 1), kq = threadIdx.x / kAggTile;
  const double* xp[kAggPT * kAggPer];
#pragma unroll
  for (int i = 0; i < kAggPT * kAggPer; ++i) {
    const int p = p0 + r8 + (kAggBlock / kAggKB) * i;
    xp[i] = A.X + ((size_t)cal * A.n_p + (p < A.n_p ? p : 0)) * K2;
  }
  const size_t per = (size_t)A.n_cal * A.N;   // one lead of an operand
  const size_t opoint = (size_t)cal * A.N + (n0 + pl < A.N ? n0 + pl : 0);
  double rx[kAggPT * kAggPer], ro[kAggPer], keepx, keepo[kAggPer];
  auto load = [&](int kb) {
    const bool in = kb + kk < K2;
    const int q = in ? kb + kk : K2 - 1;
    keepx = in ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < kAggPT * kAggPer; ++i) rx[i] = xp[i][q];
#pragma unroll
    for (int i = 0; i < kAggPer; ++i) {
      const int k = kb + kq + (kAggBlock / kAggTile) * i;
      const bool ink = k < K2;
      const int kc = ink ? k : K2 - 1;
      const double* base = kc < nT1 ? A.dA_R + (size_t)kc * per : A.dA_w + (size_t)(kc - nT1) * per;
      keepo[i] = ink ? 1.0 : 0.0;
      ro[i] = base[opoint];
    }
  };
  agg_f64x4 acc[kAggPT][kAggTile / 16];
#pragma unroll
  for (int r = 0; r < kAggPT; ++r)
#pragma unroll
    for (int c = 0; c < kAggTile / 16; ++c) acc[r][c] = agg_f64x4{0.0, 0.0, 0.0, 0.0};
  // A operand: lane l holds X[period l & 15][k = l >> 4]; B operand: op[k = l >> 4][point l & 15]
  const int frag = (lane & 15) * kAggLd + (lane >> 4);
  load(0);
  for (int kb = 0; kb < K2; kb += kAggKB) {   // block-uniform
    __syncthreads();   // the previous step's readers are done with the slabs
#pragma unroll
    for (int i = 0; i < kAggPT * kAggPer; ++i) Xs[(r8 + (kAggBlock / kAggKB) * i) * kAggLd + kk] = rx[i] * keepx;
#pragma unroll
    for (int i = 0; i < kAggPer; ++i) Os[pl * kAggLd + kq + (kAggBlock / kAggTile) * i] = ro[i] * keepo[i];
    __syncthreads();
    if (kb + kAggKB < K2) load(kb + kAggKB);   // the next slabs travel while this one is multiplied
#pragma unroll
    for (int k4 = 0; k4 < kAggKB; k4 += 4) {
      double x[kAggPT];
#pragma unroll
      for (int r = 0; r < kAggPT; ++r) x[r] = Xs[(r * kAggTile + wave * 16) * kAggLd + frag + k4];
#pragma unroll
      for (int c = 0; c < kAggTile / 16; ++c) {
        const double o = Os[c * 16 * kAggLd + frag + k4];
#pragma unroll
        for (int r = 0; r < kAggPT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[r], o, acc[r][c], 0, 0, 0);
      }
    }
  }
  // C/D: point = lane & 15 of column tile c, period = (lane >> 4) + 4 reg of the wave's 16.
  // a' = a* + sum, clamped to the grid; then savings_lottery's locate.  The 16 searches of a
  // lane take the same number of steps, so their loads are in flight together.
  const double* ag = A.a_grid + (size_t)cal * A.n_a;
  const int n_a = A.n_a;
  const double a_first = ag[0], a_last = ag[n_a - 1];
  constexpr int kE = (kAggTile / 16) * 4;
  int top = 1;
  while (top <= n_a / 2) top *= 2;   // the largest power of two <= n_a: the first step of upper_bound
#pragma unroll
  for (int r = 0; r < kAggPT; ++r) {   // one row tile at a time: 16 searches in flight
    double v[kE];
    int pos[kE];
#pragma unroll
    for (int c = 0; c < kAggTile / 16; ++c) {
      const size_t n = n0 + 16 * c + (lane & 15);
      const double as = A.a_star[(size_t)cal * A.N + (n < A.N ? n : 0)];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        double a1 = as + acc[r][c][reg];
        a1 = a1 < a_first ? a_first : a1;
        a1 = a1 > a_last ? a_last : a1;
        v[4 * c + reg] = a1;
        pos[4 * c + reg] = 0;
      }
    }
    for (int step = top; step > 0; step >>= 1) {
#pragma unroll
      for (int e = 0; e < kE; ++e) {
        const int q = pos[e] + step;
        const int qc = q <= n_a ? q : n_a;   // the load stays in the grid; q > n_a is refused below
        const double node = ag[qc - 1];
        pos[e] = (q <= n_a && node <= v[e]) ? q : pos[e];
      }
    }
#pragma unroll
    for (int c = 0; c < kAggTile / 16; ++c) {
      const size_t n = n0 + 16 * c + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int p = p0 + r * kAggTile + 16 * wave + (lane >> 4) + 4 * reg;
        const int e = 4 * c + reg;
        int j = pos[e] - 1;
        j = j < 0 ? 0 : j;
        j = j > n_a - 2 ? n_a - 2 : j;
        const double hi = ag[j + 1], low = ag[j];
        double wl = (hi - v[e]) / (hi - low);
        wl = wl < 0.0 ? 0.0 : wl;
        wl = wl > 1.0 ? 1.0 : wl;
        if (p < A.n_p && n < A.N) {
          const size_t o = ((size_t)p * A.n_cal + cal) * A.N + n;
          A.lo[o] = j;
          A.wlo[o] = wl;
        }
      }
    }
  }
}

// out = wlo a[lo] + (1 - wlo) a[lo + 1]; lo is held to [0, n_a - 2] so that the read stays in the grid.
__global__ __launch_bounds__(256) void agg_mean_kernel(size_t n, size_t N, int n_cal, int n_a, const int* __restrict__ lo,
                                                       const double* __restrict__ wlo, const double* __restrict__ a_grid,
                                                       double* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double* ag = a_grid + ((i / N) % n_cal) * (size_t)n_a;
    int j = lo[i];
    j = j < 0 ? 0 : j;
    j = j > n_a - 2 ? n_a - 2 : j;
    const double wl = wlo[i];
    out[i] = wl * ag[j] + (1.0 - wl) * ag[j + 1];
  }
}

}  // namespace aiy

using namespace aiy;

extern "C" int32_t aiy_lottery_mean(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t n_t, const int32_t* lo,
                                    const double* wlo, const double* a_grid, double* out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a);
  if (rc) return rc;
  if (n_t < 1) return fail(h, AIY_ERR_ARG, "n_t=%d must be >= 1", n_t);
  if (!lo || !wlo || !a_grid || !out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const size_t N = (size_t)S * n_a, n = (size_t)n_t * n_cal * N;
  const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 20);
  hipLaunchKernelGGL(agg_mean_kernel, dim3(nb), dim3(256), 0, st, n, N, n_cal, n_a, lo, wlo, a_grid, out);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_aggregate_lotteries(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_p,
                                           const double* a_star, const double* dA_R, const double* dA_w,
                                           const double* X, const double* a_grid, int32_t* lo_out, double* wlo_out,
                                           aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a, true, T, T <= kAggMaxT);
  if (rc) return rc;
  if (n_p < 1 || n_p > 65535 * kAggTile) return fail(h, AIY_ERR_ARG, "n_p=%d outside 1..%d", n_p, 65535 * kAggTile);
  if (!a_star || !dA_R || !dA_w || !X || !a_grid || !lo_out || !wlo_out) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  AggSyn A;
  A.n_cal = n_cal; A.n_a = n_a; A.T = T; A.n_p = n_p; A.K2 = 2 * (T + 1);
  A.N = (size_t)S * n_a;
  A.a_star = a_star; A.dA_R = dA_R; A.dA_w = dA_w; A.X = X; A.a_grid = a_grid;
  A.lo = lo_out; A.wlo = wlo_out;
  const int ptile = kAggTile * kAggPT;
  const dim3 grid((unsigned)((A.N + kAggTile - 1) / kAggTile), (unsigned)((n_p + ptile - 1) / ptile), n_cal);
  hipLaunchKernelGGL(agg_lottery_kernel, grid, dim3(kAggBlock), 0, st, A);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}
