// Statistics of any household variable on the histogram for gfx950.  A variable
// y[s][j] that is nondecreasing in assets within every income state makes a distribution S sorted
// runs: ordering it is an S-way merge, not a sort, and the merged distribution is a marginal of
// N = S n_a nodes on its own ascending "grid" that aiy_dist_stats (dist_stats.hip) takes as it is.
//
//   vs_variables_kernel  consumption, income, earnings, cash on hand, saving and wealth of every
//                        node of a stack of lotteries, element by element, each written with the
//                        operations of its NumPy expression (the build has -ffp-contract=off).
//   vs_check_kernel      one thread per neighbouring pair of a run: a pair that is not
//                        key[j - 1] <= key[j] (a decreasing pair, or a NaN on either side) raises
//                        the flag the host waits for before anything is written.
//   vs_merge_kernel      thread k of a block owns kVsChunk consecutive nodes of one run and keeps
//                        their keys and their ranks in registers.  For every other run it does one
//                        binary search, at the chunk's first key, and from there only advances one
//                        pointer through that run while it walks its own keys, because both move
//                        one way; the pointer's value at a key is the count that key's rank takes
//                        from that run.  rank(s, j) = j + sum over s' < s of #{key[s'] <= y} + sum
//                        over s' > s of #{key[s'] < y}: np.argsort(kind="stable")'s order.  Every
//                        output element is a copy of an input element at its rank.
//   vs_moments_kernel    one workgroup per distribution, two passes in one launch: the sums of w
//                        and w y_u, then the centred products w (y_u - m_u)(y_v - m_v).  A row
//                        (d, s) is summed in row_chunk chunks reduced by row_block_sum, the rows
//                        in ascending s.
// No atomics, no sort library.  Offsets are size_t.
#include "common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>
#include <vector>

namespace aiy {

constexpr int kVsChunk = 16;                      // nodes of a run per thread of the merge
constexpr int kVsSpan = kTrBlock * kVsChunk;      // nodes of a run per block
constexpr int kVsMaxVars = AIY_VAR_MAX_MOMENTS;   // variables of one aiy_var_moments call
constexpr int kVsPairs = kVsMaxVars * (kVsMaxVars + 1) / 2;
constexpr int kVsKinds = 6;                       // AIY_VAR_CONSUMPTION .. AIY_VAR_WEALTH

// ---------------------------------------------------------------------------------
// The variables
// ---------------------------------------------------------------------------------
struct VsVarArgs {
  size_t n, N, per;   // n: elements of one variable; N = S n_a; per = n_cal N
  int n_cal, S, n_a, ld_price, mask;
  const int* lo;
  const double *wlo, *R, *w, *a_grid, *lab;
  double* out;        // the variables of the mask, in ascending bit order, n elements each
};

__global__ __launch_bounds__(256) void vs_variables_kernel(VsVarArgs A) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride) {
    const size_t t = i / A.per, c = (i / A.N) % A.n_cal, r = i % A.N;
    const int s = (int)(r / A.n_a), j = (int)(r % A.n_a);
    const double* ag = A.a_grid + c * (size_t)A.n_a;
    const double aj = ag[j];
    const double Rt = A.R[c * (size_t)A.ld_price + t], wt = A.w[c * (size_t)A.ld_price + t];
    const double ls = wt * A.lab[c * (size_t)A.S + s];
    double ad = 0.0;   // the lottery's savings
    if (A.mask & (AIY_VAR_CONSUMPTION | AIY_VAR_SAVING)) {
      int d = A.lo[i];
      d = d < 0 ? 0 : d;
      d = d > A.n_a - 2 ? A.n_a - 2 : d;
      const double wl = A.wlo[i];
      ad = wl * ag[d] + (1.0 - wl) * ag[d + 1];
    }
    double* o = A.out + i;
    if (A.mask & AIY_VAR_CONSUMPTION) { *o = (Rt * aj + ls) - ad; o += A.n; }
    if (A.mask & AIY_VAR_INCOME) { *o = (Rt - 1.0) * aj + ls; o += A.n; }
    if (A.mask & AIY_VAR_EARNINGS) { *o = ls; o += A.n; }
    if (A.mask & AIY_VAR_CASH) { *o = Rt * aj + ls; o += A.n; }
    if (A.mask & AIY_VAR_SAVING) { *o = ad - aj; o += A.n; }
    if (A.mask & AIY_VAR_WEALTH) { *o = aj; }
  }
}

// ---------------------------------------------------------------------------------
// The merge
// ---------------------------------------------------------------------------------
// The pair (j - 1, j), j = 1 .. n_a - 1, of every run of the stack (n_a >= 2: every key is in a pair).
__global__ __launch_bounds__(256) void vs_check_kernel(size_t n, int n_a, const double* __restrict__ key, int* flag) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i % n_a == 0) continue;
    if (!(key[i - 1] <= key[i])) *flag = 1;   // every writer stores the same word
  }
}

// First p in [0, n) with K[p] > y (UPPER) or K[p] >= y, n if none.
template <bool UPPER>
__device__ __forceinline__ int vs_bound(const double* K, int n, double y) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const double v = K[mid];
    if (UPPER ? (v <= y) : (v < y)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct VsMergeArgs {
  int S, n_a;
  const double *key, *weight;   // [n_dist][S][n_a]
  double *key_sorted, *weight_sorted;   // [n_dist][S n_a]
  int* rank;                    // [n_dist][S][n_a] or null
};

// grid (blocks of kVsSpan nodes, S, distributions)
__global__ __launch_bounds__(kTrBlock) void vs_merge_kernel(VsMergeArgs A) {
  const int n = A.n_a, S = A.S, s = blockIdx.y;
  const size_t dist = blockIdx.z, N = (size_t)S * n;
  const double* K = A.key + dist * N;
  const int j0 = (blockIdx.x * kTrBlock + threadIdx.x) * kVsChunk;   // < n_a + kVsSpan
  if (j0 >= n) return;
  const int cnt = n - j0 < kVsChunk ? n - j0 : kVsChunk;
  const double* Ks = K + (size_t)s * n;
  double y[kVsChunk];
  int rk[kVsChunk];
#pragma unroll
  for (int e = 0; e < kVsChunk; ++e) {
    y[e] = Ks[j0 + (e < cnt ? e : cnt - 1)];   // the tail repeats the last key: its ranks are dropped
    rk[e] = j0 + e;
  }
#pragma unroll 1
  for (int q = 0; q < S; ++q) {
    if (q == s) continue;
    const double* Kq = K + (size_t)q * n;
    const bool upper = q < s;   // an earlier run goes first on a tie: count its keys <= y
    int p = upper ? vs_bound<true>(Kq, n, y[0]) : vs_bound<false>(Kq, n, y[0]);
    double head = p < n ? Kq[p] : 0.0;
#pragma unroll
    for (int e = 0; e < kVsChunk; ++e) {
      while (p < n && (upper ? head <= y[e] : head < y[e])) {
        ++p;
        head = p < n ? Kq[p] : 0.0;
      }
      rk[e] += p;
    }
  }
  const double* W = A.weight + dist * N + (size_t)s * n;
  double* ko = A.key_sorted + dist * N;
  double* wo = A.weight_sorted + dist * N;
#pragma unroll
  for (int e = 0; e < kVsChunk; ++e) {
    if (e < cnt) {
      ko[rk[e]] = y[e];
      wo[rk[e]] = W[j0 + e];
      if (A.rank) A.rank[dist * N + (size_t)s * n + j0 + e] = rk[e];
    }
  }
}

// ---------------------------------------------------------------------------------
// The moments
// ---------------------------------------------------------------------------------
struct VsMomArgs {
  int S, n_a, n_v;
  const double* w;               // [n_dist][S][n_a]
  const double* y[kVsMaxVars];   // each [n_dist][S][n_a]; the entries past n_v repeat y[0]
  double* out;                   // [n_dist][1 + n_v + n_v n_v]
};

__global__ __launch_bounds__(kTrBlock) void vs_moments_kernel(VsMomArgs A) {
  const int n = A.n_a, S = A.S, nv = A.n_v, k = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * S * n;
  __shared__ double s_wave[kVsPairs][kTrWaves];
  __shared__ double s_mean[kVsMaxVars + 1];
  int j0, j1;
  row_chunk(n, k, j0, j1);

  double tot[kVsMaxVars + 1];   // thread 0: sum w, sum w y_u
#pragma unroll
  for (int q = 0; q <= kVsMaxVars; ++q) tot[q] = 0.0;
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const size_t row = base + (size_t)s * n;
    double acc[kVsMaxVars + 1];
#pragma unroll
    for (int q = 0; q <= kVsMaxVars; ++q) acc[q] = 0.0;
    for (int j = j0; j < j1; ++j) {
      const double wj = A.w[row + j];
      acc[0] += wj;
#pragma unroll
      for (int u = 0; u < kVsMaxVars; ++u)
        if (u < nv) acc[1 + u] += wj * A.y[u][row + j];
    }
#pragma unroll
    for (int q = 0; q <= kVsMaxVars; ++q)
      if (q <= nv) tot[q] += row_block_sum(acc[q], s_wave[q]);   // block-uniform: nv is
    __syncthreads();   // s_wave is free for the next row
  }
  if (k == 0) {
    s_mean[0] = tot[0];
#pragma unroll
    for (int u = 0; u < kVsMaxVars; ++u) s_mean[1 + u] = tot[1 + u] / tot[0];
  }
  __syncthreads();
  double m[kVsMaxVars];
#pragma unroll
  for (int u = 0; u < kVsMaxVars; ++u) m[u] = s_mean[1 + u];
  const double sw = s_mean[0];

  double cov[kVsPairs];   // thread 0: sum w (y_u - m_u)(y_v - m_v), u <= v
#pragma unroll
  for (int q = 0; q < kVsPairs; ++q) cov[q] = 0.0;
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const size_t row = base + (size_t)s * n;
    double acc[kVsPairs];
#pragma unroll
    for (int q = 0; q < kVsPairs; ++q) acc[q] = 0.0;
    for (int j = j0; j < j1; ++j) {
      const double wj = A.w[row + j];
      double d[kVsMaxVars];
#pragma unroll
      for (int u = 0; u < kVsMaxVars; ++u) d[u] = u < nv ? A.y[u][row + j] - m[u] : 0.0;
      int q = 0;
#pragma unroll
      for (int u = 0; u < kVsMaxVars; ++u)
#pragma unroll
        for (int v = u; v < kVsMaxVars; ++v, ++q)
          if (v < nv) acc[q] += wj * (d[u] * d[v]);
    }
    int q = 0;
#pragma unroll
    for (int u = 0; u < kVsMaxVars; ++u)
#pragma unroll
      for (int v = u; v < kVsMaxVars; ++v, ++q)
        if (v < nv) cov[q] += row_block_sum(acc[q], s_wave[q]);
    __syncthreads();
  }
  if (k == 0) {
    double* out = A.out + (size_t)blockIdx.x * (1 + nv + nv * nv);
    out[0] = sw;
    int q = 0;
#pragma unroll
    for (int u = 0; u < kVsMaxVars; ++u) {
      if (u < nv) out[1 + u] = m[u];
#pragma unroll
      for (int v = u; v < kVsMaxVars; ++v, ++q)
        if (v < nv) {
          const double c = cov[q] / sw;
          out[1 + nv + u * nv + v] = c;
          out[1 + nv + v * nv + u] = c;
        }
    }
  }
}

// Work space (caller-owned): [the check's flag][the moments of every distribution], every region
// on a 256-byte boundary.
struct VsWork {
  int* flag;
  double* mom;
  size_t bytes;
};
static bool vs_sizes_ok(int n_dist, int S, int n_a) {
  return n_dist >= 1 && S >= 1 && S <= AIY_MAX_STATES && n_a >= 2 && (long long)S * n_a < 2147483647LL &&
         n_a < 2147483647 - kVsSpan;
}
static VsWork vs_work(Carve c, int n_dist, int S, int n_a) {
  (void)S; (void)n_a;
  VsWork L;
  L.flag = c.take<int>(256 / sizeof(int));
  L.mom = c.take<double>((size_t)n_dist * (1 + kVsMaxVars + kVsMaxVars * kVsMaxVars));
  L.bytes = c.bytes();
  return L;
}

static int32_t vs_check_sizes(aiy_handle* h, int n_dist, int S, int n_a) {
  if (n_dist < 1 || n_a < 2) return fail(h, AIY_ERR_ARG, "bad sizes n_dist=%d n_a=%d", n_dist, n_a);
  if (S < 1 || S > AIY_MAX_STATES) return fail(h, AIY_ERR_ARG, "S=%d outside 1..%d", S, AIY_MAX_STATES);
  if (!vs_sizes_ok(n_dist, S, n_a)) return fail(h, AIY_ERR_ARG, "bad sizes n_dist=%d S=%d n_a=%d", n_dist, S, n_a);
  return AIY_OK;
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_var_work_bytes(int32_t n_dist, int32_t S, int32_t n_a) {
  if (!vs_sizes_ok(n_dist, S, n_a)) return -1;
  return (int64_t)vs_work(Carve(), n_dist, S, n_a).bytes;
}

extern "C" int32_t aiy_household_variables(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t n_t,
                                           const int32_t* lo, const double* wlo, const double* R, const double* w,
                                           int32_t ld_price, const double* a_grid, const double* lab, int32_t which,
                                           double* out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a);
  if (rc) return rc;
  if (n_t < 1 || ld_price < n_t) return fail(h, AIY_ERR_ARG, "n_t=%d must be >= 1 and ld_price=%d >= n_t", n_t, ld_price);
  if (which < 1 || which >= (1 << kVsKinds)) return fail(h, AIY_ERR_ARG, "which=%d names no variable", which);
  if (!R || !w || !a_grid || !lab || !out) return fail(h, AIY_ERR_ARG, "null buffer");
  if ((which & (AIY_VAR_CONSUMPTION | AIY_VAR_SAVING)) && (!lo || !wlo))
    return fail(h, AIY_ERR_ARG, "consumption and saving need lo and wlo");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  VsVarArgs A;
  A.N = (size_t)S * n_a; A.per = (size_t)n_cal * A.N; A.n = (size_t)n_t * A.per;
  A.n_cal = n_cal; A.S = S; A.n_a = n_a; A.ld_price = ld_price; A.mask = which;
  A.lo = lo; A.wlo = wlo; A.R = R; A.w = w; A.a_grid = a_grid; A.lab = lab; A.out = out;
  const unsigned nb = (unsigned)std::min<size_t>((A.n + 255) / 256, (size_t)1 << 20);
  hipLaunchKernelGGL(vs_variables_kernel, dim3(nb), dim3(256), 0, st, A);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_var_merge(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, const double* key,
                                 const double* weight, void* work, double* key_sorted, double* weight_sorted,
                                 int32_t* rank_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = vs_check_sizes(h, n_dist, S, n_a);
  if (rc) return rc;
  if (!key || !weight || !work || !key_sorted || !weight_sorted) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const VsWork L = vs_work(Carve(work), n_dist, S, n_a);
  const size_t n = (size_t)n_dist * S * n_a;
  AIY_HIP(h, hipMemsetAsync(L.flag, 0, sizeof(int), st));
  const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 20);
  hipLaunchKernelGGL(vs_check_kernel, dim3(nb), dim3(256), 0, st, n, n_a, key, L.flag);
  AIY_CHECK_LAUNCH(h);
  int flag = 0;
  AIY_HIP(h, hipMemcpyAsync(&flag, L.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  if (flag != 0)
    return fail(h, AIY_ERR_UNSUPPORTED,
                "variable merge check failed: a run of key is not nondecreasing in assets or holds a NaN");
  VsMergeArgs A;
  A.S = S; A.n_a = n_a;
  const unsigned nx = (unsigned)((n_a + kVsSpan - 1) / kVsSpan);
  for (int d0 = 0; d0 < n_dist; d0 += 65535) {   // grid.z <= 65535
    const unsigned nz = (unsigned)std::min(65535, n_dist - d0);
    const size_t off = (size_t)d0 * S * n_a;
    A.key = key + off; A.weight = weight + off;
    A.key_sorted = key_sorted + off; A.weight_sorted = weight_sorted + off;
    A.rank = rank_out ? rank_out + off : nullptr;
    hipLaunchKernelGGL(vs_merge_kernel, dim3(nx, S, nz), dim3(kTrBlock), 0, st, A);
  }
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_var_moments(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, int32_t n_v,
                                   const double* const* vars, const double* weight, void* work, double* out,
                                   aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = vs_check_sizes(h, n_dist, S, n_a);
  if (rc) return rc;
  if (n_v < 1 || n_v > kVsMaxVars) return fail(h, AIY_ERR_ARG, "n_v=%d outside 1..%d", n_v, kVsMaxVars);
  if (!vars || !weight || !work || !out) return fail(h, AIY_ERR_ARG, "null buffer");
  for (int u = 0; u < n_v; ++u)
    if (!vars[u]) return fail(h, AIY_ERR_ARG, "null variable %d", u);
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const VsWork L = vs_work(Carve(work), n_dist, S, n_a);
  VsMomArgs A;
  A.S = S; A.n_a = n_a; A.n_v = n_v;
  A.w = weight;
  for (int u = 0; u < kVsMaxVars; ++u) A.y[u] = vars[u < n_v ? u : 0];
  A.out = L.mom;
  hipLaunchKernelGGL(vs_moments_kernel, dim3((unsigned)n_dist), dim3(kTrBlock), 0, st, A);
  AIY_CHECK_LAUNCH(h);
  const size_t n_out = (size_t)n_dist * (1 + n_v + n_v * n_v);
  AIY_HIP(h, hipMemcpyAsync(out, L.mom, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  return AIY_OK;
}
