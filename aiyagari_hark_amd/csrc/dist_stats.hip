// Wealth statistics of histogram distributions for gfx950: Gini coefficient,
// Lorenz shares, percentiles, mean, total and the share on the lowest node of a stack of
// marginals g[n_dist][n_a] over the ascending asset grid -- the stationary masses of a batch, or
// the (T + 1) x n_cal period marginals of a transition path.  The grid is sorted, so there is no
// sort: per distribution
//   cw = cumsum(g), cd = cumsum(a g), F = cw / cw[-1], L = cd / cd[-1],
//   lorenz(p)     = np.interp(p, F, L)                       (HARK get_lorenz_shares, presorted)
//   percentile(p) = interp1d(F, a, bounds_error=False)(p)    (HARK get_percentiles, presorted)
//   gini          = 1 - sum_j (F[j] - F[j-1]) (L[j] + L[j-1]),  F[-1] = L[-1] = 0.
//
//   dist_stats_kernel   one workgroup of 256 threads per distribution, one launch per stack.
//                       Thread k owns its row_chunk (transition_common.h).  Pass 1: the chunk's sums
//                       of g and a g, sequentially.  The 256 chunk totals get an exclusive scan
//                       in a fixed order: an inclusive shuffle scan per wave, then the waves in
//                       ascending order through LDS.  Pass 2: cw[j] / cd[j] = the chunk's base +
//                       its running sequential sum, written to the work space [n_dist][2][n_a],
//                       and the thread's Gini terms (a chunk's first term takes the previous
//                       chunk's last cw, cd = that chunk's base + total); the Gini partials are
//                       summed by row_block_sum (as value_reduce_kernel's).  After its barrier
//                       threads 0 .. n_p - 1 do the two searches of stats_interp_kernel
//                       (stats.hip) on cw, cd with sorted = a_grid, reading only the bracketing
//                       entries; thread 0 writes the summary.
// No atomics.  Every sum order is a function of (n_a, 256) only -- not of n_dist, the position
// in the stack, the CU count or timing: a distribution has the same bits alone and in a stack.
#include "common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <vector>

namespace aiy {

constexpr int kDsBlock = kTrBlock;
constexpr int kDsWaves = kTrWaves;
constexpr int kDsMaxPct = 256;
constexpr int kDsSummary = 4;   // total, mean, gini, bottom_share

struct DsArgs {
  int n_grid, n_a, n_p;
  const double* g;        // [n_dist][n_a]
  const double* a_grid;   // [n_grid][n_a]
  const double* pct;      // [n_p] (work)
  double* cum;            // [n_dist][2][n_a]: cw | cd (work)
  double* lorenz;         // [n_dist][n_p] (work)
  double* pctl;           // [n_dist][n_p]
  double* summary;        // [n_dist][kDsSummary]
};

// Inclusive sum over the lanes 0 .. lane of the wave (shuffle scan, the same order in every lane
// of every launch).
__device__ __forceinline__ double ds_wave_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// cum_dist[k] = cw[k] / cw[n - 1] (tot, held in a register) and its two searches, as stats.hip's
// cum_dist_at / cd_search with weights: first k in [0, n) with cum_dist[k] > p ('right') or
// >= p ('left').
__device__ __forceinline__ double ds_cum_dist(const double* cw, double tot, int k) { return cw[k] / tot; }
__device__ __forceinline__ int ds_search(const double* cw, double tot, int n, double p, bool right) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const double v = ds_cum_dist(cw, tot, mid);
    if (right ? (v <= p) : (v < p)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kDsBlock) void dist_stats_kernel(DsArgs A) {
  const int n = A.n_a, k = threadIdx.x;
  const size_t dist = blockIdx.x;
  const int lane = k & (kWave - 1), wid = k / kWave;
  const double* __restrict__ g = A.g + dist * n;
  const double* __restrict__ a = A.a_grid + (size_t)(dist % A.n_grid) * n;
  double* cw = A.cum + dist * 2 * n;
  double* cd = cw + n;
  __shared__ double s_wave[3][kDsWaves];   // wave totals of g, a g; Gini partials
  __shared__ double s_lw[kDsBlock];        // last cw of every chunk
  __shared__ double s_ld[kDsBlock];        // last cd

  int j0, j1;
  const int chunk = row_chunk(n, k, j0, j1);

  double tw = 0.0, td = 0.0;   // pass 1: the chunk's totals
  for (int j = j0; j < j1; ++j) {
    const double gj = g[j];
    tw += gj;
    td += a[j] * gj;
  }
  // exclusive scan of the chunk totals: lanes, then the waves in ascending order
  const double iw = ds_wave_scan(tw, lane), id = ds_wave_scan(td, lane);
  if (lane == kWave - 1) {
    s_wave[0][wid] = iw;
    s_wave[1][wid] = id;
  }
  __syncthreads();
  double bw = 0.0, bd = 0.0;
  for (int q = 0; q < wid; ++q) {
    bw += s_wave[0][q];
    bd += s_wave[1][q];
  }
  const double ew = __shfl_up(iw, 1, kWave), ed = __shfl_up(id, 1, kWave);
  bw += lane > 0 ? ew : 0.0;
  bd += lane > 0 ? ed : 0.0;
  s_lw[k] = bw + tw;   // the chunk's last cw: pass 2 adds the same terms in the same order
  s_ld[k] = bd + td;
  __syncthreads();
  const int kl = (n - 1) / chunk;   // the chunk of node n - 1
  const double totw = s_lw[kl], totd = s_ld[kl];

  // pass 2: cw, cd and the Gini terms (F[j] - F[j-1]) (L[j] + L[j-1])
  double Fp = 0.0, Lp = 0.0;
  if (k > 0) {
    Fp = s_lw[k - 1] / totw;
    Lp = s_ld[k - 1] / totd;
  }
  double rw = 0.0, rd = 0.0, gacc = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double gj = g[j];
    rw += gj;
    rd += a[j] * gj;
    const double cwj = bw + rw, cdj = bd + rd;
    cw[j] = cwj;
    cd[j] = cdj;
    const double F = cwj / totw, L = cdj / totd;
    gacc += (F - Fp) * (L + Lp);
    Fp = F;
    Lp = L;
  }
  const double area = row_block_sum(gacc, s_wave[2]);   // its barrier: the block's cw, cd are written

  if (k < A.n_p) {
    const double p = A.pct[k];
    // np.interp(p, xp = F, fp = L)
    {
      const double x0 = ds_cum_dist(cw, totw, 0), xl = ds_cum_dist(cw, totw, n - 1);
      double r;
      if (p < x0) {
        r = cd[0] / totd;
      } else if (p >= xl) {
        r = cd[n - 1] / totd;
      } else {
        int j = ds_search(cw, totw, n, p, true) - 1;   // xp[j] <= p < xp[j + 1]
        j = j < 0 ? 0 : (j > n - 2 ? n - 2 : j);  // (a NaN cum_dist: stay inside the row)
        const double xj = ds_cum_dist(cw, totw, j), xj1 = ds_cum_dist(cw, totw, j + 1);
        const double yj = cd[j] / totd, yj1 = cd[j + 1] / totd;
        if (p == xj) {
          r = yj;
        } else {
          const double slope = (yj1 - yj) / (xj1 - xj);
          r = slope * (p - xj) + yj;
          if (r != r) {                            // numpy's NaN retry
            r = slope * (p - xj1) + yj1;
            if (r != r && yj == yj1) r = yj;
          }
        }
      }
      A.lorenz[dist * A.n_p + k] = r;
    }
    // scipy interp1d(F, a, bounds_error=False): NaN outside [F[0], F[-1]]
    {
      const double x0 = ds_cum_dist(cw, totw, 0), xl = ds_cum_dist(cw, totw, n - 1);
      double r = __builtin_nan("");
      if (!(p < x0) && !(p > xl)) {
        int hi = ds_search(cw, totw, n, p, false);       // searchsorted(x, p) (left)
        hi = hi < 1 ? 1 : (hi > n - 1 ? n - 1 : hi);
        const int lo = hi - 1;
        const double xa = ds_cum_dist(cw, totw, lo), xb = ds_cum_dist(cw, totw, hi);
        const double slope = (a[hi] - a[lo]) / (xb - xa);
        r = slope * (p - xa) + a[lo];
      }
      A.pctl[dist * A.n_p + k] = r;
    }
  }
  if (k == 0) {
    double* out = A.summary + dist * kDsSummary;
    out[0] = totw;
    out[1] = totd / totw;
    out[2] = 1.0 - area;
    out[3] = g[0] / totw;
  }
}

// Work space (caller-owned): [cw | cd of every distribution][percentiles][results], every
// region on a 256-byte boundary; the results region holds kDsMaxPct percentiles.
struct DsWork {
  double *cum, *pct, *res;
  size_t bytes;
};
static bool ds_sizes_ok(int n_dist, int n_a) { return n_dist >= 1 && n_a >= 2; }
static DsWork ds_work(Carve c, int n_dist, int n_a) {
  DsWork L;
  L.cum = c.take<double>((size_t)n_dist * 2 * n_a);
  L.pct = c.take<double>(kDsMaxPct);
  L.res = c.take<double>((size_t)n_dist * (2 * kDsMaxPct + kDsSummary));
  L.bytes = c.bytes();
  return L;
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_dist_stats_work_bytes(int32_t n_dist, int32_t n_a) {
  if (!ds_sizes_ok(n_dist, n_a)) return -1;
  return (int64_t)ds_work(Carve(), n_dist, n_a).bytes;
}

extern "C" int32_t aiy_dist_marginal(aiy_handle* h, int32_t n_dist, int32_t S, int32_t n_a, const double* mass,
                                     double* g, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (n_dist < 1 || n_a < 2) return fail(h, AIY_ERR_ARG, "bad sizes n_dist=%d n_a=%d", n_dist, n_a);
  if (S < 1 || S > AIY_MAX_STATES) return fail(h, AIY_ERR_ARG, "S=%d outside 1..%d", S, AIY_MAX_STATES);
  if (!mass || !g) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  tr_launch_marginal(n_dist, S, n_a, mass, g, st);
  AIY_CHECK_LAUNCH(h);
  return AIY_OK;
}

extern "C" int32_t aiy_dist_stats(aiy_handle* h, int32_t n_dist, int32_t n_grid, int32_t n_a, const double* g,
                                  const double* a_grid, const double* pctiles, int32_t n_p, void* work,
                                  double* lorenz_out, double* pctl_out, double* summary_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (!ds_sizes_ok(n_dist, n_a) || n_grid < 1)
    return fail(h, AIY_ERR_ARG, "bad sizes n_dist=%d n_grid=%d n_a=%d", n_dist, n_grid, n_a);
  if (n_p < 0 || (n_p > 0 && !pctiles)) return fail(h, AIY_ERR_ARG, "null pctiles or n_p < 0");
  if (n_p > kDsMaxPct) return fail(h, AIY_ERR_UNSUPPORTED, "n_p=%d exceeds %d", n_p, kDsMaxPct);
  for (int i = 0; i < n_p; ++i)
    if (!(pctiles[i] > 0.0 && pctiles[i] < 1.0)) return fail(h, AIY_ERR_ARG, "percentiles must lie in (0, 1)");
  if (!g || !a_grid || !work) return fail(h, AIY_ERR_ARG, "null buffer");
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  const DsWork L = ds_work(Carve(work), n_dist, n_a);
  const size_t n_res = (size_t)n_dist * n_p;
  double* d_res = L.res;   // lorenz | percentiles | summary, packed
  DsArgs A;
  A.n_grid = n_grid; A.n_a = n_a; A.n_p = n_p;
  A.g = g; A.a_grid = a_grid;
  A.pct = L.pct;
  A.cum = L.cum;
  A.lorenz = d_res;
  A.pctl = d_res + n_res;
  A.summary = d_res + 2 * n_res;
  if (n_p > 0)
    AIY_HIP(h, hipMemcpyAsync(L.pct, pctiles, n_p * sizeof(double), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dist_stats_kernel, dim3((unsigned)n_dist), dim3(kDsBlock), 0, st, A);
  AIY_CHECK_LAUNCH(h);
  std::vector<double> res(2 * n_res + (size_t)n_dist * kDsSummary);   // heap: n_dist x n_p results
  AIY_HIP(h, hipMemcpyAsync(res.data(), d_res, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  if (lorenz_out && n_res) std::memcpy(lorenz_out, res.data(), n_res * sizeof(double));
  if (pctl_out && n_res) std::memcpy(pctl_out, res.data() + n_res, n_res * sizeof(double));
  if (summary_out) std::memcpy(summary_out, res.data() + 2 * n_res, (size_t)n_dist * kDsSummary * sizeof(double));
  return AIY_OK;
}
