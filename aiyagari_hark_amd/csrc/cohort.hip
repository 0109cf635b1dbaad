// Cohorts on the forward sweep for gfx950: G masses -- the restrictions of one
// distribution to G groups of households -- pushed through ONE lottery per period, with the
// occupancy of every period by wealth class and by income state.  The lotteries define the Markov
// chain on (s, a_j) exactly, so a cohort's later mass is its exact later distribution.
//
//   co_first_kernel     period 0, the cohorts as given: K_g[0] with tr_K0_kernel's column
//                       partition and order, and the occupancy partials of the block's columns.
//   co_forward_kernel   grid (64-column blocks, calibrations, chunks of GC cohorts), one launch
//                       per period.  tr_pull_multi (transition_common.h) of every (s, column) for
//                       the chunk's GC masses into the LDS tile [GC][S][64] -- the index and the
//                       weights are read once, only the masses multiply -- then tr_mix_forward per
//                       cohort, the K and C block sums by tr_block_sum: cohort by cohort the
//                       operations and their order are tr_forward_kernel's, so mass, K and C have
//                       the bits of aiy_transition_forward on that cohort alone, whatever the
//                       chunking.  No atomics.
//   co_tail             (both kernels) the two occupancy reductions of what the block holds:
//                       inc: a wave owns a state's row of the block, wave_sum_fixed over its 64
//                            columns;
//                       occ: a lane adds its column over the wave's states (ascending), the four
//                            waves' column sums meet in LDS, and thread (cohort, class) adds
//                            ((w0 + w1) + w2) + w3 of the block's columns inside the class in
//                            ascending order.
//   co_sum_kernel       the blocks' partials of K, C, occ and inc in block order.  The partials
//                       live in a ring of a few periods (CoWork), folded whenever it is full.
//
// The orders depend on (S, n_a, edges) only: not on G, the chunking, the batch or the device.
#include "common.h"
#include "hist_cluster.h"
#include "internal.h"
#include "transition_common.h"

#include <algorithm>

namespace aiy {

constexpr int kCoMaxGC = 8;             // cohorts a thread carries in registers
constexpr int kCoTileRows = 128;        // GC S <= 128: the tile [GC][S][64] doubles stays within 64 KB
constexpr int kCoRing = 8;              // periods of partials a work space holds at most

struct CoFwd {
  int n_cal, S, n_a, T, n_lot, G, Q, nblk, X, ring;   // X = 2 + Q + S values per (period, cal, cohort)
  size_t gstride;        // n_cal S n_a: one cohort
  const double* wlo;     // [n_lot][n_cal][S][n_a]
  const int* jb;         // [n_lot][n_cal][S][n_a + 1]
  const double* P;       // [n_cal][S][S]
  const double* a_grid;  // [n_cal][n_a]
  const double* R;       // [n_cal][T + 1] (WITH_C)
  const double* w;
  const double* lab;     // [n_cal][S]
  const int* edges;      // [n_cal][Q + 1], checked on the host
  double* part;          // [ring][n_cal][G][X][nblk]: K, C, occ[Q], inc[S] of period p in slot p % ring
};

// The block partials of value x of (period p, cal, cohort g).
__device__ __forceinline__ double* co_part(const CoFwd& A, int p, int cal, int g, int x) {
  return A.part + ((((size_t)(p % A.ring) * A.n_cal + cal) * A.G + g) * A.X + x) * A.nblk;
}

// Doubles of dynamic LDS: the tile, or the tail's column sums [GC][kTrWaves][64] and the block
// sums' kTrWaves words behind them, whichever is longer.
inline size_t co_lds_doubles(int GC, int S) {
  return std::max((size_t)GC * S * kTrCols, (size_t)GC * kTrWaves * kTrCols + kTrWaves);
}

// inc of one state's row of the block (the wave's lanes hold v, 0 past n_a): lane 0 writes.
__device__ __forceinline__ void co_inc(const CoFwd& A, const TrPlace& p, int period, int g, int s, double v) {
  const double r = wave_sum_fixed(v);
  if (p.lane == 0) co_part(A, period, p.cal, g, 2 + A.Q + s)[blockIdx.x] = r;
}

// occ of the block's columns and the K (and C) block sums.  colp[g]: the lane's column summed
// over the wave's states; L: the LDS, which no thread reads as a tile any more once every thread
// has arrived here.
template <int GC, bool WITH_C>
__device__ __forceinline__ void co_tail(const CoFwd& A, const TrPlace& p, int period, int g0, int ng,
                                        const double (&colp)[GC], const double (&kacc)[GC], const double (&cacc)[GC],
                                        double* L) {
  __syncthreads();
#pragma unroll
  for (int g = 0; g < GC; ++g) L[(g * kTrWaves + p.wave) * kTrCols + p.lane] = colp[g];
  __syncthreads();
  const int c0 = blockIdx.x * kTrCols;
  const int* E = A.edges + (size_t)p.cal * (A.Q + 1);
  for (int i = threadIdx.x; i < ng * A.Q; i += kTrBlock) {
    const int g = i / A.Q, q = i - g * A.Q;
    const int e0 = E[q], e1 = E[q + 1];   // e1 <= n_a: columns past the grid are in no class
    const int lo = (e0 > c0 ? e0 : c0) - c0, hi = (e1 < c0 + kTrCols ? e1 : c0 + kTrCols) - c0;
    const double* W = L + g * kTrWaves * kTrCols;
    double v = 0.0;
    for (int c = lo; c < hi; ++c)
      v += ((W[c] + W[kTrCols + c]) + W[2 * kTrCols + c]) + W[3 * kTrCols + c];
    co_part(A, period, p.cal, g0 + g, 2 + q)[blockIdx.x] = v;
  }
  double* red = L + GC * kTrWaves * kTrCols;
#pragma unroll
  for (int g = 0; g < GC; ++g) {
    const double k = tr_block_sum(kacc[g], red);
    if (threadIdx.x == 0 && g < ng) co_part(A, period, p.cal, g0 + g, 0)[blockIdx.x] = k;
    if constexpr (WITH_C) {
      const double c = tr_block_sum(cacc[g], red);
      if (threadIdx.x == 0 && g < ng) co_part(A, period, p.cal, g0 + g, 1)[blockIdx.x] = c;
    }
  }
}

template <int GC>
__global__ __launch_bounds__(kTrBlock) void co_first_kernel(CoFwd A, const double* __restrict__ mass) {
  extern __shared__ double co_lds[];
  const int S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  const int g0 = blockIdx.z * GC, ng = A.G - g0 < GC ? A.G - g0 : GC;
  const int d = p.col;
  const double ad = A.a_grid[(size_t)p.cal * n_a + (p.active ? d : n_a - 1)];
  double kacc[GC], colp[GC], none[GC];
#pragma unroll
  for (int g = 0; g < GC; ++g) kacc[g] = colp[g] = none[g] = 0.0;
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves) {
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      if (g < ng) {   // block-uniform
        double m = 0.0;
        if (p.active) {
          m = mass[(size_t)(g0 + g) * A.gstride + (p.rows + s) * (size_t)n_a + d];
          kacc[g] += m * ad;   // tr_K0_kernel's term and order
          colp[g] += m;
        }
        co_inc(A, p, 0, g0 + g, s, m);
      }
    }
  }
  co_tail<GC, false>(A, p, 0, g0, ng, colp, kacc, none, co_lds);
}

template <int GC, bool WITH_C>
__global__ __launch_bounds__(kTrBlock) void co_forward_kernel(CoFwd A, int t, const double* __restrict__ mass,
                                                              double* __restrict__ mass_out) {
  extern __shared__ double co_lds[];   // T_s[d] of the block's columns, [GC][S][64]
  const int S = A.S, n_a = A.n_a;
  const TrPlace p = tr_place(S, n_a);
  const int g0 = blockIdx.z * GC, ng = A.G - g0 < GC ? A.G - g0 : GC;
  const int d = p.col;
  const int tl = A.n_lot == 1 ? 0 : t;                       // the period's lottery
  const size_t trow = ((size_t)tl * A.n_cal + p.cal) * S;    // first row of (tl, cal) in the lottery arrays
  const double* ag = A.a_grid + (size_t)p.cal * n_a;
  const double ad = ag[p.active ? d : n_a - 1];
  double Rt = 0.0, wt = 0.0;
  if constexpr (WITH_C) {
    Rt = A.R[(size_t)p.cal * (A.T + 1) + t];
    wt = A.w[(size_t)p.cal * (A.T + 1) + t];
  }
  const double* src = mass + (size_t)g0 * A.gstride;
  double* dst = mass_out + (size_t)g0 * A.gstride;
  double cacc[GC], ts[GC];
#pragma unroll
  for (int g = 0; g < GC; ++g) cacc[g] = 0.0;
  // pull: wave w forms T_s of the block's columns for s = w, w + 4, ..., all GC masses at once
#pragma unroll 1
  for (int s = p.wave; s < S; s += kTrWaves) {
    double ls = 0.0;
    if constexpr (WITH_C) ls = wt * A.lab[p.rows + s];
    tr_pull_multi<GC, WITH_C>(A.jb + (trow + s) * (size_t)(n_a + 1), A.wlo + (trow + s) * (size_t)n_a,
                              src + (p.rows + s) * (size_t)n_a, A.gstride, ng, d, p.active, p.lane, ag, Rt, ls, ad, ts,
                              cacc);
#pragma unroll
    for (int g = 0; g < GC; ++g) co_lds[((size_t)g * S + s) * kTrCols + p.lane] = ts[g];
  }
  __syncthreads();
  // mix: wave w forms mass'[s'] for s' = w, w + 4, ...
  const double* Pc = A.P + p.rows * S;
  double kacc[GC], colp[GC];
#pragma unroll
  for (int g = 0; g < GC; ++g) kacc[g] = colp[g] = 0.0;
#pragma unroll 1
  for (int sp = p.wave; sp < S; sp += kTrWaves) {
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      if (g < ng) {   // block-uniform
        const double acc = tr_mix_forward(Pc, co_lds + (size_t)g * S * kTrCols, S, sp, p.lane);
        double m = 0.0;
        if (p.active) {
          dst[(size_t)g * A.gstride + (p.rows + sp) * (size_t)n_a + d] = acc;
          kacc[g] += acc * ad;
          colp[g] += acc;
          m = acc;
        }
        co_inc(A, p, t + 1, g0 + g, sp, m);
      }
    }
  }
  co_tail<GC, WITH_C>(A, p, t + 1, g0, ng, colp, kacc, cacc, co_lds);
}

// The periods [p0, p1) of the ring: K[cal][g][p], C[cal][g][p - 1], occ[cal][g][p][q] and
// inc[cal][g][p][s] = the blocks' partials in block order.
__global__ __launch_bounds__(256) void co_sum_kernel(CoFwd A, int p0, int p1, double* __restrict__ K,
                                                     double* __restrict__ C, double* __restrict__ occ,
                                                     double* __restrict__ inc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)A.n_cal * A.G * A.X;
  if (i >= per * (p1 - p0)) return;
  const int p = p0 + (int)(i / per);
  const long long r = i % per;
  const int x = (int)(r % A.X), g = (int)(r / A.X % A.G), cal = (int)(r / A.X / A.G);
  if (x == 1 && (C == nullptr || p == 0)) return;
  const double* part = co_part(A, p, cal, g, x);
  double v = 0.0;
  for (int b = 0; b < A.nblk; ++b) v += part[b];
  const size_t cg = (size_t)cal * A.G + g;
  if (x == 0) K[cg * (A.T + 1) + p] = v;
  else if (x == 1) C[cg * A.T + p - 1] = v;
  else if (x < 2 + A.Q) occ[(cg * (A.T + 1) + p) * A.Q + (x - 2)] = v;
  else inc[(cg * (A.T + 1) + p) * A.S + (x - 2 - A.Q)] = v;
}

// ---------------------------------------------------------------------------------
// Launch plumbing
// ---------------------------------------------------------------------------------
// Cohorts per chunk: as many as the tile and the registers admit, the chunks levelled.
struct CoPlan {
  int gc, nchunk;
};
static CoPlan co_plan(int S, int G) {
  const int cap = std::min(kCoMaxGC, kCoTileRows / S);
  CoPlan p;
  p.nchunk = (G + cap - 1) / cap;
  p.gc = (G + p.nchunk - 1) / p.nchunk;
  return p;
}

template <int GC>
static void co_launch_gc(const CoFwd& A, const CoPlan& pl, int t, bool with_c, const double* src, double* dst,
                         hipStream_t st) {
  const dim3 grid(A.nblk, A.n_cal, pl.nchunk);
  const size_t lds = co_lds_doubles(GC, A.S) * sizeof(double);
  if (t < 0) hipLaunchKernelGGL((co_first_kernel<GC>), grid, dim3(kTrBlock), lds, st, A, src);
  else if (with_c) hipLaunchKernelGGL((co_forward_kernel<GC, true>), grid, dim3(kTrBlock), lds, st, A, t, src, dst);
  else hipLaunchKernelGGL((co_forward_kernel<GC, false>), grid, dim3(kTrBlock), lds, st, A, t, src, dst);
}
// t < 0: period 0's outputs of src.
static void co_launch(const CoFwd& A, const CoPlan& pl, int t, bool with_c, const double* src, double* dst,
                      hipStream_t st) {
  switch (pl.gc) {
    case 1: co_launch_gc<1>(A, pl, t, with_c, src, dst, st); break;
    case 2: co_launch_gc<2>(A, pl, t, with_c, src, dst, st); break;
    case 3: co_launch_gc<3>(A, pl, t, with_c, src, dst, st); break;
    case 4: co_launch_gc<4>(A, pl, t, with_c, src, dst, st); break;
    case 5: co_launch_gc<5>(A, pl, t, with_c, src, dst, st); break;
    case 6: co_launch_gc<6>(A, pl, t, with_c, src, dst, st); break;
    case 7: co_launch_gc<7>(A, pl, t, with_c, src, dst, st); break;
    default: co_launch_gc<8>(A, pl, t, with_c, src, dst, st); break;
  }
}

// ---------------------------------------------------------------------------------
// Work space (caller-owned): every region starts on a 256-byte boundary.
// ---------------------------------------------------------------------------------
struct CoWork {
  int *jb, *flag, *edges;
  double *alt, *part;   // alt: ping-pong partner of the cohorts
  size_t bytes;
  int nblk, X, ring;    // ring: periods of partials, n_lot + 1 up to kCoRing (a space sized for the
};                      // steady lottery holds the two periods every call has)

static bool co_sizes_ok(int n_cal, int S, int n_a, int n_lot, int G, int Q) {
  return tr_pull_sizes_ok(n_cal, S, n_a) && n_lot >= 1 && G >= 1 && G <= AIY_MAX_COHORTS && Q >= 1 &&
         Q <= AIY_MAX_CLASSES;
}

static CoWork co_work(Carve c, int n_cal, int S, int n_a, int n_lot, int G, int Q) {
  CoWork L;
  L.nblk = tr_nblk(n_a);
  L.X = 2 + Q + S;
  L.ring = std::min(n_lot, kCoRing - 1) + 1;
  L.jb = c.take<int>((size_t)n_lot * n_cal * S * (n_a + 1));
  L.alt = c.take<double>((size_t)G * n_cal * S * n_a);
  L.part = c.take<double>((size_t)L.ring * n_cal * G * L.X * L.nblk);
  L.edges = c.take<int>((size_t)n_cal * (Q + 1));
  L.flag = c.take<int>(256 / sizeof(int));
  L.bytes = c.bytes();
  return L;
}

// The sums of every period (handle scratch: the work space is sized without T).
struct CoSums {
  double *K, *C, *occ, *inc;
  size_t bytes;
};
static CoSums co_sums(Carve c, int n_cal, int G, int T, int Q, int S) {
  CoSums L;
  const size_t cg = (size_t)n_cal * G;
  L.K = c.take<double>(cg * (T + 1));
  L.C = c.take<double>(cg * T);
  L.occ = c.take<double>(cg * (T + 1) * Q);
  L.inc = c.take<double>(cg * (T + 1) * S);
  L.bytes = c.bytes();
  return L;
}

}  // namespace aiy

using namespace aiy;

extern "C" int64_t aiy_cohort_work_bytes(int32_t n_cal, int32_t S, int32_t n_a, int32_t n_lot, int32_t G, int32_t Q) {
  if (!co_sizes_ok(n_cal, S, n_a, n_lot, G, Q)) return -1;
  return (int64_t)co_work(Carve(), n_cal, S, n_a, n_lot, G, Q).bytes;
}

extern "C" int32_t aiy_cohort_forward(aiy_handle* h, int32_t n_cal, int32_t S, int32_t n_a, int32_t T, int32_t n_lot,
                                      int32_t G, int32_t Q, const int32_t* lo, const double* wlo, const double* P,
                                      const double* a_grid, const double* R, const double* w, const double* lab,
                                      const int32_t* edges, void* work, double* mass, double* K_out, double* C_out,
                                      double* occ_out, double* inc_out, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  int32_t rc = tr_check(h, n_cal, S, n_a, true, T);
  if (rc) return rc;
  if (G < 1 || G > AIY_MAX_COHORTS) return fail(h, AIY_ERR_ARG, "G=%d outside 1..%d", G, AIY_MAX_COHORTS);
  if (Q < 1 || Q > AIY_MAX_CLASSES) return fail(h, AIY_ERR_ARG, "Q=%d outside 1..%d", Q, AIY_MAX_CLASSES);
  if (n_lot != 1 && n_lot != T) return fail(h, AIY_ERR_ARG, "n_lot=%d must be 1 or T=%d", n_lot, T);
  if (!lo || !wlo || !P || !a_grid || !edges || !work || !mass || !K_out || !occ_out)
    return fail(h, AIY_ERR_ARG, "null buffer");
  if (C_out && (!R || !w || !lab)) return fail(h, AIY_ERR_ARG, "C_out needs R, w and lab");
  for (int cal = 0; cal < n_cal; ++cal) {
    const int32_t* E = edges + (size_t)cal * (Q + 1);
    bool ok = E[0] == 0 && E[Q] == n_a;
    for (int q = 0; q < Q && ok; ++q) ok = E[q] <= E[q + 1];
    if (!ok)
      return fail(h, AIY_ERR_ARG, "edges of calibration %d must be non-decreasing from 0 to n_a=%d", cal, n_a);
  }
  AIY_HIP(h, hipSetDevice(h->device));
  hipStream_t st = as_stream(stream);
  AIY_USE_STREAM(h, st);
  const CoWork L = co_work(Carve(work), n_cal, S, n_a, n_lot, G, Q);
  rc = h->cohort.reserve(h, co_sums(Carve(), n_cal, G, T, Q, S).bytes);
  if (rc) return rc;
  const CoSums D = co_sums(Carve(h->cohort.get()), n_cal, G, T, Q, S);
  // inverse index of every lottery period and the row check, before anything is pushed
  rc = tr_build_ranges(h, n_cal, S, n_a, n_lot, lo, L.jb, L.flag, st);
  if (rc) return rc;
  AIY_HIP(h, hipMemcpyAsync(L.edges, edges, (size_t)n_cal * (Q + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  CoFwd A;
  A.n_cal = n_cal; A.S = S; A.n_a = n_a; A.T = T; A.n_lot = n_lot; A.G = G; A.Q = Q;
  A.nblk = L.nblk; A.X = L.X; A.ring = L.ring;
  A.gstride = (size_t)n_cal * S * n_a;
  A.wlo = wlo; A.jb = L.jb; A.P = P; A.a_grid = a_grid; A.R = R; A.w = w; A.lab = lab;
  A.edges = L.edges; A.part = L.part;
  const CoPlan pl = co_plan(S, G);
  const bool with_c = C_out != nullptr;
  const long long per = (long long)n_cal * G * L.X;
  int folded = 0;   // periods [0, folded) are summed
  auto fold = [&](int p1) {
    const long long n = per * (p1 - folded);
    hipLaunchKernelGGL(co_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, folded, p1, D.K,
                       with_c ? D.C : (double*)nullptr, D.occ, D.inc);
    folded = p1;
  };
  co_launch(A, pl, -1, false, mass, nullptr, st);
  for (int t = 0; t < T; ++t) {   // period t reads mass (t even) / alt (t odd) and writes slot (t + 1) % ring
    if (t + 1 - folded == L.ring) fold(t + 1);
    co_launch(A, pl, t, with_c, (t & 1) ? L.alt : mass, (t & 1) ? mass : L.alt, st);
  }
  fold(T + 1);
  AIY_CHECK_LAUNCH(h);
  const size_t cg = (size_t)n_cal * G;
  if (T & 1) AIY_HIP(h, hipMemcpyAsync(mass, L.alt, (size_t)G * A.gstride * sizeof(double), hipMemcpyDeviceToDevice, st));
  AIY_HIP(h, hipMemcpyAsync(K_out, D.K, cg * (T + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (with_c) AIY_HIP(h, hipMemcpyAsync(C_out, D.C, cg * T * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipMemcpyAsync(occ_out, D.occ, cg * (T + 1) * Q * sizeof(double), hipMemcpyDeviceToHost, st));
  if (inc_out)
    AIY_HIP(h, hipMemcpyAsync(inc_out, D.inc, cg * (T + 1) * S * sizeof(double), hipMemcpyDeviceToHost, st));
  AIY_HIP(h, hipStreamSynchronize(st));
  return AIY_OK;
}
