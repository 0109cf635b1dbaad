// What the transition sweeps (transition.hip) and the sequence-space Jacobian kernels
// (transition_jac.hip) share: the block shape of the pull kernels and the inverse index /
// row check of a lottery.
#pragma once
#include "common.h"
#include "internal.h"

namespace aiy {

constexpr int kTrBlock = 256;
constexpr int kTrWaves = kTrBlock / kWave;

constexpr int kTrRangePer = 4;   // sources per thread (one per thread: ~2 M tiny workgroups at Table II size)

// A block owns kTrCols destination columns (one per lane); its waves share the states.
constexpr int kTrCols = kWave;

// Largest sizes the pull kernels index (host-only).
inline bool tr_pull_sizes_ok(int n_cal, int S, int n_a) {
  return n_cal >= 1 && n_cal <= 65535 && S >= 1 && S <= AIY_MAX_STATES && n_a >= 2 &&
         (long long)S * (n_a + 1) < 2147483647LL && n_a < 2147483647 - 2 * kTrBlock * kTrRangePer;
}

// jb[t][cal][s][d] = first j with lo[t][cal][s][j] >= d (d in [0, n_a]) for the T periods of a
// [T][n_cal][S][n_a] lottery, and the row check (tr_range_kernel, transition.hip).  Blocks on
// `st` for the flag (4 bytes at d_flag).  AIY_ERR_UNSUPPORTED, with last_error naming the
// check, when a row is not non-decreasing or leaves [0, n_a - 2]; jb is then not to be used.
int32_t tr_build_ranges(aiy_handle* h, int n_cal, int S, int n_a, int T, const int* lo, int* jb, int* d_flag,
                        hipStream_t st);

// g[d][j] = sum over s, ascending, of mass[d][s][j] for the n_dist distributions of a
// [n_dist][S][n_a] stack (tr_marginal_kernel, transition.hip).  Asynchronous on `st`.
void tr_launch_marginal(long long n_dist, int S, int n_a, const double* mass, double* g, hipStream_t st);

}  // namespace aiy
