// Stand-alone host driver of csrc/ge_search.h for tests/test_ge_policy.py (no GPU): the GE
// search policy GeEval on a synthetic capital supply, and the EGM acceleration helpers.
// Doubles are read and printed as C hex floats, so the test compares bits.
//
//   search METHOD LOOSE LOGSEC R_TOL MAX_STEPS A PERT
//       K_s(r) = A (r + 0.06) / (0.0417 - r) + PERT * htol * K_d  (+ - * / only), alpha = 0.36,
//       delta = 0.08, disc = 0.96, default bracket, secant / warm starts on.  One line per
//       evaluation (printed after plan(), before accept()):
//         E r Kd loose adapt etol htol theta refine final lo hi xcur xblk
//       refine: this plan re-evaluates an r whose sign was not trusted; lo hi xcur xblk: the
//       bracket (bisection phase / Brent).
//       Then "END done steps x".
//   aa N w0[N] w1[N] w2[N] w3[N] w4[N]    ->  "MIX 1 x[N]" or "MIX 0"
//   ext D1 D0 ETOL N LAM_PREV             ->  "EXT factor lam_prev"
#include "../../aiyagari_hark_amd/csrc/ge_search.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace aiy;

static double num(const char* s) { return std::strtod(s, nullptr); }

static int run_search(char** a) {
  const GeEvalOpts o{std::atoi(a[0]), std::atoi(a[1]), std::atoi(a[2]), 1, 1, 1, num(a[3]), 1e-8, 1e-12, 1e-8};
  const int max_steps = std::atoi(a[4]);
  const double A = num(a[5]), pert = num(a[6]);
  const double alpha = 0.36, delta = 0.08, disc = 0.96;
  GeEval ev;
  ev.init(o, GeEval::default_lo(delta), GeEval::default_hi(disc));
  while ((!ev.rs.done && ev.steps < max_steps) || ev.final_ks) {   // the resident kernel's loop
    const int refine = ev.refine;
    ev.plan(o, alpha, delta);
    const double Ks = A * (ev.r + 0.06) / (0.0417 - ev.r) + pert * ev.htol * ev.Kd;
    std::printf("E %a %a %d %d %a %a %a %d %d %a %a %a %a\n", ev.r, ev.Kd, ev.loose, ev.adapt, ev.etol, ev.htol, ev.theta,
                refine, ev.final_ks, ev.rs.lo, ev.rs.hi, ev.rs.xcur, ev.rs.xblk);
    if (ev.final_ks) break;   // the full-tolerance pass of the last evaluated r: K_s only
    ev.accept(Ks);
  }
  std::printf("END %d %d %a\n", (int)ev.rs.done, ev.steps, ev.rs.x);
  return 0;
}

static int run_aa(int argc, char** a) {
  const int n = std::atoi(a[0]);
  if (n < 1 || argc != 1 + 5 * n) return 2;
  std::vector<double> w(5 * (size_t)n);
  for (size_t q = 0; q < w.size(); ++q) w[q] = num(a[1 + q]);
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gam[3];
  for (int q = 0; q < n; ++q) aa_gram_add(w[q], w[n + q], w[2 * n + q], w[3 * n + q], w[4 * n + q], acc);
  if (!aa_solve(acc, gam)) {
    std::printf("MIX 0\n");
    return 0;
  }
  std::printf("MIX 1");
  for (int q = 0; q < n; ++q) std::printf(" %a", aa_mix(gam, w[n + q], w[2 * n + q], w[3 * n + q], w[4 * n + q]));
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 9 && !std::strcmp(argv[1], "search")) return run_search(argv + 2);
  if (argc >= 3 && !std::strcmp(argv[1], "aa")) return run_aa(argc - 2, argv + 2);
  if (argc == 7 && !std::strcmp(argv[1], "ext")) {
    double lam_prev = num(argv[6]);
    const double f = egm_extrap_factor(num(argv[2]), num(argv[3]), num(argv[4]), std::atoi(argv[5]), lam_prev);
    std::printf("EXT %a %a\n", f, lam_prev);
    return 0;
  }
  std::fprintf(stderr, "usage: search | aa | ext (see the file header)\n");
  return 2;
}
