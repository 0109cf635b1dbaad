// One calibration's root search on f(r) = K_s(r) - K_d(r) (build-defined row E1), shared
// by the host-driven search (ge.hip) and the device-resident one (ge_resident.hip):
// method 0 = bisection (oracle/stationary.py ge_bisect, step for step); method 1 =
// bisection until both signs of f are evaluated, then Brent's method (the
// scipy.optimize.brentq algorithm; aiyagari_hark_amd/stationary.py _Brent is the same
// coroutine in Python), or -- with loose bracketing -- the log-coordinate bracketing and
// Brent described at `logsec` below (no Python mirror: the Python engine runs without loose
// bracketing).  Every workgroup of a device cluster runs its own copy on bit-identical
// inputs, so all copies take the same steps.
// (Ports that must follow a change of RootSearch: tools/multisection_study.py and
// aiyagari_hark_amd/stationary.py _Brent.)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace aiy {


struct RootSearch {
  double lo, hi, xtol;
  bool have_lo, have_hi, brent, done;
  // log-secant bracketing (with loose bracketing): while only K_s < K_d has been seen, the
  // next point comes from a secant of g = log(K_s / K_d) against u = log(rtop - r) through
  // the last two such points -- near 1/beta - 1 the excess supply grows about exponentially
  // in u -- aimed 20 % past the predicted root, its distance to rtop kept within [1/16, 1/2]
  // of the current one (1/2: bisection toward rtop)
  // ... and Brent's method then runs in the same coordinates (u, g), where the root is nearly
  // linear, with the tolerance xtol / (rtop - lo) in u (so the bracket in r is <= xtol)
  bool logsec, logsec1;   // logsec1: also the one-point step (log_secant == 2)
  int nneg;
  double rtop, ua, ga, ub, gb, glo, ghi;
  bool logb;   // Brent runs in (u, g)
  double flo, fhi, x;
  double xpre, fpre, xcur, fcur, xblk, fblk, spre, scur;
  double xprev_eval, fprev_eval;
  int method;

  __host__ __device__ static double fabs_(double v) { return v < 0 ? -v : v; }
  __host__ __device__ static double fmin_(double a, double b) { return (b < a) ? b : a; }   // std::min

  __host__ __device__ void init(double l, double h, double tol, int meth, int log_secant = 0) {
    lo = l; hi = h; xtol = tol; method = meth;
    logsec = log_secant > 0 && meth == 1;
    logsec1 = logsec && log_secant >= 2;
    nneg = 0;
    rtop = h;
    ua = ga = ub = gb = glo = ghi = 0.0;
    logb = false;
    have_lo = have_hi = brent = false;
    flo = fhi = 0.0;
    xpre = fpre = xcur = fcur = xblk = fblk = spre = scur = 0.0;
    xprev_eval = fprev_eval = 0.0;
    x = 0.5 * (lo + hi);
    done = !(hi - lo > xtol);
  }
  __host__ __device__ void update(double f, double Kd = 0.0) {
    if (done) return;
    if (method == 0) {   // oracle ge_bisect: Ks > Kd -> hi = mid
      if (f > 0) hi = x; else lo = x;
      if (!(hi - lo > xtol)) { done = true; x = 0.5 * (lo + hi); return; }
      x = 0.5 * (lo + hi);
      return;
    }
    const bool tr = logsec && Kd > 0 && f > -Kd;   // transformed coordinates available
    if (!brent) {
      if (f > 0) { hi = x; fhi = f; have_hi = true; } else { lo = x; flo = f; have_lo = true; }
      if (tr) (f > 0 ? ghi : glo) = log1p(f / Kd);
      if (hi - lo <= xtol) { done = true; x = 0.5 * (lo + hi); return; }
      if (!have_lo || !have_hi) {
        const double xe = x;
        x = 0.5 * (lo + hi);
        if (logsec1 && !have_lo && tr && f > 0 && xe < rtop) {
          // only K_s > K_d seen (the first point was above the root): the same unit-slope
          // prediction from the latest point, aimed 25 % beyond the root (away from rtop),
          // the distance to rtop grown 2 .. 16 times; bisection if that leaves the bracket
          const double dc = rtop - xe;
          double dn = 1.25 * exp(log(dc) + log1p(f / Kd));
          dn = dn < 2 * dc ? 2 * dc : (dn > 16 * dc ? 16 * dc : dn);
          const double xn = rtop - dn;
          if (xn > lo && xn < hi) x = xn;
        }
        if (logsec && !have_hi && Kd > 0 && f > -Kd && xe < rtop) {
          ua = ub; ga = gb;
          ub = log(rtop - xe); gb = log1p(f / Kd);
          ++nneg;
          // one point: the slope dg/du = -1 the Table II cells show far from 1/beta - 1
          // (K_s / K_d - 1 about doubles per halving of the distance); two: their secant
          const bool two = nneg >= 2 && gb > ga && ub < ua;
          // (the one-point prediction only where it lies well toward rtop, < 1/4 of the current
          // distance: the slope is steeper where the root is far below 1/beta - 1)
          const double us = two ? ub - gb * (ub - ua) / (gb - ga) : ub + gb;   // predicted root in u
          const double dc = rtop - xe;
          if (two || (nneg == 1 && logsec1 && exp(us) < dc / 4)) {
            double dn = 0.8 * exp(us);
            dn = dn < dc / 16 ? dc / 16 : (dn > dc / 2 ? dc / 2 : dn);
            const double xn = rtop - dn;
            if (xn > lo && xn < hi) x = xn;
          }
        }
        return;
      }
      brent = true;
      if (logsec && tr && hi < rtop) {   // Brent in (u, g); xtol in u keeps the r bracket <= xtol
        logb = true;
        xtol = xtol / (rtop - lo);
        xpre = log(rtop - lo); fpre = glo; xcur = log(rtop - hi); fcur = ghi;
      } else {
        xpre = lo; fpre = flo; xcur = hi; fcur = fhi;
      }
      xblk = fblk = spre = scur = 0.0;
      step();
      if (logb) x = rtop - exp(x);
      return;
    }
    xpre = xprev_eval; fpre = fprev_eval; fcur = logb ? (tr ? log1p(f / Kd) : (f > 0 ? 1e300 : -1e300)) : f;
    step();
    if (logb) x = rtop - exp(x);
  }
  __host__ __device__ void step() {
    const double kEps = 2.220446049250313e-16;   // DBL_EPSILON
    if (fpre * fcur < 0) { xblk = xpre; fblk = fpre; spre = scur = xcur - xpre; }
    if (fabs_(fblk) < fabs_(fcur)) {
      const double xp = xcur, xc = xblk, fp = fcur, fc = fblk;
      xpre = xp; xcur = xc; xblk = xp;
      fpre = fp; fcur = fc; fblk = fp;
    }
    const double delta = 0.5 * (xtol + 4 * kEps * fabs_(xcur));
    const double sbis = 0.5 * (xblk - xcur);
    if (fcur == 0 || fabs_(sbis) < delta) { done = true; x = xcur; return; }
    if (fabs_(spre) > delta && fabs_(fcur) < fabs_(fpre)) {
      double stry;
      if (xpre == xblk) {
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
      }
      if (2 * fabs_(stry) < fmin_(fabs_(spre), 3 * fabs_(sbis) - delta)) { spre = scur; scur = stry; }
      else { spre = sbis; scur = sbis; }
    } else {
      spre = sbis; scur = sbis;
    }
    xprev_eval = xcur; fprev_eval = fcur;
    xcur += fabs_(scur) > delta ? scur : (sbis > 0 ? delta : -delta);
    x = xcur;
  }
};

// loose-bracketing tolerances (aiy_ge_options.loose_bracket) and the sign margin a loose
// evaluation's K_s - K_d needs (|f| >= kGeSignMargin K_d)
#ifndef AIY_GE_LOOSE_EGM
#define AIY_GE_LOOSE_EGM 1e-6
#endif
// (the histogram's loose tolerance is the handle option AIY_OPT_GE_LOOSE_HIST: 10^-8 by default
// since round 4, 10^-10 before; the full-size Table II / stress parity tests pass at both)
constexpr double kGeSignMargin = 0.05;

// Adaptive distribution tolerance of Brent's evaluations (with loose bracketing).  A BiCGSTAB
// solve stopped at max|T x - x| < tol leaves K_s about 4e5 tol off relative (DESIGN.md §4c:
// 4e-7 at 1e-12), and Brent's next |f| is rarely below 1/100 of the smallest |f| seen so far
// (the Table II searches: 20-80x per step), so an evaluation at tol = kGeAdaptC |f|_min / K_d
// already resolves f to well inside its expected size; its sign and value are trusted when
// |f| >= kGeAdaptMargin tol K_d (5 % at 1e-8, the bracketing margin: 12x the error estimate),
// else the same r is evaluated again at the full tolerance (continuing from its mass: the
// stopping rule of the final bracket is unchanged).  -DAIY_DIAG_NO_ADAPT turns it off.
constexpr double kGeAdaptC = 1e-9;
constexpr double kGeAdaptMargin = 5e6;
#ifdef AIY_DIAG_NO_ADAPT
constexpr bool kGeAdapt = false;
#else
constexpr bool kGeAdapt = true;
#endif
__host__ __device__ inline double ge_adapt_htol(double fmin_rel, double hist_tol, double loose_hist) {
  const double t = kGeAdaptC * fmin_rel;
  return t > loose_hist ? loose_hist : (t < hist_tol ? hist_tol : t);   // NaN: hist_tol
}

__host__ __device__ inline bool ge_finite(double v) {
#ifdef __HIP_DEVICE_COMPILE__
  return isfinite(v);
#else
  return std::isfinite(v);
#endif
}

// The firm's prices at r (calc_R_and_W's firm, L = 1): R = 1 + r, the wage and K_d.
struct GePrices {
  double R, wage, Kd;
};
__host__ __device__ inline GePrices ge_prices(double r, double alpha, double delta) {
  const double KtoL = pow(alpha / (r + delta), 1.0 / (1.0 - alpha));
  return {1.0 + r, (1.0 - alpha) * pow(KtoL, alpha), KtoL};
}

// The search options one evaluation is planned and accepted with (aiy_ge_options and the
// handle's AIY_OPT_GE_LOGSEC / AIY_OPT_GE_LOOSE_HIST, as flags).
struct GeEvalOpts {
  int method, loose, logsec, warm_egm, warm_hist, secant;
  double r_tol, egm_tol, hist_tol, loose_hist;
};

// One calibration's search around its RootSearch: what it carries between the K_s(r)
// evaluations, and the plan of the next one.  plan() before an evaluation, accept() with its
// K_s after it; the host-driven loop (ge.hip) and the device-resident kernel (ge_resident.hip)
// drive the same two calls.
struct GeEval {
  RootSearch rs;
  double r_cur, r_prev;   // the last two evaluated r (secant starts)
  double fmin;            // smallest |K_s - K_d| / K_d accepted so far (adaptive tolerance)
  int refine;             // the last evaluation's sign was not trusted: the same r again, full tolerances
  int final_ks;           // the search ended on a loose or adaptive-tolerance evaluation: that r is
                          // evaluated once more at the full tolerances before K_s is reported
  int steps;              // evaluations accepted
  // the planned evaluation
  double r, R, wage, Kd, etol, htol, theta;
  int loose, adapt, warm_egm, secant, fresh_mass;

  // the bracket where the caller gives none: [-delta / 2, 1 / disc - 1)
  __host__ __device__ static double default_lo(double delta) { return -0.5 * delta; }
  __host__ __device__ static double default_hi(double disc) { return 1.0 / disc - 1.0 - 1e-9; }

  __host__ __device__ void init(const GeEvalOpts& o, double lo, double hi) {
    rs.init(lo, hi, o.r_tol, o.method, o.loose ? o.logsec : 0);
    r_cur = r_prev = 0.0;
    fmin = HUGE_VAL;
    refine = final_ks = steps = 0;
    r = R = wage = Kd = theta = 0.0;
    etol = o.egm_tol;
    htol = o.hist_tol;
    loose = adapt = warm_egm = secant = fresh_mass = 0;
  }

  // Prices, tolerances and starts of the next evaluation.  (The final pass re-evaluates the
  // LAST evaluated r at the full tolerances, from its own tables and mass: no secant start.)
  __host__ __device__ void plan(const GeEvalOpts& o, double alpha, double delta) {
    r = final_ks ? r_cur : rs.x;
    const GePrices p = ge_prices(r, alpha, delta);
    R = p.R;
    wage = p.wage;
    Kd = p.Kd;
    // bracketing evaluations run loose, Brent's at the adaptive tolerance, refined ones and
    // a finished search's at the full tolerances
    const bool open = o.loose && o.method == 1 && !rs.done && !refine;
    const double loose_hist = fmax(o.hist_tol, o.loose_hist);
    loose = open && !rs.brent;
    etol = loose ? fmax(o.egm_tol, AIY_GE_LOOSE_EGM) : o.egm_tol;
    htol = loose ? loose_hist : o.hist_tol;
    adapt = 0;
    if (kGeAdapt && open && rs.brent) {
      htol = ge_adapt_htol(fmin, o.hist_tol, loose_hist);
      adapt = htol > o.hist_tol;
    }
    warm_egm = o.warm_egm && steps > 0;
    secant = o.secant && o.warm_egm && o.warm_hist && steps >= 2 && !final_ks;
    fresh_mass = !(o.warm_hist && steps > 0);
    double th = 0.0;
    if (secant) {
      const double den = r_cur - r_prev;
      th = den != 0.0 ? (r - r_cur) / den : 0.0;
      th = ge_finite(th) ? fmax(-1.0, ::fmin(1.0, th)) : 0.0;
    }
    theta = th;
  }

  // The evaluation's K_s: move the bracket unless its sign is not trusted (then the same r is
  // planned again at the full tolerances).
  __host__ __device__ void accept(double Ks) {
    r_prev = r_cur;
    r_cur = rs.x;
    const double f = Ks - Kd;
    refine = (loose && !(fabs(f) >= kGeSignMargin * Kd)) ||   // NaN: refine
             (adapt && !(fabs(f) >= kGeAdaptMargin * htol * Kd));
    if (!refine) {
      rs.update(f, Kd);
      fmin = ::fmin(fmin, fabs(f) / Kd);   // (the member hides the function)
    }
    ++steps;
    // a search that ends on an evaluation at looser tolerances (a loose bracketing
    // one, or Brent's at the adaptive distribution tolerance) reports K_s only after that r is
    // evaluated again at egm_tol / hist_tol (one more pass, warm from its tables and mass: a few
    // cycles and matvecs; searches normally end on full-tolerance evaluations near the root)
    if (rs.done && (adapt || loose)) final_ks = 1;
  }
};

// ---- the EGM accelerations of the household solves (egm.hip's host-driven solve and the
//      resident kernel): every expression in this operand order (-ffp-contract=off), so both
//      paths mix and extrapolate to the same bits from the same sums ----

// Type-II Anderson over the plain chain w0 .. w4 (m = 3): g_i = w_{i+1} - w_i, dG_i = g_{i+1} -
// g_i; one point's terms of the Gram matrix dG' dG (acc[0..5]: 00 01 02 11 12 22) and of
// dG' g_3 (acc[6..8]).
__host__ __device__ inline void aa_gram_add(double w0, double w1, double w2, double w3, double w4, double* acc) {
  const double g0 = w1 - w0, g1 = w2 - w1, g2 = w3 - w2, g3 = w4 - w3;
  const double d0 = g1 - g0, d1 = g2 - g1, d2 = g3 - g2;
  acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2;
  acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
  acc[6] += d0 * g3; acc[7] += d1 * g3; acc[8] += d2 * g3;
}
// gamma = argmin |g_3 - dG gamma| from the summed terms: Cholesky of the Gram matrix plus
// 1e-12 of its trace.  false: degenerate or non-finite (a converging chain whose differences
// vanish, NaN nodes) -- no mix, the cycle's output stands.
__host__ __device__ inline bool aa_solve(const double* gs, double* gam) {
  double a00 = gs[0], a01 = gs[1], a02 = gs[2], a11 = gs[3], a12 = gs[4], a22 = gs[5];
  const double b0 = gs[6], b1 = gs[7], b2 = gs[8];
  const double reg = 1e-12 * (a00 + a11 + a22);
  if (!(reg > 0.0)) return false;
  a00 += reg; a11 += reg; a22 += reg;
  const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
  const double l11 = sqrt(a11 - l10 * l10), l21 = (a12 - l20 * l10) / l11;
  const double l22 = sqrt(a22 - l20 * l20 - l21 * l21);
  const double y0 = b0 / l00, y1 = (b1 - l10 * y0) / l11, y2 = (b2 - l20 * y0 - l21 * y1) / l22;
  gam[2] = y2 / l22;
  gam[1] = (y1 - l21 * gam[2]) / l11;
  gam[0] = (y0 - l10 * gam[1] - l20 * gam[2]) / l00;
  return ge_finite(gam[0]) && ge_finite(gam[1]) && ge_finite(gam[2]);
}
// the mixed iterate of one point: w4 - dF gamma, dF_i = w_{i+2} - w_{i+1}
__host__ __device__ inline double aa_mix(const double* gam, double w1, double w2, double w3, double w4) {
  return w4 - ((gam[0] * (w2 - w1) + gam[1] * (w3 - w2)) + gam[2] * (w4 - w3));
}

// Geometric extrapolation at a check (cycle n, cluster distances d1 now and d0 one cycle ago):
// where the distances fall at a steady rate lambda = d1 / d0 (0.5 < lambda < 0.999, within 20 %
// of 1 - lambda of the previous check's, the distance still > 100 tol, n >= 4) the factor
// lambda / (1 - lambda) of X_n += factor (X_n - X_{n-1}), else 0; lam_prev <- lambda.
__host__ __device__ inline double egm_extrap_factor(double d1, double d0, double etol, int n, double& lam_prev) {
  const double lam = d1 / d0;
  double f = 0.0;
  if (n >= 4 && d1 > 100.0 * etol && lam > 0.5 && lam < 0.999 && lam_prev > 0.0 &&
      fabs(lam - lam_prev) < 0.2 * (1.0 - lam))
    f = lam / (1.0 - lam);
  lam_prev = lam;
  return f;
}

}  // namespace aiy
