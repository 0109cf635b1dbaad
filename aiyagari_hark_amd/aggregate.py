"""The stationary economy with aggregate risk, to first order in the aggregates.

The sequence-space Jacobians of ``transition.household_jacobian`` give the linear response of
capital and prices to a TFP innovation (``linear_model``).  Under certainty equivalence the
households of period t then face the expected price deviations E_t[dx_{t+u}], u = 0 .. T, which
are a moving average of the innovations so far (``expectations``), and save

    a'_t(s, a_j) = a'*(s, a_j) + sum_x sum_u (d a' / d x_u)(s, a_j) E_t[dx_{t+u}],  x in {R, w}.

``policy_jacobian`` takes d a' / d x_u from the shocked backward sweeps of the Jacobian (the
savings policy is the mean of the Young lottery, which is what the histogram moves by);
``simulate`` forms every period's policy and its lottery on the device (aiy_aggregate_lotteries,
csrc/aggregate.hip: an FP64 matrix-instruction product with the locate as its epilogue) and
moves the whole distribution through them with the forward sweep of the transition paths.
Prices are the linear model's; ``AggregateSimulation.gap`` reports how far the simulated
capital is from the capital those prices assume.  ``moments`` and ``saving_rule`` (the
Krusell-Smith rule log K' = a + b log K + c (Z - 1)) summarise the model and a simulation.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import stats as _stats
from . import transition as _tr
from .stationary import StationaryBatch, firm_prices

F64 = torch.float64


# -------------------------------------------------------------------------------------
# Policy derivatives
# -------------------------------------------------------------------------------------
@dataclass
class PolicyJacobian:
    a_star: torch.Tensor   # [n_cal][S][n_a] device: the steady savings policy (mean of the steady lottery)
    dA_R: torch.Tensor     # [T+1][n_cal][S][n_a] device: d a' / d R_u, the lead u outermost
    dA_w: torch.Tensor     # [T+1][n_cal][S][n_a] device
    h: float               # the step of the one-sided differences


class PolicyBuffers:
    """Device buffers of one (batch, T) ``policy_jacobian``: the lottery buffers of the backward
    sweeps (``TransitionBuffers`` of T + 1 periods), the ghost's means and the two results
    ([T+1][n_cal][S][n_a], 4 GB each at the Table II shape with T = 300); nothing else is allocated."""

    def __init__(self, batch: StationaryBatch, T: int):
        n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
        dev = batch.device
        self.T = int(T)
        self.sweep = _tr.TransitionBuffers(batch, self.T + 1)
        self.ghost = torch.empty((self.T + 1, n_cal, S, n_a), dtype=F64, device=dev)
        self.dA = [torch.empty_like(self.ghost), torch.empty_like(self.ghost)]   # R, w
        self.a_star = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)
        self.lo = torch.empty((n_cal, S, n_a), dtype=torch.int32, device=dev)   # the steady lottery
        self.wlo = torch.empty((n_cal, S, n_a), dtype=F64, device=dev)


def lottery_mean(batch, lo, wlo, out=None, stream=None):
    """aiy_lottery_mean: wlo a[lo] + (1 - wlo) a[lo + 1] of a device lottery [n_cal][S][n_a] or
    [n_t][n_cal][S][n_a] on the grids of ``batch``: the savings policy the lottery stands for."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    if tuple(lo.shape[-3:]) != (n_cal, S, n_a) or lo.shape != wlo.shape or lo.dim() not in (3, 4):
        raise ValueError(f"lottery must be [n_t][n_cal={n_cal}][S={S}][n_a={n_a}], got {tuple(lo.shape)}")
    n_t = lo.shape[0] if lo.dim() == 4 else 1
    if out is None:
        out = torch.empty(lo.shape, dtype=F64, device=lo.device)
    hd = _lib.handle(batch.device.index)
    hd.check(hd.lib.aiy_lottery_mean(hd.h, n_cal, S, n_a, int(n_t), _lib.ptr(lo), _lib.ptr(wlo), _lib.ptr(batch.d_a),
                                     _lib.ptr(out), _lib.stream_ptr(stream)), "aiy_lottery_mean")
    return out


def policy_jacobian(batch, r, T, h=1e-5, buffers=None):
    """Derivatives of the savings policy of every calibration of ``batch`` at its steady state
    (interest rate ``r`` [n_cal], tables ``batch.last_tables``) with respect to R and w at the
    leads u = 0 .. T: the three backward sweeps of ``household_jacobian`` over T + 2 periods (a
    ghost and one per input with x[T] += h), the lottery mean of every period of each, and
    dA_x[u] = (mean_x[T - u] - mean_ghost[T - u]) / h.  The results are views of ``buffers``."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    T = int(T)
    if getattr(batch, "last_tables", None) is None:
        raise ValueError("no steady-state policy: run steady_state / capital_supply first")
    m_term, c_term = (_tr._tables(t, n_cal, S, n_a) for t in batch.last_tables)
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (n_cal,))
    w, _ = firm_prices(r, batch.alpha, batch.delta)
    Rs = 1.0 + r
    if buffers is None:
        buffers = PolicyBuffers(batch, T)
    elif buffers.T != T:
        raise ValueError(f"buffers hold T={buffers.T}, asked for T={T}")
    hd = _lib.handle(batch.device.index)

    def means_of_sweep(shock, out):
        _tr._shocked_backward(batch, Rs, w, T, h, shock, m_term, c_term, buffers.sweep)
        for c in range(T + 1):   # lottery period c = T - u straight into lead u: no copy, no reordering pass
            lottery_mean(batch, buffers.sweep.lo[c], buffers.sweep.wlo[c], out=out[T - c])

    means_of_sweep(None, buffers.ghost)
    for x, name in enumerate(("R", "w")):
        means_of_sweep(name, buffers.dA[x])
        hd.check(hd.lib.aiy_jacobian_diff(hd.h, buffers.ghost.numel(), _lib.ptr(buffers.dA[x]),
                                          _lib.ptr(buffers.ghost), float(h), _lib.stream_ptr()), "aiy_jacobian_diff")
    _tr.steady_lottery(batch, r, tables=(m_term, c_term), lo=buffers.lo, wlo=buffers.wlo)
    lottery_mean(batch, buffers.lo, buffers.wlo, out=buffers.a_star)
    return PolicyJacobian(a_star=buffers.a_star, dA_R=buffers.dA[0], dA_w=buffers.dA[1], h=float(h))


# -------------------------------------------------------------------------------------
# The linear model of the aggregates (host)
# -------------------------------------------------------------------------------------
def ar1(rho, T):
    """The response rho^t, t = 0 .. T, of an AR(1) TFP process to a unit innovation."""
    return float(rho) ** np.arange(int(T) + 1)


@dataclass
class AggregateModel:
    dZ: np.ndarray      # [n_cal][T+1] responses to a unit TFP innovation at t = 0
    dK: np.ndarray      # [n_cal][T+1] (dK[:, 0] = 0)
    dr: np.ndarray      # [n_cal][T+1]
    dw: np.ndarray      # [n_cal][T+1]
    K: np.ndarray       # [n_cal] K*
    r: np.ndarray       # [n_cal] the firm's rate and wage at K*
    w: np.ndarray       # [n_cal]
    alpha: np.ndarray   # [n_cal]


def linear_model(batch, jac, irf_Z):
    """The economy of ``batch`` linearised at its steady state: the responses of K, r and w to a
    unit innovation whose TFP response is ``irf_Z`` ([T+1] or [n_cal][T+1], e.g. ``ar1(rho, T)``),
    by ``impulse_response`` on the HouseholdJacobian ``jac``."""
    n_cal, T = jac.JR.shape[0], jac.JR.shape[1]
    dZ = np.array(np.broadcast_to(np.asarray(irf_Z, dtype=np.float64), (n_cal, T + 1)))
    dK, dr, dw = _tr.impulse_response(batch, jac, dZ)
    rs, ws = _tr.path_prices(jac.K[:, None], np.ones((n_cal, 1)), batch.alpha, batch.delta)
    return AggregateModel(dZ=dZ, dK=dK, dr=dr, dw=dw, K=np.array(jac.K, dtype=np.float64), r=rs[:, 0], w=ws[:, 0],
                          alpha=np.array(jac.alpha, dtype=np.float64))


MOMENT_VARIABLES = ("Z", "K", "r", "w", "Y")   # the order of the axes i, j of ``moments``


def moments(model, sigma, lags):
    """Analytic covariances of (Z, K, r, w, Y) of the linear model driven by white-noise
    innovations of standard deviation ``sigma``: [n_cal][lags+1][5][5] with
    cov[c][k][i][j] = Cov(X^i_t, X^j_{t+k}) = sigma^2 sum_s dX^i_s dX^j_{s+k} (i, j: ``MOMENT_VARIABLES``),
    dY = K*^alpha dZ + alpha K*^(alpha - 1) dK (output at L = 1).  Host only."""
    a, K = model.alpha[:, None], model.K[:, None]
    dY = K ** a * model.dZ + a * K ** (a - 1.0) * model.dK
    D = np.stack([model.dZ, model.dK, model.dr, model.dw, dY], axis=1)   # [n_cal][5][T+1]
    n = D.shape[2]
    lags = int(lags)
    out = np.zeros((D.shape[0], lags + 1, 5, 5))
    for k in range(min(lags, n - 1) + 1):
        out[:, k] = float(sigma) ** 2 * np.einsum("cis,cjs->cij", D[:, :, :n - k], D[:, :, k:])
    return out


@dataclass
class Expectations:
    X: np.ndarray       # [n_cal][n][2(T+1)]: E_t[dR_{t+u}], u = 0 .. T, then E_t[dw_{t+u}]
    dr: np.ndarray      # [n_cal][n] realised deviations (X at lead 0)
    dw: np.ndarray      # [n_cal][n]
    Z: np.ndarray       # [n_cal][n] realised TFP
    K_lin: np.ndarray   # [n_cal][n+1] the moving-average capital path


def expectations(model, eps):
    """Expected price deviations of every period of a history of innovations ``eps`` ([n] or
    [n_cal][n]) that starts from the steady state: X[c][t][x][u] = sum_{k = 0 .. min(t, T - u)}
    dx[c][u + k] eps[c][t - k] (leads beyond T are truncated), one Hankel product per
    calibration and input, on the host."""
    n_cal, T1 = model.dZ.shape
    eps = np.asarray(eps, dtype=np.float64)
    if eps.ndim not in (1, 2) or (eps.ndim == 2 and eps.shape[0] != n_cal) or eps.shape[-1] < 1:
        raise ValueError(f"eps must be [n] or [n_cal={n_cal}][n], got {eps.shape}")
    eps = np.broadcast_to(eps, (n_cal, eps.shape[-1]))
    n = eps.shape[1]
    X = np.empty((n_cal, n, 2 * T1))
    Z = np.empty((n_cal, n))
    K_lin = np.empty((n_cal, n + 1))
    t, k = np.arange(n + 1)[:, None], np.arange(T1)[None, :]
    u = np.arange(T1)[None, :]
    for c in range(n_cal):
        ext = np.concatenate([eps[c], [0.0]])   # K_lin[n] needs no innovation of period n: dK[0] = 0
        lag = np.where(t - k >= 0, ext[np.clip(t - k, 0, n)], 0.0)   # [n+1][T+1]: eps[t - k]
        for x, d in enumerate((model.dr[c], model.dw[c])):
            hank = np.where(k.T + u < T1, d[np.clip(k.T + u, 0, T1 - 1)], 0.0)   # [k][u]: dx[u + k]
            X[c, :, x * T1:(x + 1) * T1] = lag[:n] @ hank
        Z[c] = 1.0 + lag[:n] @ model.dZ[c]
        dK = np.array(model.dK[c])
        dK[0] = 0.0
        K_lin[c] = model.K[c] + lag @ dK
    return Expectations(X=X, dr=X[:, :, 0].copy(), dw=X[:, :, T1].copy(), Z=Z, K_lin=K_lin)


# -------------------------------------------------------------------------------------
# Simulation
# -------------------------------------------------------------------------------------
def aggregate_lotteries(batch, pol, X, lo, wlo, stream=None):
    """aiy_aggregate_lotteries: the Young lotteries (lo, wlo) [n_p][n_cal][S][n_a] (device, written)
    of the policies a* + sum_k op[k] X[cal][p][k] for the device X [n_cal][n_p][2(T+1)]."""
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    T = pol.dA_R.shape[0] - 1
    if X.dim() != 3 or X.shape[0] != n_cal or X.shape[2] != 2 * (T + 1) or X.dtype != F64:
        raise ValueError(f"X must be float64 [n_cal={n_cal}][n_p][{2 * (T + 1)}], got {tuple(X.shape)}")
    n_p = X.shape[1]
    if tuple(lo.shape) != (n_p, n_cal, S, n_a) or tuple(wlo.shape) != (n_p, n_cal, S, n_a):
        raise ValueError(f"lo / wlo must be [n_p={n_p}][n_cal][S][n_a], got {tuple(lo.shape)}, {tuple(wlo.shape)}")
    if lo.dtype != torch.int32 or wlo.dtype != F64:
        raise ValueError("lo must be int32 and wlo float64")
    for name, t in (("a_star", pol.a_star), ("dA_R", pol.dA_R), ("dA_w", pol.dA_w)):
        want = (n_cal, S, n_a) if name == "a_star" else (T + 1, n_cal, S, n_a)
        if tuple(t.shape) != want or t.dtype != F64:
            raise ValueError(f"{name} must be float64 {want}, got {tuple(t.shape)}")
    hd = _lib.handle(batch.device.index)
    hd.check(hd.lib.aiy_aggregate_lotteries(hd.h, n_cal, S, n_a, int(T), int(n_p), _lib.ptr(pol.a_star),
                                            _lib.ptr(pol.dA_R), _lib.ptr(pol.dA_w), _lib.ptr(X), _lib.ptr(batch.d_a),
                                            _lib.ptr(lo), _lib.ptr(wlo), _lib.stream_ptr(stream)),
             "aiy_aggregate_lotteries")
    return lo, wlo


@dataclass
class AggregateSimulation:
    K: np.ndarray            # [n_cal][n+1] capital the distribution holds (K[:, 0] = sum mass0 a)
    C: np.ndarray | None     # [n_cal][n] aggregate consumption
    Z: np.ndarray            # [n_cal][n] realised TFP
    r: np.ndarray            # [n_cal][n] realised prices (the linear model's)
    w: np.ndarray            # [n_cal][n]
    K_lin: np.ndarray        # [n_cal][n+1] the linear model's capital
    stats: _stats.WealthStats | None   # [n_cal][n+1] wealth statistics of every period (percentiles=)
    mass: torch.Tensor       # [n_cal][S][n_a] device: the distribution after the last period
    gap: np.ndarray          # [n_cal] max_t |K - K_lin| / K*: the accuracy measure
    rows_turned: int | None = None   # rows="any": lottery rows with a decreasing pair, all chunks; else None


def simulate(batch, model, pol, eps, chunk=64, percentiles=None, mass0=None, want_c=True, timings=None,
             rows="monotone"):
    """The economy of ``batch`` under the history of TFP innovations ``eps`` ([n] or [n_cal][n]),
    from the distribution ``mass0`` (default: ``batch.mass``, the steady state).  In chunks of at
    most ``chunk`` periods: the chunk's expectations go to the device, aiy_aggregate_lotteries
    turns them and the PolicyJacobian ``pol`` into the chunk's lotteries, and the forward sweep
    moves the running distribution through them at the realised prices R_t = 1 + r* + dr_t,
    w_t = w* + dw_t.  The results do not depend on ``chunk``.  ``percentiles`` (in (0, 1)): also
    the ``path_wealth_stats`` of every period.  ``timings``: a dict that receives the
    milliseconds of the stages (each stage is then synchronised).

    A shock so large that a linearised policy is no longer increasing in assets fails the
    forward sweep's row check: AiyagariLibError (AIY_ERR_UNSUPPORTED).  That is the default,
    ``rows="monotone"``, and it still refuses: on fine grids (from about 1 000 points) a linearised
    policy swaps a few neighbouring nodes at the policy's kinks and the run stops there.
    ``rows="any"`` moves the mass with ``transition_forward(rows="any")`` instead,
    which runs through such rows, and fills ``AggregateSimulation.rows_turned`` with their number
    over all chunks; it still refuses a row turned so far that its windows hold more than
    4 (n_a + 1) sources.  Where the default runs, both give the same bits."""
    if rows not in ("monotone", "any"):
        raise ValueError(f"rows must be 'monotone' or 'any', got {rows!r}")
    what = "transition_any" if rows == "any" else "transition"
    turned = 0 if rows == "any" else None
    n_cal, S, n_a = len(batch.cals), batch.S, batch.n_a
    dev = batch.device
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk={chunk} must be >= 1")
    ex = expectations(model, eps)
    n = ex.Z.shape[1]
    chunk = min(chunk, n)
    mass = _tr._device(batch.mass if mass0 is None else mass0, dev).reshape(n_cal, S, n_a).clone()
    lo = torch.empty((chunk, n_cal, S, n_a), dtype=torch.int32, device=dev)
    wlo = torch.empty((chunk, n_cal, S, n_a), dtype=F64, device=dev)
    marg = torch.empty((n + 1, n_cal, n_a), dtype=F64, device=dev) if percentiles is not None else None
    marg_c = torch.empty((chunk + 1, n_cal, n_a), dtype=F64, device=dev) if percentiles is not None else None
    works = {}
    K = np.empty((n_cal, n + 1))
    C = np.empty((n_cal, n)) if want_c else None
    t_last = [time.perf_counter()]

    def stage(name):
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + (now - t_last[0]) * 1e3
            t_last[0] = now

    if timings is not None:
        torch.cuda.synchronize(dev)
        t_last[0] = time.perf_counter()
    for t0 in range(0, n, chunk):
        L = min(chunk, n - t0)
        if L not in works:
            works[L] = _lib.work_space(dev, what, "transition", n_cal=n_cal, S=S, n_a=n_a, T=L)
        X = torch.as_tensor(np.ascontiguousarray(ex.X[:, t0:t0 + L])).to(dev)
        aggregate_lotteries(batch, pol, X, lo[:L], wlo[:L])
        stage("synthesis")
        R = w = None
        if want_c:   # [n_cal][L + 1]: the sweep reads the first L
            R = np.repeat((1.0 + model.r)[:, None], L + 1, axis=1)
            w = np.repeat(model.w[:, None], L + 1, axis=1)
            R[:, :L] += ex.dr[:, t0:t0 + L]
            w[:, :L] += ex.dw[:, t0:t0 + L]
            R, w = _tr._device(R, dev), _tr._device(w, dev)
        out = _tr.transition_forward(batch, lo[:L], wlo[:L], mass, L, works[L], R, w, want_c=want_c,
                                     marg=marg_c[:L + 1] if marg is not None else None, rows=rows)
        Ks, Cc = out[0], out[1]
        if rows == "any":
            turned += out[2]
        K[:, t0:t0 + L + 1] = Ks
        if want_c:
            C[:, t0:t0 + L] = Cc
        if marg is not None:
            marg[t0:t0 + L + 1].copy_(marg_c[:L + 1])
        stage("forward")
    ws = None
    if marg is not None:
        ws = _tr.path_wealth_stats(batch, marg, percentiles)
        stage("statistics")
    gap = np.max(np.abs(K - ex.K_lin), axis=1) / model.K
    return AggregateSimulation(K=K, C=C, Z=ex.Z, r=model.r[:, None] + ex.dr, w=model.w[:, None] + ex.dw, K_lin=ex.K_lin,
                               stats=ws, mass=mass, gap=gap, rows_turned=turned)


def saving_rule(sim, burn=0):
    """The Krusell-Smith saving rule of a simulation: per calibration (intercept, slope on log K,
    coefficient on Z - 1, R^2) of log K[t+1] on (1, log K[t], Z[t] - 1), t = burn .. n - 1, by
    least squares on the host; [n_cal][4]."""
    K, Z = np.asarray(sim.K, dtype=np.float64), np.asarray(sim.Z, dtype=np.float64)
    if K.ndim == 1:
        K, Z = K[None], Z[None]
    n = Z.shape[1]
    burn = int(burn)
    if not 0 <= burn <= n - 3:
        raise ValueError(f"burn={burn} leaves fewer than three observations of {n}")
    out = np.empty((K.shape[0], 4))
    for c in range(K.shape[0]):
        y = np.log(K[c, burn + 1:n + 1])
        A = np.stack([np.ones(n - burn), np.log(K[c, burn:n]), Z[c, burn:n] - 1.0], axis=1)
        coef, *_ = np.linalg.lstsq(A, y, rcond=None)
        res, tot = y - A @ coef, y - y.mean()
        out[c, :3] = coef
        out[c, 3] = 1.0 - float(res @ res) / float(tot @ tot) if float(tot @ tot) > 0.0 else 1.0
    return out
