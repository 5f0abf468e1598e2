"""Reference of the soft box  + sum_rows s_i dist(w_i, [lo_i, hi_i])   for the tests: tests/_fuel_ref.py::solve's
loop with the z-update

    c = clip(v, lo, hi),  e = v - c,  z = |e| <= kap ? c : (e > 0 ? v - kap : v + kap),  y = v - z         (kap = s / rho)

on every row but the control rows of a stage with a thrust bound or a fuel weight, which keep _fuel_ref.prox's shrink-and-scale
-- and nothing else: factor, x_update, residuals, converged, expand_bounds, expand_unorm come from oracle/admm_ref.py and
expand_fuel / prox from _fuel_ref.py, as _fuel_ref.py takes them.  With every weight +inf the loop is _fuel_ref.solve bit for bit
(tests/test_soft_host.py).

  expand_soft(soft, N, nb)            None / (nb,) / (N, nb) -> (L,) weights, inf = hard
  soft_clip(v, lo, hi, kap)           the four operations above, elementwise
  prox(v, lo, hi, un, kap, m, skap)   the z-update of a soft handle
  solve(p, ...)                       the batch loop on a Problem with p.soft -> admm_ref.Result
  report(p, z, soft)                  penalty (an fma chain in row order, exact rationals rounded once per step), largest
                                      violation and violated rows per QP over the rows with a finite weight
  conditions(p, z, y, rho, soft)      optimality conditions of the soft problem at (z, mu = rho y), from tests/_indep.py
"""
import os
import sys
from fractions import Fraction

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from admm_ref import Result, converged, expand_bounds, expand_unorm, factor, residuals, x_update  # noqa: E402
import _fuel_ref as fr  # noqa: E402


def expand_soft(soft, N, nb):
    if soft is None:
        return np.full(N * nb, np.inf)
    return np.broadcast_to(np.asarray(soft, np.float64), (N, nb)).reshape(-1).copy()


def soft_clip(v, lo, hi, kap):
    c = np.minimum(np.maximum(v, lo), hi)
    e = v - c
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(e) <= kap, c, np.where(e > 0, v - kap, v + kap))


def prox(v, lo, hi, un, kap, m, skap):
    """v: (batch, L); lo, hi, skap: (L,); un, kap: (N,)."""
    zn = soft_clip(v, lo, hi, skap)
    soc = np.isfinite(un) | (kap > 0)
    if soc.any():
        N = un.shape[0]
        nb = v.shape[1] // N
        zh = fr.prox(v, lo, hi, un, kap, m).reshape(v.shape[0], N, nb)
        zn.reshape(v.shape[0], N, nb)[:, soc, :m] = zh[:, soc, :m]
    return zn


def solve(p, rho=1.0, alpha=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=10, z0=None, y0=None,
          record=None, stop=True, adapt_interval=0, adapt_max=16, adapt_mu=10.0, adapt_tau=2.0, fuel="problem", soft="problem",
          decisions=None) -> Result:
    """_fuel_ref.solve's loop (same arguments, same Result) with the soft prox; soft overrides p.soft.  decisions: a list that
    receives (iteration, R, S, rho after the decision) at every decision of the adaptive rule."""
    x0 = np.atleast_2d(np.asarray(p.x0, np.float64))
    batch, N = x0.shape[0], p.N
    f = factor(p.A, p.B, p.Q, p.R, p.QN, rho, N)
    n, m = f.B.shape[1], f.B.shape[2]
    nb = n + m
    L = N * nb
    lo, hi = expand_bounds(p.lo, p.hi, N, nb)
    un = expand_unorm(p.unorm, N)
    fu = fr.expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
    sw = expand_soft(p.soft if isinstance(soft, str) else soft, N, nb)
    z = np.zeros((batch, L)) if z0 is None else np.array(z0, np.float64).reshape(batch, L)
    y = np.zeros((batch, L)) if y0 is None else np.array(y0, np.float64).reshape(batch, L)
    qq = None if p.q is None else np.asarray(p.q, np.float64).reshape(batch, L)
    w = np.zeros((batch, L))
    iters = np.full(batch, max_iter, np.int32)
    status = np.zeros(batch, np.int32)
    r = np.full(batch, np.inf)
    s = np.full(batch, np.inf)
    history = []
    it = 0
    n_updates = 0
    for it in range(1, max_iter + 1):
        g = -rho * (z - y)
        if qq is not None:
            g = g + qq
        w = x_update(f, g, x0)
        wh = alpha * w + (1.0 - alpha) * z if alpha != 1.0 else w
        v = wh + y
        zn = prox(v, lo, hi, un, fu / rho, m, sw / rho)
        yn = v - zn
        check = (it % check_interval == 0) or it == max_iter
        if check:
            r, s, nw, nz, ny = residuals(w, z, zn, yn, rho)
            ok = converged(r, s, nw, nz, ny, L, eps_abs, eps_rel)
            newly = ok & (status == 0)
            iters[newly] = it
            status[newly] = 1
        z, y = zn, yn
        if record is not None and it in record:
            history.append((it, w.copy(), z.copy(), y.copy()))
        if stop and check and status.all():
            break
        if (check and adapt_interval > 0 and it % adapt_interval == 0 and n_updates < adapt_max
                and it < max_iter):
            Rsum = Ssum = 0.0
            for b in range(batch):              # same summation order as admm_ref.solve
                if not status[b]:
                    Rsum += r[b] * r[b]
                    Ssum += s[b] * s[b]
            rho_new = rho
            if Rsum > adapt_mu ** 2 * Ssum:
                rho_new = rho * adapt_tau
            elif Ssum > adapt_mu ** 2 * Rsum:
                rho_new = rho / adapt_tau
            if decisions is not None:
                decisions.append((it, Rsum, Ssum, rho_new))
            if rho_new != rho:
                y = y * (rho / rho_new)
                f = factor(p.A, p.B, p.Q, p.R, p.QN, rho_new, N)
                rho = rho_new
                n_updates += 1
    return Result(w=w, z=z, y=y, iters_run=it, iters=iters, status=status,
                  r=r, s=s, history=history, rho=rho, rho_updates=n_updates)


def violation(p, z):
    """(batch, L): dist(z_i, [lo_i, hi_i]) = max(lo - z, 0, z - hi), each difference rounded once."""
    lo, hi = expand_bounds(p.lo, p.hi, p.N, p.nb)
    return np.maximum(np.maximum(lo[None] - z, 0.0), z - hi[None])


def report(p, z, soft="problem"):
    """(penalty, max_violation, n_violated) per QP, over the rows with a finite weight.  The penalty is the chain
    pen = fma(s_i, d_i, pen) in row order: each step in exact rationals, rounded once."""
    sw = expand_soft(p.soft if isinstance(soft, str) else soft, p.N, p.nb)
    d = violation(p, z)
    fin = np.isfinite(sw)
    pen = np.zeros(z.shape[0])
    for b in range(z.shape[0]):
        acc = 0.0
        for i in np.nonzero(fin & (d[b] > 0) & (sw > 0))[0]:         # (a zero product leaves the chain where it is)
            acc = float(Fraction(float(sw[i])) * Fraction(float(d[b, i])) + Fraction(acc))
        pen[b] = acc
    dm = np.where(fin[None], d, 0.0)
    return pen, dm.max(axis=1), (dm > 0).sum(axis=1).astype(np.int32)


def conditions(p, z, y, rho, soft="problem", on_bound_atol=1e-9):
    """Optimality conditions of   min 1/2 w'Pw + q'w + sum_i s_i dist(w_i, [lo_i, hi_i])  s.t. dynamics   (box problems: no thrust
    ball, no fuel) at z with mu = rho y, per QP (dict of arrays of length batch):
      feas_dyn, stat   dynamics defect and stationarity  P z + q + mu + G'nu = 0  (tests/_indep.kkt_certificate_batch)
      inside           max |mu_i| over the rows strictly inside their box
      on_bound         on a bound: the part of mu_i outside [0, s_i] (upper bound) / [-s_i, 0] (lower bound)
      outside          beyond a bound: | |mu_i| - s_i |, and the wrong sign
      feas_hard        largest violation over the rows with an infinite weight
    and n_outside, the number of rows beyond a bound."""
    import _indep
    Bt = p.batch
    sw = expand_soft(p.soft if isinstance(soft, str) else soft, p.N, p.nb)[None]
    feas_dyn, _, stat, _, _ = _indep.kkt_certificate_batch(p, z, y, rho)
    lo, hi = expand_bounds(p.lo, p.hi, p.N, p.nb)
    lo, hi = lo[None], hi[None]
    mu = rho * y
    at_lo = np.isclose(z, lo, rtol=0, atol=on_bound_atol)
    at_hi = np.isclose(z, hi, rtol=0, atol=on_bound_atol)
    above, below = (z > hi) & ~at_hi, (z < lo) & ~at_lo
    inside = ~(at_lo | at_hi | above | below)
    swf = np.where(np.isfinite(sw), sw, 0.0)
    e_in = np.where(inside, np.abs(mu), 0.0)
    e_hi = np.where(at_hi & ~at_lo, np.maximum(-mu, 0.0) + np.where(np.isfinite(sw), np.maximum(mu - swf, 0.0), 0.0), 0.0)
    e_lo = np.where(at_lo & ~at_hi, np.maximum(mu, 0.0) + np.where(np.isfinite(sw), np.maximum(-mu - swf, 0.0), 0.0), 0.0)
    e_pin = np.where(at_lo & at_hi & np.isfinite(sw), np.maximum(np.abs(mu) - swf, 0.0), 0.0)
    e_out = np.where(above, np.abs(mu - swf), 0.0) + np.where(below, np.abs(mu + swf), 0.0)
    hard = ~np.isfinite(sw)
    feas_hard = np.where(hard, np.maximum(np.maximum(lo - z, 0.0), z - hi), 0.0)
    mx = lambda a: np.broadcast_to(a, z.shape).reshape(Bt, -1).max(axis=1)
    return dict(feas_dyn=feas_dyn, stat=stat, inside=mx(e_in), on_bound=np.maximum(np.maximum(mx(e_hi), mx(e_lo)), mx(e_pin)),
                outside=mx(e_out), feas_hard=mx(feas_hard), n_outside=(above | below).reshape(Bt, -1).sum(axis=1))
