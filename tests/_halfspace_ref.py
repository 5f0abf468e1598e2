"""Reference of one half-space per stage  a_k . xi_k <= b_k   for the tests: oracle/admm_ref.py::solve's loop
(as tests/_fuel_ref.py restates it) with the z-update

    nn = a.a,  d = a.v - b,  t = d > 0 ? d / nn : 0,  z = v - t a,  y = v - z

on xi_k = the first nh state rows of every stage whose a_k is not 0, _fuel_ref.prox on every other row -- and nothing else:
factor, x_update, residuals, converged, expand_bounds, expand_unorm come from oracle/admm_ref.py and expand_fuel / prox from
_fuel_ref.py, as _fuel_ref.py takes them.  With every a = 0 the loop is admm_ref.solve bit for bit (tests/test_halfspace_host.py).

  planes(p, a, b)                     (batch, N, nh), (batch, N) from the shared or the per-QP form (default: p.hs_a, p.hs_b)
  project(a, b, v)                    the prox of one stage in exact fma chains (Fractions, rounded once per step): the bits
                                      admm_prox.hpp's halfspace_project must give; None where a = 0
  prox(v, lo, hi, un, kap, m, A, Bv)  the z-update of a half-space handle (NumPy arithmetic: within an ulp or two of project)
  solve(p, ...)                       the batch loop on a Problem with p.hs_a / p.hs_b -> admm_ref.Result
  stage_kinds(p, res_or_v...)         per QP the number of active stages, of stages satisfied with t = 0, of stages with a = 0
  report(p, w, y, rho)                max_violation, n_active, lam per QP as admm_get_halfspace_report defines them
  conditions(p, z, y, rho)            optimality conditions of the constrained QP at (z, mu = rho y)
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


def planes(p, a=None, b=None):
    a = np.asarray(p.hs_a if a is None else a, np.float64)
    b = np.asarray(p.hs_b if b is None else b, np.float64)
    if a.ndim == 2:
        a, b = np.broadcast_to(a, (p.batch,) + a.shape), np.broadcast_to(b, (p.batch,) + b.shape)
    return np.array(a), np.array(b)


def _fma(x, y, z):
    return float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))


def project(a, b, v):
    """One stage, exactly as specified: (z, y) of the nh rows, or None if a.a == 0 (no half-space)."""
    nn, d = 0.0, -float(b)
    for ai in a:
        nn = _fma(ai, ai, nn)
    for ai, vi in zip(a, v):
        d = _fma(ai, vi, d)
    if nn == 0.0:
        return None
    t = d / nn if d > 0.0 else 0.0
    z = np.array([_fma(-t, ai, vi) for ai, vi in zip(a, v)])
    return z, np.asarray(v, np.float64) - z


def prox(v, lo, hi, un, kap, m, A, Bv):
    """v: (batch, L); lo, hi: (L,); un, kap: (N,); A: (batch, N, nh); Bv: (batch, N)."""
    zn = fr.prox(v, lo, hi, un, kap, m)
    batch, N, nh = A.shape
    nb = v.shape[1] // N
    vx = v.reshape(batch, N, nb)[:, :, m:m + nh]
    nn = np.sum(A * A, axis=2)
    act = nn != 0.0
    d = np.sum(A * vx, axis=2) - Bv
    t = np.where(act & (d > 0), d / np.where(act, nn, 1.0), 0.0)
    zx = zn.reshape(batch, N, nb)[:, :, m:m + nh]
    zx[...] = np.where(act[:, :, None], vx - t[:, :, None] * A, zx)
    return zn


def solve(p, rho=1.0, alpha=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=10, z0=None, y0=None,
          record=None, stop=True, adapt_interval=0, adapt_max=16, adapt_mu=10.0, adapt_tau=2.0, fuel="problem", hs=None,
          decisions=None, last_v=None) -> Result:
    """_fuel_ref.solve's loop (same arguments, same Result) with the half-space prox; hs = (a, b) overrides p.hs_a / p.hs_b.
    decisions: a list that receives (iteration, rho after the decision) at every decision of the adaptive rule; last_v: a list
    that receives v of the last iteration."""
    x0 = np.atleast_2d(np.asarray(p.x0, np.float64))
    batch, N = x0.shape[0], p.N
    f = factor(p.A, p.B, p.Q, p.R, p.QN, rho, N)
    n, m = f.B.shape[1], f.B.shape[2]
    nb = n + m
    L = N * nb
    lo, hi = expand_bounds(p.lo, p.hi, N, nb)
    un = expand_unorm(p.unorm, N)
    fu = fr.expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
    A, Bv = planes(p, *(hs or (None, None)))
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
    v = None
    for it in range(1, max_iter + 1):
        g = -rho * (z - y)
        if qq is not None:
            g = g + qq
        w = x_update(f, g, x0)
        wh = alpha * w + (1.0 - alpha) * z if alpha != 1.0 else w
        v = wh + y
        zn = prox(v, lo, hi, un, fu / rho, m, A, Bv)
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
                decisions.append((it, rho_new))
            if rho_new != rho:
                y = y * (rho / rho_new)
                f = factor(p.A, p.B, p.Q, p.R, p.QN, rho_new, N)
                rho = rho_new
                n_updates += 1
    if last_v is not None:
        last_v.append(v)
    return Result(w=w, z=z, y=y, iters_run=it, iters=iters, status=status,
                  r=r, s=s, history=history, rho=rho, rho_updates=n_updates)


def stage_kinds(p, v, hs=None):
    """Per QP, at the z-update input v (batch, L): (stages with d > 0, stages with a plane and d <= 0, stages with a = 0)."""
    A, Bv = planes(p, *(hs or (None, None)))
    nh = A.shape[2]
    vx = v.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
    act = np.sum(A * A, axis=2) != 0.0
    d = np.sum(A * vx, axis=2) - Bv
    return (act & (d > 0)).sum(axis=1), (act & (d <= 0)).sum(axis=1), (~act).sum(axis=1)


def report(p, w, y, rho, hs=None):
    """(max_violation, n_active, lam) per QP: max_k (a_k . w_xi - b_k)+ / |a_k|;  stages with lam_k > 0;
    lam (batch, N) = rho (a_k . y_xi) / a_k . a_k, 0 where a_k = 0."""
    A, Bv = planes(p, *(hs or (None, None)))
    nh = A.shape[2]
    wx = w.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
    yx = y.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
    nn = np.sum(A * A, axis=2)
    act = nn != 0.0
    nn1 = np.where(act, nn, 1.0)
    viol = np.where(act, np.maximum(np.sum(A * wx, axis=2) - Bv, 0.0) / np.sqrt(nn1), 0.0)
    lam = np.where(act, rho * np.sum(A * yx, axis=2) / nn1, 0.0)
    return viol.max(axis=1), (lam > 0).sum(axis=1).astype(np.int32), lam


def conditions(p, z, y, rho, hs=None, active_rtol=1e-9):
    """Optimality conditions of   min 1/2 w'Pw + q'w [+ fuel]  s.t. dynamics, box / ball, a_k . xi_k <= b_k   at z with mu = rho y, per QP
    (dict of arrays of length batch):
      feas_dyn, stat   dynamics defect and stationarity  P z + q + mu + G'nu = 0  (tests/_indep.kkt_certificate_batch)
      feas_plane       max_k (a_k . z_xi - b_k)+ / |a_k|
      normal           on the stages with a plane: |mu_xi - lam a| with lam = (a . mu_xi) / a.a  (mu_xi is a multiple of a), relative to rho
      sign             (-lam)+ |a|: the multiplier must not pull into the plane
      comp             lam |a . z_xi - b| / |a|: complementarity
    The rows outside xi of such stages, and all rows of the others, are the box / ball problem's (tests/_fuel_ref.certificate)."""
    import _indep
    A, Bv = planes(p, *(hs or (None, None)))
    nh = A.shape[2]
    Bt = p.batch
    feas_dyn, _, stat, _, _ = _indep.kkt_certificate_batch(p, z, y, rho)
    zx = z.reshape(Bt, p.N, p.nb)[:, :, p.m:p.m + nh]
    mux = rho * y.reshape(Bt, p.N, p.nb)[:, :, p.m:p.m + nh]
    nn = np.sum(A * A, axis=2)
    act = nn != 0.0
    nn1 = np.where(act, nn, 1.0)
    na = np.sqrt(nn1)
    gap = np.sum(A * zx, axis=2) - Bv
    lam = np.where(act, np.sum(A * mux, axis=2) / nn1, 0.0)
    feas_plane = np.where(act, np.maximum(gap, 0.0) / na, 0.0).max(axis=1)
    normal = np.where(act[:, :, None], np.abs(mux - lam[:, :, None] * A), 0.0).reshape(Bt, -1).max(axis=1)
    sign = np.where(act, np.maximum(-lam, 0.0) * na, 0.0).max(axis=1)
    comp = np.where(act, np.abs(lam * gap) / na, 0.0).max(axis=1)
    return dict(feas_dyn=feas_dyn, stat=stat, feas_plane=feas_plane, normal=normal, sign=sign, comp=comp,
                n_active=(act & (lam > 0)).sum(axis=1))
