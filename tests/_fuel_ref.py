"""Reference of the minimum-fuel cost  + sum_k f_k ||u_k||_2   for the tests.

The C oracle under oracle/ does not know the term, so this restates the batch loop of oracle/admm_ref.py::solve with the
prox of the term in the z-update -- and nothing else: factor, x_update, residuals, converged, expand_bounds, expand_unorm are
IMPORTED from admm_ref (same Riccati form, same adaptive-rho rule, same summation order).  With fuel = 0 the loop is
admm_ref.solve bit for bit (tests/test_fuel_host.py).

  prox(v, lo, hi, un, kap, m)   z-update projection: box on every row; the control rows of a stage with a finite thrust bound
                                un_k or kap_k = f_k / rho > 0 are shrunk by kap_k, then scaled onto the ball ||u|| <= un_k
  solve(p, ...)                 the batch loop on a Problem (p.fuel, p.unorm, p.q) -> admm_ref.Result
  certificate(p, z, y, rho)     optimality conditions of the fuel problem at (z, mu = rho y), from the pieces of tests/_indep.py
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from admm_ref import Result, converged, expand_bounds, expand_unorm, factor, residuals, x_update  # noqa: E402


def expand_fuel(fuel, N):
    """None / scalar / (N,) -> (N,) weights, 0 = none."""
    if fuel is None:
        return np.zeros(N)
    return np.broadcast_to(np.asarray(fuel, np.float64), (N,)).copy()


def prox(v, lo, hi, un, kap, m):
    """v: (batch, L); lo, hi: (L,); un, kap: (N,).
        nrm = ||v_u||,  t = min(un, max(nrm - kap, 0)),  c = nrm > t ? t / nrm : 1,  z_u = c v_u
    on the control rows of the stages with a finite bound or kap > 0; the box elsewhere."""
    zn = np.minimum(np.maximum(v, lo), hi)
    soc = np.isfinite(un) | (kap > 0)
    if soc.any():
        N = un.shape[0]
        nb = v.shape[1] // N
        vb = v.reshape(v.shape[0], N, nb)
        zb = zn.reshape(v.shape[0], N, nb)
        nrm = np.sqrt(np.sum(vb[:, :, :m] ** 2, axis=2))
        t = np.minimum(un[None, :], np.maximum(nrm - kap[None, :], 0.0))
        scale = np.where(nrm > t, t / np.where(nrm > 0, nrm, 1.0), 1.0)
        zb[:, soc, :m] = vb[:, soc, :m] * scale[:, soc, None]
    return zn


def solve(p, rho=1.0, alpha=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=10, z0=None, y0=None,
          record=None, stop=True, adapt_interval=0, adapt_max=16, adapt_mu=10.0, adapt_tau=2.0, fuel="problem") -> Result:
    """admm_ref.solve's loop (same arguments, same Result) on Problem p with the fuel prox; fuel overrides p.fuel."""
    x0 = np.atleast_2d(np.asarray(p.x0, np.float64))
    batch, N = x0.shape[0], p.N
    f = factor(p.A, p.B, p.Q, p.R, p.QN, rho, N)
    n, m = f.B.shape[1], f.B.shape[2]
    nb = n + m
    L = N * nb
    lo, hi = expand_bounds(p.lo, p.hi, N, nb)
    un = expand_unorm(p.unorm, N)
    fu = expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
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
        zn = prox(v, lo, hi, un, fu / rho, m)
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
            if rho_new != rho:
                y = y * (rho / rho_new)
                f = factor(p.A, p.B, p.Q, p.R, p.QN, rho_new, N)
                rho = rho_new
                n_updates += 1
    return Result(w=w, z=z, y=y, iters_run=it, iters=iters, status=status,
                  r=r, s=s, history=history, rho=rho, rho_updates=n_updates)


def last_residuals(p, w, z_old, z, y, rho):
    """(r, s) of the iteration that produced (w, z, y) from z_old."""
    r, s, _, _, _ = residuals(w, z_old, z, y, rho)
    return r, s


def certificate(p, z, y, rho, fuel="problem", on_bound_rtol=1e-9):
    """Optimality conditions of   min 1/2 w'Pw + q'w + sum_k f_k ||u_k||  s.t. dynamics, state box, ||u_k|| <= un_k   at z with
    the multiplier mu = rho y of the non-smooth part, per QP (dict of arrays of length batch):
      feas_dyn, stat   dynamics defect and stationarity  P z + q + mu + G'nu = 0  of the QP (tests/_indep.kkt_certificate_batch)
      feas_ball        max_k (||z_u,k|| - un_k)+ / un_k
      fuel             the control rows of mu lie in  f d||.||(z_u) + N_ball(z_u):
                         0 < ||z_u|| < un:  |mu_u - f z_u / ||z_u|||
                         z_u = 0:           (||mu_u|| - f)+
                         ||z_u|| = un:      the part of mu_u orthogonal to z_u, and (f - mu_u . z_u / ||z_u||)+
                       (control rows of a stage with neither a bound nor a weight: their box, as comp_x)
      comp_x           box complementarity of the state rows (and of such control rows), as kkt_certificate_batch
    and the per-QP counts n_coast, n_mid, n_bound of stages."""
    import _indep
    N, m, nb, Bt = p.N, p.m, p.nb, p.batch
    fu = expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
    un = expand_unorm(p.unorm, N)
    feas_dyn, _, stat, _, _ = _indep.kkt_certificate_batch(p, z, y, rho)
    Z = z.reshape(Bt, N, nb)
    mu = rho * y.reshape(Bt, N, nb)
    lo, hi = _indep.stage_bounds(p)
    soc = np.isfinite(un) | (fu > 0)
    zu, muu = Z[:, :, :m], mu[:, :, :m]
    nz = np.sqrt(np.sum(zu ** 2, axis=2))
    nmu = np.sqrt(np.sum(muu ** 2, axis=2))
    feas_ball = np.where(np.isfinite(un)[None], np.maximum(nz - un[None], 0.0) / np.where(np.isfinite(un), un, 1.0)[None], 0.0).max(axis=1)
    coast = soc[None] & (nz == 0.0)
    bound = soc[None] & np.isfinite(un)[None] & (nz >= un[None] * (1.0 - on_bound_rtol))
    mid = soc[None] & ~coast & ~bound
    zhat = zu / np.where(nz > 0, nz, 1.0)[:, :, None]
    along = np.sum(muu * zhat, axis=2)
    e_mid = np.abs(muu - fu[None, :, None] * zhat).max(axis=2)
    e_coast = np.maximum(nmu - fu[None], 0.0)
    e_bound = np.maximum(np.abs(muu - along[:, :, None] * zhat).max(axis=2), np.maximum(fu[None] - along, 0.0))
    e_fuel = np.where(coast, e_coast, np.where(bound, e_bound, np.where(mid, e_mid, 0.0))).max(axis=1)
    # rows under their box: all state rows, and the control rows of stages outside soc
    boxed = np.ones((N, nb), bool)
    boxed[soc, :m] = False
    at_lo = np.isclose(Z, lo[None], rtol=0, atol=1e-9)
    at_hi = np.isclose(Z, hi[None], rtol=0, atol=1e-9)
    viol = np.where(at_lo, np.maximum(mu, 0.0), np.where(at_hi, np.maximum(-mu, 0.0), np.abs(mu)))
    comp_x = np.where(boxed[None], viol, 0.0).reshape(Bt, -1).max(axis=1)
    feas_box = np.where(boxed[None], np.maximum(np.maximum(lo[None] - Z, 0.0), np.maximum(Z - hi[None], 0.0)), 0.0).reshape(Bt, -1).max(axis=1)
    return dict(feas_dyn=feas_dyn, stat=stat, feas_ball=feas_ball, feas_box=feas_box, fuel=e_fuel, comp_x=comp_x,
                n_coast=coast.sum(axis=1), n_mid=mid.sum(axis=1), n_bound=bound.sum(axis=1))
