"""Reference of one approach cone per stage  r <= g s   for the tests: oracle/admm_ref.py::solve's loop (as
tests/_fuel_ref.py restates it) with the z-update

    dl = v - p,  nn = c.c,  d = c.dl,  q = dl.dl,  rn = sqrt(nn),  s = d / rn,  r = sqrt(max(q - s^2, 0))
    r <= g s: z = v;   else g r <= -s: z = p;   else t = (g r + s) / (1 + g^2), bet = g t / r, kap = (t - bet s) / rn,
                                                     z = p + bet dl + kap c;         y = v - z

on xi_k = the first nh state rows of every stage whose c_k is not 0, _fuel_ref.prox on every other row -- and nothing else:
factor, x_update, residuals, converged, expand_bounds, expand_unorm come from oracle/admm_ref.py and expand_fuel / prox from
_fuel_ref.py, as _fuel_ref.py takes them.  With every c = 0 the loop is admm_ref.solve bit for bit (tests/test_cone_host.py).

  cones(p, c, apex, g)                (batch, N, nh) twice, (batch, N) from the shared or the per-QP form (default: p.cone_*)
  project(c, apex, g, v)              the prox of one stage in exact fma chains (Fractions, rounded once per step; math.sqrt and
                                      float division are correctly rounded): the bits admm_prox.hpp's cone_project must give;
                                      None where c = 0, else (z, y, branch)
  prox(v, lo, hi, un, kap, m, C, Pa, G)  the z-update of a cone handle (NumPy arithmetic: within a few ulps of project)
  solve(p, ...)                       the batch loop on a Problem with p.cone_c / cone_p / cone_g -> admm_ref.Result
  stage_kinds(p, v)                   over the batch, at the z-update input v: the number of stages inside, at the apex, on the
                                      surface and without a cone
  report(p, w, y, rho)                max_violation, n_active, lam per QP as admm_get_cone_report defines them
  conditions(p, z, y, rho)            optimality conditions of the constrained QP at (z, mu = rho y)
"""
import math
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

INSIDE, APEX, SURFACE = 0, 1, 2


def cones(p, c=None, apex=None, g=None):
    c = np.asarray(p.cone_c if c is None else c, np.float64)
    apex = np.asarray(p.cone_p if apex is None else apex, np.float64)
    g = np.asarray(p.cone_g if g is None else g, np.float64)
    if c.ndim == 2:
        c, apex, g = (np.broadcast_to(x, (p.batch,) + x.shape) for x in (c, apex, g))
    return np.array(c), np.array(apex), np.array(g)


def _fma(x, y, z):
    return float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))


def project(c, apex, g, v):
    """One stage, exactly as specified: (z, y, branch) of the nh rows, or None if c.c == 0 (no cone)."""
    c, apex, v = (np.asarray(x, np.float64) for x in (c, apex, v))
    g = float(g)
    dl = v - apex
    nn = d = q = 0.0
    for ci, di in zip(c, dl):
        nn = _fma(ci, ci, nn)
        d = _fma(ci, di, d)
        q = _fma(di, di, q)
    if nn == 0.0:
        return None
    rn = math.sqrt(nn)
    s = d / rn
    r = math.sqrt(max(_fma(-s, s, q), 0.0))
    if r <= g * s:
        z, branch = v.copy(), INSIDE
    elif g * r <= -s:
        z, branch = apex.copy(), APEX
    else:
        t = _fma(g, r, s) / _fma(g, g, 1.0)
        bet = (g * t) / r
        kap = (t - bet * s) / rn
        z, branch = np.array([_fma(kap, ci, _fma(bet, di, pi)) for ci, di, pi in zip(c, dl, apex)]), SURFACE
    return z, v - z, branch


def _coords(C, Pa, x):
    """(act, s, r, dl, rn) of the points x (batch, N, nh) in the cones' coordinates (s, r arbitrary where a stage has no cone)."""
    nn = np.sum(C * C, axis=2)
    act = nn != 0.0
    rn = np.sqrt(np.where(act, nn, 1.0))
    dl = x - Pa
    s = np.sum(C * dl, axis=2) / rn
    r = np.sqrt(np.maximum(np.sum(dl * dl, axis=2) - s * s, 0.0))
    return act, s, r, dl, rn


def branches(C, Pa, G, vx):
    """(batch, N): INSIDE / APEX / SURFACE, -1 where the stage has no cone."""
    act, s, r, _, _ = _coords(C, Pa, vx)
    br = np.where(r <= G * s, INSIDE, np.where(G * r <= -s, APEX, SURFACE))
    return np.where(act, br, -1)


def prox(v, lo, hi, un, kap, m, C, Pa, G):
    """v: (batch, L); lo, hi: (L,); un, kap: (N,); C, Pa: (batch, N, nh); G: (batch, N)."""
    zn = fr.prox(v, lo, hi, un, kap, m)
    batch, N, nh = C.shape
    nb = v.shape[1] // N
    vx = v.reshape(batch, N, nb)[:, :, m:m + nh]
    act, s, r, dl, rn = _coords(C, Pa, vx)
    br = np.where(r <= G * s, INSIDE, np.where(G * r <= -s, APEX, SURFACE))
    t = (G * r + s) / (G * G + 1.0)
    bet = G * t / np.where(br == SURFACE, r, 1.0)
    kp = (t - bet * s) / rn
    surf = Pa + bet[:, :, None] * dl + kp[:, :, None] * C
    z = np.where((br == INSIDE)[:, :, None], vx, np.where((br == APEX)[:, :, None], Pa, surf))
    zx = zn.reshape(batch, N, nb)[:, :, m:m + nh]
    zx[...] = np.where(act[:, :, None], z, zx)
    return zn


def solve(p, rho=1.0, alpha=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=10, z0=None, y0=None,
          record=None, stop=True, adapt_interval=0, adapt_max=16, adapt_mu=10.0, adapt_tau=2.0, fuel="problem", cone=None,
          decisions=None, kinds=None) -> Result:
    """_fuel_ref.solve's loop (same arguments, same Result) with the cone prox; cone = (c, apex, g) overrides p.cone_*.
    decisions: a list that receives (iteration, rho after the decision) at every decision of the adaptive rule; kinds: a list that
    receives stage_kinds of every iteration's v."""
    x0 = np.atleast_2d(np.asarray(p.x0, np.float64))
    batch, N = x0.shape[0], p.N
    f = factor(p.A, p.B, p.Q, p.R, p.QN, rho, N)
    n, m = f.B.shape[1], f.B.shape[2]
    nb = n + m
    L = N * nb
    lo, hi = expand_bounds(p.lo, p.hi, N, nb)
    un = expand_unorm(p.unorm, N)
    fu = fr.expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
    C, Pa, G = cones(p, *(cone or (None, None, None)))
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
        if kinds is not None:
            kinds.append(stage_kinds(p, v, cone))
        zn = prox(v, lo, hi, un, fu / rho, m, C, Pa, G)
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
    return Result(w=w, z=z, y=y, iters_run=it, iters=iters, status=status,
                  r=r, s=s, history=history, rho=rho, rho_updates=n_updates)


def stage_kinds(p, v, cone=None):
    """Over the batch, at the z-update input v (batch, L): the number of stages (inside, at the apex, on the surface, without a
    cone)."""
    C, Pa, G = cones(p, *(cone or (None, None, None)))
    nh = C.shape[2]
    br = branches(C, Pa, G, v.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh])
    return tuple(int((br == k).sum()) for k in (INSIDE, APEX, SURFACE, -1))


def report(p, w, y, rho, cone=None):
    """(max_violation, n_active, lam) per QP: max_k (r_k - g_k s_k)+ / sqrt(1 + g_k^2) at w_xi;  stages with a cone whose y_xi has a
    nonzero entry;  lam (batch, N) = rho |y_xi|_2, 0 where c_k = 0."""
    C, Pa, G = cones(p, *(cone or (None, None, None)))
    nh = C.shape[2]
    wx = w.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
    yx = y.reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
    act, s, r, _, _ = _coords(C, Pa, wx)
    viol = np.where(act, np.maximum(r - G * s, 0.0) / np.sqrt(1.0 + G * G), 0.0)
    lam = np.where(act, rho * np.sqrt(np.sum(yx * yx, axis=2)), 0.0)
    return viol.max(axis=1), (act & np.any(yx != 0.0, axis=2)).sum(axis=1).astype(np.int32), lam


def conditions(p, z, y, rho, cone=None):
    """Optimality conditions of   min 1/2 w'Pw + q'w [+ fuel]  s.t. dynamics, box / ball, xi_k - p_k in K_k   at z with mu = rho y, per QP
    (dict of arrays of length batch):
      feas_dyn, stat   dynamics defect and stationarity  P z + q + mu + G'nu = 0  (tests/_indep.kkt_certificate_batch)
      feas_cone        max_k (r - g s)+ / sqrt(1 + g^2) of z_xi - p: z_xi - p in the cone
      polar            max_k (g r_mu + s_mu)+ / sqrt(1 + g^2) of mu_xi: mu_xi in the polar cone  { g r <= -s }
      comp             max_k |mu_xi . (z_xi - p)|: complementarity
    The rows outside xi of such stages, and all rows of the others, are the box / ball problem's (tests/_fuel_ref.certificate)."""
    import _indep
    C, Pa, G = cones(p, *(cone or (None, None, None)))
    nh = C.shape[2]
    Bt = p.batch
    feas_dyn, _, stat, _, _ = _indep.kkt_certificate_batch(p, z, y, rho)
    zx = z.reshape(Bt, p.N, p.nb)[:, :, p.m:p.m + nh]
    mux = rho * y.reshape(Bt, p.N, p.nb)[:, :, p.m:p.m + nh]
    act, s, r, dl, rn = _coords(C, Pa, zx)
    sm = np.sum(C * mux, axis=2) / rn
    rm = np.sqrt(np.maximum(np.sum(mux * mux, axis=2) - sm * sm, 0.0))
    nrm = np.sqrt(1.0 + G * G)
    feas_cone = np.where(act, np.maximum(r - G * s, 0.0) / nrm, 0.0).max(axis=1)
    polar = np.where(act, np.maximum(G * rm + sm, 0.0) / nrm, 0.0).max(axis=1)
    comp = np.where(act, np.abs(np.sum(mux * dl, axis=2)), 0.0).max(axis=1)
    on = act & np.any(mux != 0.0, axis=2)
    return dict(feas_dyn=feas_dyn, stat=stat, feas_cone=feas_cone, polar=polar, comp=comp, n_active=on.sum(axis=1))
