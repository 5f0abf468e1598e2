"""Reference of scenario consensus for the tests: tests/_fuel_ref.py::solve's loop with the z-update

    state rows     z = clip(v),  y = v - z                                                   (per QP)
    control rows   vbar = mean of v over the group,  zbar = prox(vbar),  z_b = zbar,  y_b = v_b - zbar

-- the group mean by NumPy, then _fuel_ref.prox on the mean, broadcast back -- and nothing else: factor, x_update, residuals,
converged, expand_bounds, expand_unorm come from oracle/admm_ref.py and expand_fuel / prox from _fuel_ref.py, as _fuel_ref.py
takes them.  With group size 1 the loop is _fuel_ref.solve bit for bit (tests/test_consensus_host.py).

  prox(v, lo, hi, un, kap, m, G)      the z-update projection onto box x {control rows equal within a group}
  solve(p, ...)                        the batch loop on a Problem with p.consensus set -> admm_ref.Result
  coupled_conditions(p, z, y, rho)     optimality conditions of the coupled problem at (z, mu = rho y), from tests/_indep.py
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from admm_ref import Result, converged, expand_bounds, expand_unorm, factor, residuals, x_update  # noqa: E402
import _fuel_ref as fr  # noqa: E402


def prox(v, lo, hi, un, kap, m, G):
    """v: (batch, L), batch = ngroups * G; the rest as _fuel_ref.prox."""
    batch, L = v.shape
    N = un.shape[0]
    nb = L // N
    zn = fr.prox(v, lo, hi, un, kap, m)                                   # state rows: per QP
    vbar = v.reshape(batch // G, G, L).mean(axis=1)                       # (ngroups, L); its control rows are what is used
    zbar = fr.prox(vbar, lo, hi, un, kap, m).reshape(batch // G, 1, N, nb)
    zn.reshape(batch // G, G, N, nb)[:, :, :, :m] = zbar[:, :, :, :m]
    return zn


def solve(p, rho=1.0, alpha=1.0, eps_abs=1e-6, eps_rel=1e-6, max_iter=1000, check_interval=10, z0=None, y0=None,
          record=None, stop=True, adapt_interval=0, adapt_max=16, adapt_mu=10.0, adapt_tau=2.0, fuel="problem", group=None,
          decisions=None) -> Result:
    """_fuel_ref.solve's loop (same arguments, same Result) with the group prox; group overrides p.consensus.  decisions: a list
    that receives (iteration, R, S, rho after the decision) at every decision of the adaptive rule."""
    G = int(p.consensus if group is None else group)
    x0 = np.atleast_2d(np.asarray(p.x0, np.float64))
    batch, N = x0.shape[0], p.N
    assert G >= 1 and batch % G == 0
    f = factor(p.A, p.B, p.Q, p.R, p.QN, rho, N)
    n, m = f.B.shape[1], f.B.shape[2]
    nb = n + m
    L = N * nb
    lo, hi = expand_bounds(p.lo, p.hi, N, nb)
    un = expand_unorm(p.unorm, N)
    fu = fr.expand_fuel(p.fuel if isinstance(fuel, str) else fuel, N)
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
        zn = prox(v, lo, hi, un, fu / rho, m, G)
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


def consensus_of(p, z, group=None):
    """(ngroups, N, m): the control rows of each group's first QP."""
    G = int(p.consensus if group is None else group)
    return z.reshape(p.batch // G, G, p.N, p.nb)[:, 0, :, :p.m].copy()


def coupled_conditions(p, z, y, rho, group=None):
    """Optimality conditions of the coupled problem (box constraints, no thrust ball, no fuel) at z with mu_b = rho y_b:
      feas_dyn, feas_box, stat   per QP, tests/_indep.kkt_certificate_batch: dynamics, box, P z_b + q_b + mu_b + G'nu_b = 0
      comp                       per QP: box complementarity of the STATE rows with mu_b, and of the control rows with the
                                 group's SUM of mu_u -- sum_b rho y_{u,b} in N_box(ubar): zero inside, signed at a bound
      spread                     max over groups of the spread of the control rows within a group (0: consensus is exact)
    -> dict of arrays of length batch (spread: a float), and n_active of the second evaluation."""
    import _indep
    G = int(p.consensus if group is None else group)
    Bt, N, nb, m = p.batch, p.N, p.nb, p.m
    feas_dyn, feas_box, stat, _, _ = _indep.kkt_certificate_batch(p, z, y, rho)
    Y = y.reshape(Bt // G, G, N, nb).copy()
    Y[:, :, :, :m] = Y[:, :, :, :m].sum(axis=1, keepdims=True)
    _, _, _, comp, n_active = _indep.kkt_certificate_batch(p, z, Y.reshape(Bt, -1), rho)
    U = z.reshape(Bt // G, G, N, nb)[:, :, :, :m]
    spread = float(np.abs(U - U[:, :1]).max())
    return dict(feas_dyn=feas_dyn, feas_box=feas_box, stat=stat, comp=comp, spread=spread), n_active
