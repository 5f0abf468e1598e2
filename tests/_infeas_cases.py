"""The four classification problems of the infeasibility probe, shared by tests/test_infeas_host.py (oracle
iterates) and tests/test_gpu_infeas.py (the handle's): problem, the two iterations at which y is taken, the expected flags and the
values of sep the NumPy reference gives on the oracle's iterates (rho = 1)."""
import dataclasses

import numpy as np

import admm_library_amd as pkg

RHO = 1.0
EPS = 1e-6


def per_stage(p):
    """The box of p as (N, nb) arrays."""
    return dataclasses.replace(p, lo=np.array(np.broadcast_to(p.lo, (p.N, p.nb))), hi=np.array(np.broadcast_to(p.hi, (p.N, p.nb))))


def pin_terminal(p):
    """x_N = 0."""
    p = per_stage(p)
    p.lo[-1, p.m:] = 0.0
    p.hi[-1, p.m:] = 0.0
    return p


def di_pinned(N=12):
    p = pkg.double_integrator(N=N, batch=6)
    x0 = np.array([[0.5, 0.0], [1.0, 0.5], [3.0, 0.0], [6.0, 1.0], [10.0, 0.0], [-8.0, -1.0]])
    return pin_terminal(dataclasses.replace(p, x0=x0))


def di_position_box(N=12):
    p = per_stage(pkg.double_integrator(N=N, batch=4))
    p.lo[:, p.m] = -1.0
    p.hi[:, p.m] = 1.0
    return dataclasses.replace(p, x0=np.array([[0.9, 0.0], [0.9, 3.0], [0.0, 8.0], [-0.5, -6.0]]))


def cw_pinned():
    p = pkg.cw_rendezvous(N=16, batch=4)
    return pin_terminal(dataclasses.replace(p, x0=p.x0 * np.array([0.01, 1.0, 5.0, 20.0])[:, None]))


def cw_pinned_ball():
    p = cw_pinned()
    p.lo[:, :p.m] = -np.inf
    p.hi[:, :p.m] = np.inf
    return dataclasses.replace(p, unorm=np.float64(0.2))


# id -> (factory, (iteration of the snapshot, of the second y), flags, sep to three digits (the reference on the oracle's iterates), linprog applies)
CASES = {
    "di_pinned": (di_pinned, (200, 210), [0, 1, 1, 1, 1, 1], [3.24, -0.23, -1.48, -5.98, -8.15, -7.97], True),
    "di_position_box": (di_position_box, (100, 110), [0, 1, 1, 1], [np.inf, -11.8, -34.8, -26.0], True),
    "cw_pinned": (cw_pinned, (1000, 1010), [0, 0, 1, 1], [2.11, 2.07, -1.38, -10.1], True),
    "cw_pinned_ball": (cw_pinned_ball, (1000, 1010), [0, 0, 1, 1], [1.65, 1.65, -1.66, -10.3], False),
}

_CACHE = {}


def oracle_probe(case):
    """(problem, y at the two iterations from oracle/admm_ref.solve with stop=False, the reference's probe of them); computed once."""
    if case not in _CACHE:
        import admm_ref
        import _infeas_ref as ir
        make, its, _, _, _ = CASES[case]
        p = make()
        res = admm_ref.solve(p.A, p.B, p.Q, p.R, p.QN, p.x0, p.lo, p.hi, p.N, q=p.q, rho=RHO, max_iter=its[1], stop=False,
                             record=set(its), unorm=p.unorm)
        (ia, _, _, ya), (ib, _, _, yb) = res.history
        assert (ia, ib) == its
        _CACHE[case] = (p, ya, yb, ir.probe(p, ya, yb, its[1] - its[0], EPS))
    return _CACHE[case]
