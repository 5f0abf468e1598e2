"""Inputs and references of the SCvx adjoint tests (tests/test_scvx_adjoint_host.py, tests/test_gpu_scvx_adjoint.py; DESIGN.md
§2.8.4), built on the CPU once and shared read-only: the scatter of tests/_scvx_device_case.py with CLIPPED controls (uniform in
+-3 U_MAX clipped to the box: about a third on each bound), a restatement of the recursion of scvx.adjoint at any precision -- with
one deliberate error at a time for the mutation check --, extended-precision central differences of the nonlinear cost, and the
first-order bound on what an entrywise error of A, B does to the outputs."""
import functools

import numpy as np

from admm_library_amd import scvx as sc

import _scvx_case as case
import _scvx_device_case as dc

LD = np.longdouble
WRONG = ("A_not_transposed", "B_transposed_index", "Q_for_QN", "stage_off_by_one", "A_one_stage_late")
FD_H = 1e-3               # central differences in long double: the difference to the adjoint is flat over h = 1e-2 .. 1e-5
LIN_BOUND = 5e-7          # |device - host| on the entries of A, B (tests/test_gpu_scvx_device.py)


@functools.lru_cache(maxsize=None)
def scattered_clipped(B, N):
    """x0 (B, 6) of dc.scattered, controls uniform in +-3 U_MAX clipped to +-U_MAX (B, N, 3), their host rollout x (B, N, 6)."""
    rng = np.random.default_rng(11)
    x0 = case.X0[None] * (1.0 + 0.05 * rng.standard_normal((B, 6)))
    u = np.clip(rng.uniform(-3.0 * case.U_MAX, 3.0 * case.U_MAX, (B, N, 3)), -case.U_MAX, case.U_MAX)
    x = sc.rollout(x0, u, dc.DT)
    for a in (x0, u, x):
        a.setflags(write=False)
    return x0, u, x


@functools.lru_cache(maxsize=None)
def host_jacobians(B, N):
    """scvx.linearise about scattered_clipped(B, N)."""
    x0, u, x = scattered_clipped(B, N)
    A, Bm = sc.linearise(np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1), u, dc.DT)
    A.setflags(write=False)
    Bm.setflags(write=False)
    return A, Bm


def recursion(A, Bm, x, u, Q, R, QN, dtype=np.float64, wrong=None):
    """nu, primer, grad, dJdx0 of scvx.adjoint, restated at `dtype` with every operand converted first; wrong: one of WRONG."""
    A, Bm, x, u, Q, R, QN = (np.asarray(a, dtype) for a in (A, Bm, x, u, Q, R, QN))
    Bn, N = u.shape[:2]
    qu = u @ R.T
    qx = x @ Q.T
    if wrong != "Q_for_QN":
        qx[:, -1] = x[:, -1] @ QN.T
    At = "bij,bj->bi" if wrong == "A_not_transposed" else "bji,bj->bi"
    nu = np.empty((Bn, N, 6), dtype)
    nu[:, -1] = -qx[:, -1]
    for k in range(N - 2, -1, -1):
        nu[:, k] = np.einsum(At, A[:, k if wrong == "A_one_stage_late" else k + 1], nu[:, k + 1]) - qx[:, k]
    if wrong == "stage_off_by_one":                   # the costates stored one stage late: stage k pairs B_k with nu_{k+2}
        primer = np.zeros((Bn, N, 3), dtype)
        primer[:, :-1] = np.einsum("bkij,bki->bkj", Bm[:, :-1], nu[:, 1:])
        nu = np.concatenate([nu[:, 1:], np.zeros((Bn, 1, 6), dtype)], axis=1)
    elif wrong == "B_transposed_index":                 # the block read as if it were stored 3 x 6
        primer = np.einsum("bkji,bki->bkj", Bm.reshape(Bn, N, 3, 6), nu)
    else:
        primer = np.einsum("bkij,bki->bkj", Bm, nu)
    return dict(nu=nu, primer=primer, grad=qu - primer, dJdx0=-np.einsum(At, A[:, 0], nu[:, 0]))


def ld_cost(x0, u, p=dc.ORIGINAL):
    return dc.ld_trajectory_cost(dc.ld_rollout(x0, u, p.dt, p.substeps, p.rc), u, p.Q, p.R, p.QN)


def fd_gradients(x0, u, h=FD_H):
    """dJ/du (B, N, 3) and dJ/dx0 (B, 6) of the scenario's cost by central differences of step h, every operand long double; the
    2 (3 N + 6) perturbed trajectories per trajectory are rolled out as one batch."""
    x0, u, h = np.asarray(x0, LD), np.asarray(u, LD), LD(h)
    B, N = u.shape[:2]
    du = (h * np.eye(3 * N, dtype=LD)).reshape(3 * N, 1, N, 3)
    dx = (h * np.eye(6, dtype=LD)).reshape(6, 1, 6)
    us = np.concatenate([u[None] + du, u[None] - du, np.broadcast_to(u, (12, B, N, 3))])
    xs = np.concatenate([np.broadcast_to(x0, (6 * N, B, 6)), x0[None] + dx, x0[None] - dx])
    J = ld_cost(xs.reshape(-1, 6), us.reshape(-1, N, 3)).reshape(-1, B)
    g = ((J[:3 * N] - J[3 * N:6 * N]) / (LD(2) * h)).T.reshape(B, N, 3)
    g0 = ((J[6 * N:6 * N + 6] - J[6 * N + 6:]) / (LD(2) * h)).T
    return g, g0


FD_POINTS = ("zero", "interior", "clipped")


@functools.lru_cache(maxsize=None)
def fd_case(B, N, point):
    """x0, u, x of one point of the finite-difference test -- u = 0, uniform in +-0.9 U_MAX, or scattered_clipped's -- with the
    long-double central differences of the cost there."""
    x0, u, _ = scattered_clipped(B, N)
    if point == "zero":
        u = np.zeros_like(u)
    elif point == "interior":
        u = np.random.default_rng(5).uniform(-0.9 * case.U_MAX, 0.9 * case.U_MAX, u.shape)
    x = sc.rollout(x0, u, dc.DT)
    g, g0 = fd_gradients(x0, u)
    return x0, u, x, g, g0


def nu_scale(nu):
    """max |nu| per trajectory, as a column for (B, N, .) and (B, .) arrays alike."""
    return np.abs(np.asarray(nu, np.float64)).max(axis=(1, 2))


def scaled_errors(got, ref, scale):
    """max |got - ref| / scale[b] per output, got / ref: dicts of (B, ...) arrays (ref may be long double)."""
    out = {}
    for k, r in ref.items():
        d = np.abs(np.asarray(got[k], LD) - r)
        out[k] = float((d.reshape(d.shape[0], -1).max(axis=1) / scale).max())
    return out


def fp64_vs_ld(B, N):
    """scvx.adjoint(A=, B=) in fp64 against the long-double recursion on scattered_clipped(B, N) with the host Jacobians, per
    output, normalised by max |nu| per trajectory (stat: the same measure of |stat - stat_ld|)."""
    x0, u, x = scattered_clipped(B, N)
    A, Bm = host_jacobians(B, N)
    c = sc.adjoint(x0, u, x, dc.DT, case.Q, case.R, case.QN, -case.U_MAX, case.U_MAX, A=A, B=Bm)
    ld = recursion(A, Bm, x, u, case.Q, case.R, case.QN, LD)
    scale = nu_scale(ld["nu"])
    err = scaled_errors(dict(nu=c.nu, primer=c.primer, grad=c.grad, dJdx0=c.dJdx0), ld, scale)
    stat_ld = sc.stationarity(ld["grad"].astype(np.float64), u, -case.U_MAX, case.U_MAX)[0]
    err["stat"] = float((np.abs(c.stat - stat_ld) / scale).max())
    return err


# fp64_vs_ld(B, N) per output as tests/test_scvx_adjoint_host.py printed it (rounded up to two digits; that test keeps the table
# current: each entry bounds today's value and is at most twice it).  The GPU test allows dc.GPU_MARGIN times as much: the kernel
# differs from NumPy's einsum by the order of its fma chains, which is of the order of NumPy's own rounding.  stat is a maximum of
# entries of grad, so it inherits grad's bound (its own difference may be 0 where the maximum sits on a well-rounded entry)
FP64_VS_LD = {
    (1, 1): dict(nu=3.6e-17, primer=4.5e-19, grad=4.5e-19, dJdx0=3.1e-17),
    (63, 7): dict(nu=5.3e-16, primer=1.9e-17, grad=1.9e-17, dJdx0=5.6e-16),
    (65, 64): dict(nu=8.2e-15, primer=3.7e-16, grad=3.7e-16, dJdx0=8.4e-15),
    (130, 65): dict(nu=1.2e-14, primer=5.0e-16, grad=5.0e-16, dJdx0=1.2e-14),
}


def linearisation_bound(A, Bm, nu, eps=LIN_BOUND):
    """First-order bound on what entrywise errors of at most eps in A and B do to nu, primer (= grad = stat) and dJdx0, in long
    double, normalised by max |nu| per trajectory.  An error d_l of A_l (l = k+1 .. N-1, array indices: nu[k] = A[k+1]' nu[k+1] - qx[k])
    reaches nu[k] as M_kl d_l' nu[l] with M_kl = A[k+1]' .. A[l-1]' (the true products, so that their cancellation is kept; the
    product of the |A_l| grows like 1e5 over 64 stages), and |d_l' nu[l]| <= eps |nu[l]|_1 per entry:
        e[k] = eps sum_l rowsum|M_kl| |nu[l]|_1,    primer: |B_k|' e[k] + eps |nu[k]|_1,    dJdx0: |A_0|' e[0] + eps |nu[0]|_1."""
    A, Bm, nu, eps = np.asarray(A, LD), np.asarray(Bm, LD), np.abs(np.asarray(nu, LD)), LD(eps)
    Bn, N = nu.shape[:2]
    s1 = nu.sum(axis=2)                                # (B, N): |nu[l]|_1
    e = np.zeros((Bn, N, 6), LD)
    M = np.zeros((Bn, N, 6, 6), LD)                    # M[:, l] = M_kl for the current k, l > k
    for k in range(N - 2, -1, -1):
        M[:, k + 2:] = np.einsum("bji,bljm->blim", A[:, k + 1], M[:, k + 2:])
        M[:, k + 1] = np.eye(6, dtype=LD)
        e[:, k] = eps * np.einsum("blij,bl->bi", np.abs(M[:, k + 1:]), s1[:, k + 1:])
    pe = np.einsum("bkij,bki->bkj", np.abs(Bm), e) + eps * s1[:, :, None]
    e0 = np.einsum("bji,bj->bi", np.abs(A[:, 0]), e[:, 0]) + eps * s1[:, 0, None]
    scale = nu.max(axis=(1, 2))
    worst = lambda a: float((a.reshape(Bn, -1).max(axis=1) / scale).max())      # noqa: E731
    return dict(nu=worst(e), primer=worst(pe), grad=worst(pe), dJdx0=worst(e0), stat=worst(pe))
