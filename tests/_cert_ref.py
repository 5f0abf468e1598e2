"""Reference of the on-device certificate for the tests: the four definitions as a plain sequential fp64
recursion with a single segment, in NumPy.

With g = P z + q + rho y, P = blkdiag(R, Q, ..., R, QN) in block order (u_k, x_{k+1}):
  nu        nu_N = -g^x_N,  nu_k = A_k' nu_{k+1} - g^x_k  (k = N-1 .. 1); nu[:, k] holds nu_{k+1}, the multiplier of stage k's row
  stat      max_k |g^u_k - B_k' nu_{k+1}|_inf
  feas_dyn  max_k |x_{k+1} - A_k x_k - B_k u_k|_inf
  obj       1/2 z'Pz + q'z + sum_k f_k ||z_u,k||_2,   and  obj_abs = the sum of the absolute values of its terms (tolerance scale)
"""
import numpy as np

from _indep import hessian_diag_blocks, stage_dynamics


def expand_fuel(fuel, N):
    if fuel is None:
        return np.zeros(N)
    return np.broadcast_to(np.asarray(fuel, np.float64), (N,)).copy()


def gradient(p, z, y, rho):
    """g = P z + q + rho y as (batch, N, nb); weights symmetrised as admm_setup does."""
    Bt, N, nb = p.batch, p.N, p.nb
    Pd = hessian_diag_blocks(p)
    Pd = 0.5 * (Pd + Pd.transpose(0, 2, 1))
    Z = np.asarray(z, np.float64).reshape(Bt, N, nb)
    g = np.einsum("kij,bkj->bki", Pd, Z) + rho * np.asarray(y, np.float64).reshape(Bt, N, nb)
    if p.q is not None:
        g = g + np.asarray(p.q, np.float64).reshape(Bt, N, nb)
    return g


def certificate(p, z, y, rho, fuel="problem"):
    """dict(obj, obj_abs, feas_dyn, stat: (batch,); nu: (batch, N, n)) at (z, mu = rho y)."""
    Bt, N, n, m, nb = p.batch, p.N, p.n, p.m, p.nb
    A, B = stage_dynamics(p)
    Z = np.asarray(z, np.float64).reshape(Bt, N, nb)
    g = gradient(p, z, y, rho)
    nu = np.zeros((Bt, N, n))
    c = np.zeros((Bt, n))
    for k in range(N - 1, -1, -1):
        nu[:, k] = c - g[:, k, m:]
        c = nu[:, k] @ A[k]                       # rows: A_k' nu_{k+1}
    stat = np.abs(g[:, :, :m] - np.einsum("kij,bki->bkj", B, nu)).reshape(Bt, -1).max(axis=1)
    u, x = Z[:, :, :m], Z[:, :, m:]
    xprev = np.concatenate([np.atleast_2d(p.x0)[:, None, :], x[:, :-1]], axis=1)
    defect = x - np.einsum("kij,bkj->bki", A, xprev) - np.einsum("kij,bkj->bki", B, u)
    feas_dyn = np.abs(defect).reshape(Bt, -1).max(axis=1)
    Pd = hessian_diag_blocks(p)
    Pd = 0.5 * (Pd + Pd.transpose(0, 2, 1))
    fu = expand_fuel(getattr(p, "fuel", None) if isinstance(fuel, str) else fuel, N)
    quad = 0.5 * Z[:, :, :, None] * Pd[None] * Z[:, :, None, :]                 # every product of z'Pz / 2
    lin = np.zeros_like(Z) if p.q is None else np.asarray(p.q, np.float64).reshape(Bt, N, nb) * Z
    fl = fu[None] * np.sqrt(np.sum(u * u, axis=2))
    obj = quad.reshape(Bt, -1).sum(axis=1) + lin.reshape(Bt, -1).sum(axis=1) + fl.sum(axis=1)
    obj_abs = np.abs(quad).reshape(Bt, -1).sum(axis=1) + np.abs(lin).reshape(Bt, -1).sum(axis=1) + fl.sum(axis=1)
    return dict(obj=obj, obj_abs=obj_abs, feas_dyn=feas_dyn, stat=stat, nu=nu)
