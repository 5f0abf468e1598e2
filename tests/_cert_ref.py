"""Reference of the on-device certificate for the tests: the four definitions as a plain sequential fp64
recursion with a single segment, in NumPy -- and, with dtype=np.longdouble, the same definitions in extended precision (every operand
converted first), against which the rounding error of both the fp64 form and the kernels is measured.

With g = P z + q + rho y, P = blkdiag(R, Q, ..., R, QN) in block order (u_k, x_{k+1}):
  nu        nu_N = -g^x_N,  nu_k = A_k' nu_{k+1} - g^x_k  (k = N-1 .. 1); nu[:, k] holds nu_{k+1}, the multiplier of stage k's row
  stat      max_k |g^u_k - B_k' nu_{k+1}|_inf
  feas_dyn  max_k |x_{k+1} - A_k x_k - B_k u_k|_inf
  obj       1/2 z'Pz + q'z + sum_k f_k ||z_u,k||_2,   and  obj_abs = the sum of the absolute values of its terms (tolerance scale)
"""
import numpy as np

from _indep import hessian_diag_blocks, stage_dynamics


def expand_fuel(fuel, N, dtype=np.float64):
    if fuel is None:
        return np.zeros(N, dtype)
    return np.broadcast_to(np.asarray(fuel, np.float64), (N,)).astype(dtype)


def _weights(p, dtype):
    """The diagonal blocks of P the device holds: symmetrised in fp64 as admm_setup does, THEN converted."""
    Pd = hessian_diag_blocks(p)
    return (0.5 * (Pd + Pd.transpose(0, 2, 1))).astype(dtype)


def gradient(p, z, y, rho, dtype=np.float64):
    """g = P z + q + rho y as (batch, N, nb); weights symmetrised as admm_setup does."""
    Bt, N, nb = p.batch, p.N, p.nb
    Pd = _weights(p, dtype)
    Z = np.asarray(z, dtype).reshape(Bt, N, nb)
    g = np.einsum("kij,bkj->bki", Pd, Z) + dtype(rho) * np.asarray(y, dtype).reshape(Bt, N, nb)
    if p.q is not None:
        g = g + np.asarray(p.q, dtype).reshape(Bt, N, nb)
    return g


def certificate(p, z, y, rho, fuel="problem", dtype=np.float64):
    """dict(obj, obj_abs, feas_dyn, stat: (batch,); nu: (batch, N, n)) at (z, mu = rho y), as arrays of `dtype`.

    dtype=np.longdouble: the same definitions with every operand (the fp64 data of the problem, z, y, rho, the weights) converted
    first and every operation in extended precision -- what a faithful evaluation is measured against."""
    Bt, N, n, m, nb = p.batch, p.N, p.n, p.m, p.nb
    A, B = (np.asarray(a, dtype) for a in stage_dynamics(p))
    Z = np.asarray(z, dtype).reshape(Bt, N, nb)
    g = gradient(p, z, y, rho, dtype)
    nu = np.zeros((Bt, N, n), dtype)
    c = np.zeros((Bt, n), dtype)
    for k in range(N - 1, -1, -1):
        nu[:, k] = c - g[:, k, m:]
        c = nu[:, k] @ A[k]                       # rows: A_k' nu_{k+1}
    stat = np.abs(g[:, :, :m] - np.einsum("kij,bki->bkj", B, nu)).reshape(Bt, -1).max(axis=1)
    u, x = Z[:, :, :m], Z[:, :, m:]
    xprev = np.concatenate([np.broadcast_to(np.atleast_2d(np.asarray(p.x0, dtype)), (Bt, n))[:, None, :], x[:, :-1]], axis=1)
    defect = x - np.einsum("kij,bkj->bki", A, xprev) - np.einsum("kij,bkj->bki", B, u)
    feas_dyn = np.abs(defect).reshape(Bt, -1).max(axis=1)
    Pd = _weights(p, dtype)
    fu = expand_fuel(getattr(p, "fuel", None) if isinstance(fuel, str) else fuel, N, dtype)
    quad = dtype(0.5) * Z[:, :, :, None] * Pd[None] * Z[:, :, None, :]          # every product of z'Pz / 2
    lin = np.zeros_like(Z) if p.q is None else np.asarray(p.q, dtype).reshape(Bt, N, nb) * Z
    fl = fu[None] * np.sqrt(np.sum(u * u, axis=2))
    obj = quad.reshape(Bt, -1).sum(axis=1) + lin.reshape(Bt, -1).sum(axis=1) + fl.sum(axis=1)
    obj_abs = np.abs(quad).reshape(Bt, -1).sum(axis=1) + np.abs(lin).reshape(Bt, -1).sum(axis=1) + fl.sum(axis=1)
    return dict(obj=obj, obj_abs=obj_abs, feas_dyn=feas_dyn, stat=stat, nu=nu)
