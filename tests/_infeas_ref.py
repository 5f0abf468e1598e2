"""Reference of the on-device infeasibility probe for the tests: the table of §2.10 as a plain sequential fp64
recursion with a single segment, in NumPy, and a dense restatement of the Farkas inequality that shares nothing with it.  With dtype=np.longdouble
the table is evaluated in extended precision (every operand converted first): the measure of the rounding error of the fp64 form and
of the kernels.

With lambda = (y_after - y_before) / span in block order (u_k, x_{k+1}):
  nu      nu_N = -lambda^x_N,  nu_k = A_k' nu_{k+1} - lambda^x_k  (k = N-1 .. 1); nu[:, k] holds nu_{k+1}, the multiplier of stage k's row
  mu      state rows lambda^x, control rows B_k' nu_{k+1}  (= -G' nu)
  drift   |lambda|_inf;   defect  |mu - lambda|_inf / |mu|_inf
  sigma   the support function of C at mu: hi mu (mu > 0), lo mu (mu < 0) per box row -- a row whose needed bound is infinite adds
          nothing and |mu| enters `open` --, unorm_k ||mu^u_k||_2 for the control rows of a stage with a finite thrust bound
  sep     (x0' A_0' nu_1 + sigma) / |mu|_inf  if |mu|_inf > 0 and open <= eps |mu|_inf, else +inf;   infeasible = sep < -eps
  sep_abs the sum of the absolute values of sep's terms over |mu|_inf (tolerance scale of a comparison in another summation order)
"""
import numpy as np

from _indep import stage_bounds, stage_dynamics


def stage_unorm(p):
    if p.unorm is None:
        return np.full(p.N, np.inf)
    return np.broadcast_to(np.asarray(p.unorm, np.float64), (p.N,)).copy()


def probe(p, y_before, y_after, span, eps, dtype=np.float64):
    """dict(sep, drift, defect, sep_abs, mu_max, open: (batch,); infeasible: (batch,) int32; nu: (batch, N, n)), as arrays of `dtype`;
    open is the largest |mu_i| over the rows whose needed bound is infinite, the left side of the ray test open <= eps |mu|_inf.

    dtype=np.longdouble: the same table with every operand (the fp64 data of the problem, both y, span, eps) converted first and
    every operation in extended precision -- what a faithful evaluation is measured against."""
    Bt, N, n, m, nb = p.batch, p.N, p.n, p.m, p.nb
    A, B = (np.asarray(a, dtype) for a in stage_dynamics(p))
    lo, hi = (np.asarray(a, dtype) for a in stage_bounds(p))
    un = stage_unorm(p).astype(dtype)
    eps = dtype(eps)
    lam = ((np.asarray(y_after, dtype) - np.asarray(y_before, dtype)) / dtype(span)).reshape(Bt, N, nb)
    nu = np.zeros((Bt, N, n), dtype)
    mu = lam.copy()
    sig = np.zeros(Bt, dtype)
    sig_abs = np.zeros(Bt, dtype)
    opn = np.zeros(Bt, dtype)
    c = np.zeros((Bt, n), dtype)
    zero, one, inf = dtype(0.0), dtype(1.0), dtype(np.inf)

    def box_row(v, l, h):
        nonlocal sig, sig_abs, opn
        b = np.where(v > zero, h, l)
        fin = np.isfinite(b)
        t = np.where(fin, b, zero) * v
        sig = sig + t
        sig_abs = sig_abs + np.abs(t)
        opn = np.maximum(opn, np.where(fin, zero, np.abs(v)))

    for k in range(N - 1, -1, -1):
        nu[:, k] = c - lam[:, k, m:]
        mu[:, k, :m] = nu[:, k] @ B[k]                # rows: B_k' nu_{k+1}
        for i in range(n):
            box_row(mu[:, k, m + i], lo[k, m + i], hi[k, m + i])
        if np.isfinite(un[k]):
            t = un[k] * np.sqrt(np.sum(mu[:, k, :m] ** 2, axis=1))
            sig = sig + t
            sig_abs = sig_abs + t
        else:
            for j in range(m):
                box_row(mu[:, k, j], lo[k, j], hi[k, j])
        c = nu[:, k] @ A[k]                           # rows: A_k' nu_{k+1}
    terms = np.atleast_2d(np.asarray(p.x0, dtype)) * c    # h' nu = x0' (A_0' nu_1)
    sig = sig + terms.sum(axis=1)
    sig_abs = sig_abs + np.abs(terms).sum(axis=1)
    mu_max = np.abs(mu).reshape(Bt, -1).max(axis=1)
    d_max = np.abs(mu - lam).reshape(Bt, -1).max(axis=1)
    drift = np.abs(lam).reshape(Bt, -1).max(axis=1)
    ray = (mu_max > zero) & (opn <= eps * mu_max)
    safe = np.where(mu_max > zero, mu_max, one)
    sep = np.where(ray, sig / safe, inf)
    defect = np.where(mu_max > zero, d_max / safe, np.where(d_max > zero, inf, zero))
    return dict(sep=sep, drift=drift, defect=defect, infeasible=(sep < -eps).astype(np.int32), nu=nu,
                sep_abs=np.where(ray, sig_abs / safe, zero), mu_max=mu_max, open=opn)


def check(ref, r, eps, tol=1e-10, flags_exact=False, defect_on=None):
    """All outputs of a device probe `r` (sep, drift, defect, infeasible, nu or None) against probe()'s `ref`, on the scales of the
    file header of tests/test_gpu_infeas.py: +inf must match as +inf; a flag may differ from the reference's only where sep sits
    within the comparison's tolerance of -eps (flags_exact: nowhere).  defect_on: the QPs on which defect is compared (all: where mu and
    lambda are rounding errors of a stationary y, their quotient is one too).  -> {output: worst error / tolerance}."""
    on = np.ones(ref["sep"].shape[0], bool) if defect_on is None else np.asarray(defect_on, bool)
    batch = ref["sep"].shape[0]
    s_nu = np.maximum(1.0, np.abs(ref["nu"]).reshape(batch, -1).max(axis=1))
    for name, got in (("sep", r.sep), ("defect", r.defect)):
        d = np.flatnonzero((np.isinf(got) != np.isinf(ref[name])) & (on | (name == "sep")))
        assert d.size == 0, (name + ": +inf on other QPs than the reference's", d, got[d], ref[name][d], "mu_max", ref["mu_max"][d],
                             "drift", r.drift[d], ref["drift"][d])
    assert np.all(r.sep[np.isinf(r.sep)] > 0)
    fs, fd = np.isfinite(ref["sep"]), np.isfinite(ref["defect"]) & on
    ratio_mu = np.where(ref["mu_max"] > 0, s_nu / np.where(ref["mu_max"] > 0, ref["mu_max"], 1.0), 1.0)
    ratios = {"sep": (np.abs(r.sep - ref["sep"])[fs] / (tol * np.maximum(1.0, ref["sep_abs"])[fs])).max(initial=0.0),
              "drift": (np.abs(r.drift - ref["drift"]) / (tol * np.maximum(1.0, ref["drift"]))).max(),
              "defect": (np.abs(r.defect - ref["defect"])[fd] /
                         (tol * np.maximum(np.maximum(1.0, ref["defect"]), ratio_mu))[fd]).max(initial=0.0)}
    if r.nu is not None:
        ratios["nu"] = (np.abs(r.nu - ref["nu"]).reshape(batch, -1).max(axis=1) / (tol * s_nu)).max()
    print("error / tolerance:", {k: float(f"{v:.3g}") for k, v in ratios.items()}, "finite sep:", int(fs.sum()), "of", batch,
          "flags:", int(ref["infeasible"].sum()))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
    near = fs & (np.abs(ref["sep"] + eps) <= tol * np.maximum(1.0, ref["sep_abs"]))
    if flags_exact:
        assert not near.any(), ("a sep within the tolerance of -eps", ref["sep"][near])
    assert r.infeasible.dtype == np.int32 and np.array_equal(r.infeasible[~near], ref["infeasible"][~near])
    return ratios


def dense_farkas(p, b, nu, open_tol=0.0):
    """h' nu + sigma_C(-G' nu) of QP b for the costates nu ((N, n): nu_1 .. nu_N), from the dense G, h of oracle/admm_ref.dense_qp,
    row by row; normalised by |G' nu|_inf like sep.  +inf if a row that needs an infinite bound has |mu_i| > open_tol |mu|_inf.
    Negative: no w has G w = h and w in C."""
    import admm_ref
    N, m, nb = p.N, p.m, p.nb
    _, _, G, h = admm_ref.dense_qp(p.A, p.B, p.Q, p.R, p.QN, p.x0[b], N)
    v = np.asarray(nu, np.float64).reshape(-1)
    mu = -(G.T @ v)
    lo, hi = stage_bounds(p)
    lo, hi = lo.reshape(-1), hi.reshape(-1)
    un = stage_unorm(p)
    mu_max = np.abs(mu).max()
    if not mu_max > 0.0:
        return np.inf
    total = float(h @ v)
    for i in range(N * nb):
        k, r = divmod(i, nb)
        if r < m and np.isfinite(un[k]):
            if r == 0:
                total += un[k] * np.linalg.norm(mu[i:i + m])
            continue
        if mu[i] == 0.0:
            continue
        bound = hi[i] if mu[i] > 0.0 else lo[i]
        if not np.isfinite(bound):
            if abs(mu[i]) > open_tol * mu_max:
                return np.inf
            continue
        total += bound * mu[i]
    return total / mu_max
