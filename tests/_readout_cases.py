"""The problems of the pair x chunk-edge sweeps of the read-out kernels (tests/_shapes.py: chunk_edge), shared by the GPU sweeps
(tests/test_gpu_cert.py, tests/test_gpu_infeas.py) and the host checks of their inputs (tests/test_readout_refs_host.py), and the
two-sided comparison both sweeps make: the project's tolerance, and a rounding-level bound against an extended-precision reference.

  refill  random_ltv(with_q=True, thrust_norm=True); for the certificate with per-stage fuel weights (stage_fuel)
  fit     box only, no q, made LTI with one shared box (lti): time_varying = 0, stage_bounds = 0 -- the host expands both to N stages
  stage   random_ltv(with_q=True)
For the infeasibility probe the state box is shrunk to 0.3 of itself (as in test_gpu_infeas.py::test_matches_reference: as drawn
it is never active within 25 iterations and the comparison would be one of zeros)."""
import dataclasses

import numpy as np

import admm_library_amd as pkg
from _shapes import chunk_edge

RHO = 0.3
CERT_ITERS = 8                      # run(8), then the certificate
PROBE_ITERS, PROBE_SPAN = 20, 5     # run(20), then two probes of span 5
PROBE_EPS = (1e-6, 1e3)
EPS64 = 2.0 ** -52
# Seeds: 3000 + 16 n + m, or the first + 100 j that meets the conditions tests/test_readout_refs_host.py keeps on the inputs:
#   growth      max_k max |A_{N-1} ... A_k| <= GROWTH_MAX, the conditioning bound admm_setup applies to automatic segment counts
#               (include/admm_hip.h).  The costate recursion nu_k = A_k' nu_{k+1} - g_k amplifies a rounding error by that product,
#               and the `fit` problems repeat ONE random A = I + 0.15 G / sqrt(n) for up to 129 stages: as drawn most are unstable
#               (growth 1e3 .. 1e13) and NO fp64 evaluation of section 2.9 holds 1e-10 there -- the fp64 NumPy reference misses the
#               longdouble one by up to 3.5e-11 x scale -- for reasons that are no kernel's fault
#   dual drift  mu_max > 0 in at least DRIFT_FLOOR QPs of both probes on the oracle's iterates
# `refill` needs no other seed; `stage` one ((4, 4): y has not moved on any state row of its 3 QPs).
GROWTH_MAX = 100.0
DRIFT_FLOOR = {"refill": 30, "fit": 30, "stage": 1}          # of 70, 261 and 3 QPs
SEEDS = {((1, 1), "fit"): 3117, ((2, 1), "fit"): 3533, ((3, 1), "fit"): 3149, ((3, 2), "fit"): 3150, ((3, 3), "fit"): 3251,
         ((4, 1), "fit"): 3365, ((4, 2), "fit"): 3466, ((4, 3), "fit"): 3267, ((4, 4), "stage"): 3168, ((5, 1), "fit"): 5081,
         ((5, 2), "fit"): 4382, ((5, 3), "fit"): 5783, ((6, 1), "fit"): 3297, ((6, 2), "fit"): 3698, ((6, 3), "fit"): 3299,
         ((6, 4), "fit"): 5400, ((7, 2), "fit"): 6014, ((7, 3), "fit"): 3815, ((8, 2), "fit"): 9530, ((8, 3), "fit"): 12731,
         ((8, 4), "fit"): 8332, ((9, 3), "fit"): 7947, ((10, 2), "fit"): 3262, ((10, 4), "fit"): 4264, ((12, 4), "fit"): 3296}


def lti(p):
    """The stage-1 dynamics, box and thrust bound of a random_ltv problem at every stage: time_varying = 0, stage_bounds = 0."""
    return dataclasses.replace(p, A=p.A[1].copy(), B=p.B[1].copy(), lo=p.lo[1].copy(), hi=p.hi[1].copy(),
                               unorm=None if p.unorm is None else np.float64(p.unorm[1]))


def stage_fuel(p):
    """Per-stage weights on a thrust_norm random_ltv problem: positive where the control rows are unbounded."""
    return dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), 0.3, 0.0))


def seed_of(pair, case):
    return SEEDS.get((pair, case), 3000 + 16 * pair[0] + pair[1])


def problem(pair, case, probe):
    """(problem, segments) of a sweep cell; probe: the infeasibility sweep's form (else the certificate's)."""
    n, m = pair
    N, S, batch = chunk_edge(n, m, case)
    seed = seed_of(pair, case)
    if case == "refill":
        p = pkg.random_ltv(N, n, m, batch, seed=seed, with_q=True, thrust_norm=True)
        if not probe:
            p = stage_fuel(p)
    elif case == "fit":
        p = lti(pkg.random_ltv(N, n, m, batch, seed=seed, with_q=False))
    else:
        p = pkg.random_ltv(N, n, m, batch, seed=seed, with_q=True)
    if probe:
        p.lo[..., m:] *= 0.3
        p.hi[..., m:] *= 0.3
    return p, S


def growth(p):
    """max_k max |A_{N-1} ... A_k|: what the costate recursion multiplies an error made at stage N - 1 by on its way to stage k."""
    A = np.broadcast_to(p.A, (p.N,) + p.A.shape[-2:])
    P, g = np.eye(p.n), 1.0
    for k in range(p.N - 1, -1, -1):
        P = P @ A[k]
        g = max(g, float(np.abs(P).max()))
    return g


def worst(err, scale):
    """max over the batch of err / scale, as a float (err: (batch,) or (batch, ...), of any float type)."""
    err = np.asarray(err)
    per_qp = err.reshape(err.shape[0], -1).max(axis=1, initial=0.0) if err.size else np.zeros(0)
    return float((per_qp / scale).max(initial=0.0))


def two_sided(name, e_dev, e_np, tol, M):
    """The two assertions of a sweep on one output, both on the scale of its _compare: the project's tolerance, and a
    rounding-level bound -- the device's worst error against the extended-precision reference is at most M times what the fp64
    NumPy evaluation of the same definitions achieves (never less than one ulp of the scale)."""
    ratio = e_dev / max(e_np, EPS64)
    assert e_dev <= tol, (name, e_dev)
    assert ratio <= M, (name, "device", e_dev, "fp64 NumPy", e_np, "ratio", ratio, "M", M)
    return ratio


LD = np.longdouble


def _get(r, name):
    return r[name] if isinstance(r, dict) else getattr(r, name)


def cert_errors(p, z, got, ld):
    """Worst error over the batch of the four outputs of a certificate (`got`: a Certificate or a reference's dict) against the
    extended-precision reference `ld`, on the scales of test_gpu_cert._compare taken from `ld`."""
    b = p.batch
    s_nu = np.maximum(1.0, np.abs(ld["nu"]).reshape(b, -1).max(axis=1))
    s_obj = np.maximum(1.0, ld["obj_abs"])
    s_z = np.maximum(1.0, np.abs(np.asarray(z, LD)).reshape(b, -1).max(axis=1))
    d = lambda k: np.abs(np.asarray(_get(got, k), LD) - ld[k])
    return {"nu": worst(d("nu"), s_nu), "stat": worst(d("stat"), s_nu), "obj": worst(d("obj"), s_obj),
            "feas_dyn": worst(d("feas_dyn"), s_z)}


def probe_errors(p, got, ld):
    """The same for the four real outputs of a probe, on the scales of test_gpu_infeas._compare taken from `ld`; sep and defect
    where both sides are finite (that +inf matches as +inf is asserted apart)."""
    b = p.batch
    s_nu = np.maximum(1.0, np.abs(ld["nu"]).reshape(b, -1).max(axis=1))
    pos = ld["mu_max"] > 0
    ratio_mu = np.where(pos, s_nu / np.where(pos, ld["mu_max"], 1.0), 1.0)
    def d(k):
        with np.errstate(invalid="ignore"):          # (inf - inf where both sides are +inf: masked below)
            return np.abs(np.asarray(_get(got, k), LD) - ld[k])

    fs = np.isfinite(ld["sep"]) & np.isfinite(np.asarray(_get(got, "sep"), LD))
    fd = np.isfinite(ld["defect"]) & np.isfinite(np.asarray(_get(got, "defect"), LD))
    s_sep = np.maximum(1.0, ld["sep_abs"])
    s_def = np.maximum(np.maximum(1.0, np.where(fd, ld["defect"], 0.0)), ratio_mu)
    return {"nu": worst(d("nu"), s_nu), "sep": worst(np.where(fs, d("sep"), 0.0), s_sep),
            "drift": worst(d("drift"), np.maximum(1.0, ld["drift"])), "defect": worst(np.where(fd, d("defect"), 0.0), s_def)}
