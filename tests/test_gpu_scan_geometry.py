"""The segment scan's geometry against the C oracle (tests/_shapes.py SCAN_GEOMETRIES).

The scan GEMM (xscan_mfma_kernel) is the one kernel whose shape is no template parameter: row groups, padded M and K, the
k-step range of every group, the number of double-buffer rounds and the split-K factor follow from S n, the batch and the CU
count.  The (n, m) sweeps of tests/test_gpu_shapes.py hold S = 4; this module sweeps S, the width n, the pitch and -- forced
through ADMM_SCAN_SPLIT, and checked through Solver.scan_geometry() so that a split that was not applied fails -- every
split-K factor against every consumer of the scan's output slabs.  The per-QP scans of per-instance dynamics get the segment
counts they never ran with: one-stage segments, N % S != 0 at the wide pairs, 64 segments of a short horizon.
Every case: 1e-10 relative to max(1, |oracle|_inf) on w, z, y (and on r, s where the last residual iteration is compared);
the forward-elimination fallback warning is an error, as in tests/test_gpu_shapes.py.  PARITY UNPINNED."""
import numpy as np
import pytest

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd import _abi
from _shapes import (MFMA, SCAN_EMPTY_SLICE, SCAN_GEOMETRIES, SCAN_REFACTOR_RHO, SCAN_REFACTOR_SEED, SCAN_SLICEABLE, gid,
                     scan_shape)
from _sweep import SCHEDULE_ITERATIONS, TOL, close, schedule

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]
INVALID = {v: k for k, v in _abi.STATUS_NAMES.items()}["ADMM_ERR_INVALID"]
NO_MFMA, PLAIN, UNFUSED = _abi.FLAG_NO_MFMA, _abi.FLAG_NO_MFMA | _abi.FLAG_NO_ALTERNATE, _abi.FLAG_UNFUSED
LAST_RESIDUAL = SCHEDULE_ITERATIONS - 1      # the schedule ends with run(7, residual_every=2): its last residuals are iteration 38's

_REFS = {}


def _problem(geom, batch, **kw):
    n, m, N, S, seed, rho = geom
    return pkg.random_ltv(N=N, n=n, m=m, batch=batch, seed=seed, **kw)


def _state(p, seed):
    rng = np.random.default_rng(seed)
    return 0.1 * rng.standard_normal((p.batch, p.L)), 0.1 * rng.standard_normal((p.batch, p.L))


def _reference(key, p, rho, alpha, z0, y0, iters=SCHEDULE_ITERATIONS, resid_at=LAST_RESIDUAL):
    """Oracle iterates after `iters` iterations and the residuals of iteration resid_at, computed once per key and shared."""
    if key not in _REFS:
        ref = oc.solve(p, rho=rho, alpha=alpha, max_iter=iters, stop=False, z0=z0, y0=y0)
        res = oc.solve(p, rho=rho, alpha=alpha, max_iter=resid_at, check_interval=resid_at, stop=False, z0=z0, y0=y0)
        _REFS[key] = dict(w=ref["w"], z=ref["z"], y=ref["y"], r=res["r"], s=res["s"])
        for a in _REFS[key].values():
            a.setflags(write=False)
    return _REFS[key]


def _residuals_close(s, ref):
    r, sd = s.residuals()[:2]
    return all(np.abs(a - b).max() <= TOL * max(1.0, np.abs(b).max()) for a, b in ((r, ref["r"]), (sd, ref["s"])))


MI355X_CUS = 256            # the compute units admm_setup sizes its grids for


def _automatic_split(pitch, groups, K, cus):
    """admm_setup's rule, restated: aim at one workgroup per CU, at most 8 slices, at least two batches of 8 k-steps per slice."""
    sp = 1
    while sp < 8 and (pitch // 64) * groups * sp < cus:
        sp *= 2
    while sp > 1 and (K // 4) // sp < 16:
        sp //= 2
    return sp


# ---- every geometry at the automatic split, pitch 64 and 128 ----
@pytest.mark.parametrize("batch", [5, 67], ids=["pitch64", "pitch128"])
@pytest.mark.parametrize("geom", SCAN_GEOMETRIES, ids=gid)
def test_every_geometry_at_the_automatic_split(gpu, geom, batch, monkeypatch):
    """The alternating one-lane kernels and the plain fused ones (the scans of WB and of W) on the GEMM scan."""
    monkeypatch.delenv("ADMM_SCAN_SPLIT", raising=False)
    n, m, N, S, seed, rho = geom
    Se, M, K, groups = scan_shape(n, N, S)
    p = _problem(geom, batch)
    z0, y0 = _state(p, batch + n)
    ref = _reference(("auto", geom, batch), p, rho, 1.0, z0, y0)
    split = _automatic_split((batch + 63) // 64 * 64, groups, K, MI355X_CUS)
    for flags, alternating in ((NO_MFMA, True), (PLAIN, False)):
        with pkg.Solver(p, pkg.Options(rho=rho, segments=S, flags=flags)) as s:
            path = s.path()
            assert (path["segments"], path["alternating"], path["scan_form"], path["kernel_family"]) == \
                (Se, alternating, "mfma_gemm", "one_lane_fp64"), (flags, path)
            assert s.scan_geometry() == {"split": split, "M": M, "K": K, "groups": groups}, (flags, s.scan_geometry())
            got = schedule(s, z0, y0, first_residuals=batch == 5)
            assert _residuals_close(s, ref), flags
        assert close(got, ref), flags


# ---- the matrix-vector scan of batches of up to 4 QPs ----
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("geom", SCAN_GEOMETRIES, ids=gid)
def test_every_geometry_on_the_matrix_vector_scan(gpu, geom, batch, monkeypatch):
    """xscan_gemv_kernel writes whole sums: a forced split must not reach it (the consumers would add slabs nobody wrote)."""
    monkeypatch.setenv("ADMM_SCAN_SPLIT", "8")
    n, m, N, S, seed, rho = geom
    Se, M, K, groups = scan_shape(n, N, S)
    p = _problem(geom, batch, with_q=False)
    z0, y0 = _state(p, batch + n)
    ref = _reference(("gemv", geom, batch), p, rho, 1.0, z0, y0)
    for flags in (NO_MFMA,) + ((0,) if (n, m) in MFMA else ()):       # (the default family of these batches at an MFMA pair: fp64 MFMA)
        with pkg.Solver(p, pkg.Options(rho=rho, segments=S, flags=flags)) as s:
            path = s.path()
            assert (path["segments"], path["alternating"], path["scan_form"]) == (Se, True, "matrix_vector"), (flags, path)
            assert path["kernel_family"] == ("one_lane_fp64" if flags else "mfma_fp64"), (flags, path)
            assert s.scan_geometry() == {"split": 1, "M": M, "K": K, "groups": groups}, (flags, s.scan_geometry())
            got = schedule(s, z0, y0, first_residuals=batch == 1)
            assert _residuals_close(s, ref), flags
        assert close(got, ref), flags


# ---- forced split x consumer ----
# name -> (problem keywords, option keywords, tolerance, what path() must say)
CONSUMERS = {
    "alternating": (dict(with_q=False), dict(flags=NO_MFMA), TOL, dict(alternating=True, kernel_family="one_lane_fp64")),
    "plain_fused": (dict(with_q=False), dict(flags=PLAIN), TOL, dict(alternating=False, kernel_family="one_lane_fp64")),
    "unfused": (dict(with_q=False), dict(flags=UNFUSED), TOL, dict(alternating=False, kernel_family="one_lane_fp64")),
    "state_rows_unbounded": (dict(with_q=False, state_bounds=False), dict(flags=NO_MFMA), TOL,     # XFREE and lean-residual forms
                             dict(alternating=True, xfree=True, kernel_family="one_lane_fp64")),
    "q_and_thrust_bound": (dict(with_q=True, thrust_norm=True), dict(flags=NO_MFMA), TOL, dict(alternating=True)),
    "q_and_thrust_bound_plain": (dict(with_q=True, thrust_norm=True), dict(flags=PLAIN), TOL, dict(alternating=False)),
    "relaxed": (dict(with_q=False), dict(flags=NO_MFMA, alpha=1.6), TOL, dict(alternating=True)),
    "relaxed_plain": (dict(with_q=True), dict(flags=PLAIN, alpha=1.6), TOL, dict(alternating=False)),
    "mfma_fp64": (dict(with_q=False), dict(precision_mode=_abi.PRECISION_FP64_MFMA), TOL, dict(alternating=True, kernel_family="mfma_fp64")),
    "mfma_mixed": (dict(with_q=False), dict(precision_mode=_abi.PRECISION_MIXED), 1e-5, dict(kernel_family="mfma_mixed")),
    "step_x_read_out": (dict(with_q=True), dict(flags=NO_MFMA), TOL, dict(alternating=True)),
}
SPLITS = (1, 2, 4, 8)
SPLIT_BATCH = 67            # pitch 128: two column blocks of the GEMM grid, a second wave with clamped lanes in the consumers
AGREE = 1e-13               # splits differ by the association of one sum per scan row (cf. test_rows_factorisation_agrees_...)
# every consumer meets every split at every sliceable and every empty-slice entry (the MFMA forms at the MFMA pairs among them):
# the whole module runs in well under a minute on an MI355X, so the consumer x geometry product is not thinned
SPLIT_CASES = [(g, c) for g in SCAN_SLICEABLE + SCAN_EMPTY_SLICE for c in CONSUMERS if not c.startswith("mfma") or g[:2] in MFMA]


@pytest.fixture(scope="module")
def consumer_runs():
    """(geometry, consumer, split) -> what that handle returned: every split > 1 is compared with the split-1 run of the same
    geometry and consumer, which is computed once, by whichever case needs it first."""
    return {}


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _consumer_run(runs, geom, consumer, split, monkeypatch):
    """The consumer's schedule on a handle with the split forced, checked against the oracle: the (w, z, y) it returned."""
    key = (geom, consumer, split)
    if key in runs:
        return runs[key]
    n, m, N, S, seed, rho = geom
    pkw, okw, tol, expect = CONSUMERS[consumer]
    alpha = okw.get("alpha", 1.0)
    p = _problem(geom, SPLIT_BATCH, **pkw)
    z0, y0 = _state(p, 1000 + n)
    monkeypatch.setenv("ADMM_SCAN_SPLIT", str(split))            # read at set-up
    with pkg.Solver(p, pkg.Options(rho=rho, segments=S, **okw)) as s:
        path = s.path()
        assert path["segments"] == min(S, N) and path["scan_form"] == "mfma_gemm", path
        assert {k: path[k] for k in expect} == expect, path
        assert s.scan_geometry()["split"] == split, s.scan_geometry()        # a split that was not applied is a failure
        if consumer == "step_x_read_out":
            s.set_state(z=z0, y=y0)          # w = x-update(z0, y0), the w of the oracle's first iteration; z, y stay
            s.step_x()
            got = s.get()
            ref = dict(w=_reference(("x", geom), p, rho, 1.0, z0, y0, iters=1, resid_at=1)["w"], z=z0, y=y0)
        else:
            ref = _reference(("c", geom, tuple(sorted(pkw.items())), alpha), p, rho, alpha, z0, y0)
            got = schedule(s, z0, y0, first_residuals=True)
            if tol == TOL:
                assert _residuals_close(s, ref), key
    errs = [_rel(a, ref[k]) for a, k in zip(got, ("w", "z", "y"))]
    print(f"{gid(geom)} {consumer} split {split}: max relative |HIP - oracle| {max(errs):.3e} (bound {tol:.0e})")
    assert close(got, ref, tol), (key, errs)
    runs[key] = got
    return got


@pytest.mark.parametrize("split", SPLITS, ids=lambda v: f"split{v}")
@pytest.mark.parametrize("geom,consumer", SPLIT_CASES, ids=[f"{gid(g)}-{c}" for g, c in SPLIT_CASES])
def test_every_consumer_adds_the_slabs_of_every_split(gpu, consumer_runs, geom, consumer, split, monkeypatch):
    """Each consumer of the scan's output slabs (CONSUMERS) on a handle whose split-K factor is forced: against the oracle at
    the consumer's tolerance (1e-10; 1e-5 for the mixed-precision MFMA form), and -- splits 2, 4 and 8 -- against the split-1 run
    of the same geometry and consumer to AGREE = 1e-13 relative to max(1, |split 1|_inf) on w, z and y after the 39 iterations.
    A consumer that reads slab 0 only, or strides the slabs wrongly, misses both at every split > 1 and passes at split 1.

    Observed on an MI355X (maximum over the geometries and splits 2, 4, 8, relative as above): 1.5e-14 over all consumers
    (state_rows_unbounded; relaxed 1.2e-14, q_and_thrust_bound 6.5e-15, alternating 5.8e-15, mfma_fp64 5.2e-15, the rest below
    2e-15), exactly 0 at two of the empty-slice entries.  The mixed form is held to the same 1e-13: it differs
    from the oracle by up to 3.4e-7 here (SUB_F and ELIM_B run in fp32), but between splits by at most 5.5e-15, as the fp64
    forms do -- v, the scan, its slabs and the iterates are fp64 in every mode.  (A slab sum moved by an ulp could cross the
    fp32 rounding of one operand of those products, about one chance in 1e9 per element and iteration, and would then show
    near 1e-8; at these seeds none does, and the arithmetic, split order included, is deterministic.)"""
    got = _consumer_run(consumer_runs, geom, consumer, split, monkeypatch)
    if split == 1:
        return
    base = _consumer_run(consumer_runs, geom, consumer, 1, monkeypatch)
    diff = max(_rel(a, b) for a, b in zip(got, base))
    print(f"{gid(geom)} {consumer}: split {split} vs split 1: {diff:.3e} (bound {AGREE:.0e})")
    assert diff <= AGREE, (geom, consumer, split, diff)


# ---- refactors on a split handle ----
REFACTOR_GEOMETRY, REFACTOR_RHO, REFACTOR_SEED = SCAN_SLICEABLE[0], SCAN_REFACTOR_RHO, SCAN_REFACTOR_SEED    # (tests/test_shapes.py)


def test_refactors_keep_the_split_and_reload_the_ranges(gpu, monkeypatch):
    """admm_set_rho, then admm_update_problem to a second seed, on a handle with split 4: the packed matrices and the ranges
    are uploaded again and the slices follow the new ranges."""
    monkeypatch.setenv("ADMM_SCAN_SPLIT", "4")
    geom = REFACTOR_GEOMETRY
    n, m, N, S, seed, rho = geom
    p = _problem(geom, SPLIT_BATCH)
    p2 = pkg.random_ltv(N=N, n=n, m=m, batch=SPLIT_BATCH, seed=REFACTOR_SEED)
    z0, y0 = _state(p, 7)
    with pkg.Solver(p, pkg.Options(rho=rho, segments=S, flags=NO_MFMA)) as s:
        for step, (prob, r) in enumerate(((p, rho), (p, REFACTOR_RHO), (p2, REFACTOR_RHO))):
            if step == 1:
                s.set_rho(r)
            if step == 2:
                s.update_problem(prob)
            assert s.scan_geometry()["split"] == 4 and s.path()["alternating"] and s.path()["segments"] == S, step
            got = schedule(s, z0, y0, first_residuals=step != 1)
            ref = _reference(("refactor", step), prob, r, 1.0, z0, y0)
            assert close(got, ref) and _residuals_close(s, ref), step


# ---- per-instance scans ----
PI_FORMS = [((6, 3), "ADMM_PI_LANE_PER_QP"), ((6, 3), "ADMM_PI_ROWS"), ((4, 2), None), ((12, 6), None), ((8, 4), None)]
# (N, segments requested): N % S != 0, one-stage segments (S = N), 64 segments of 70 stages, and a request capped at N
PI_SEGMENTS = [(13, 2), (13, 3), (13, 13), (13, 64), (64, 3), (64, 64), (70, 3), (70, 64)]


def _pi_problem(shape, N, batch, soc):
    n, m = shape
    return pkg.random_instances(N=N, n=n, m=m, batch=batch, seed=700 + 16 * n + m, thrust_norm=soc)


@pytest.mark.parametrize("N,segments", PI_SEGMENTS, ids=[f"N{N}S{S}" for N, S in PI_SEGMENTS])
@pytest.mark.parametrize("shape,form", PI_FORMS, ids=[f"n{s[0]}m{s[1]}" + {None: "", "ADMM_PI_LANE_PER_QP": "-lane_per_qp",
                                                                           "ADMM_PI_ROWS": "-rows"}[f] for s, f in PI_FORMS])
def test_per_instance_scans_at_their_segment_counts(gpu, shape, form, N, segments, monkeypatch):
    """pscan / pseg / pseg_rows: 16 iterations on the schedule of test_every_per_instance_pair_and_form_matches_the_oracle
    against the one-QP oracle.  (4, 2) takes the form its batch selects (rows-over-lanes at 9 QPs, lane-per-QP at 70); the
    wide pairs run rows-over-lanes; the thrust-bound forms of the narrow pairs exist lane-per-QP only."""
    monkeypatch.delenv("ADMM_PI_LANE_PER_QP", raising=False)
    monkeypatch.delenv("ADMM_PI_ROWS", raising=False)
    if form:
        monkeypatch.setenv(form, "1")
    for batch in (9, 70):
        for soc in (False, True):
            if soc and form == "ADMM_PI_ROWS":
                continue
            p = _pi_problem(shape, N, batch, soc)
            z0, y0 = _state(p, batch)
            ref = _reference(("pi", shape, N, batch, soc), p, 0.3, 1.0, z0, y0, iters=16, resid_at=16)   # (run(6, 2) ends on one)
            with pkg.Solver(p, pkg.Options(rho=0.3, segments=segments)) as s:
                path = s.path()
                assert (path["per_instance"], path["segments"], path["alternating"], path["scan_form"]) == \
                    (True, min(segments, N), False, "per_qp"), path
                assert s.scan_geometry() == {"split": 1, "M": 0, "K": 0, "groups": 0}
                s.set_state(z=z0, y=y0)
                s.run(1, residual_every=1 if batch == 9 else 0)
                s.run(6, residual_every=3)
                s.iterate(3)
                s.run(6, residual_every=2)
                got = s.get()
                assert _residuals_close(s, ref), (batch, soc)
            assert close(got, ref), (batch, soc)


@pytest.mark.parametrize("N", [13, 70])
@pytest.mark.parametrize("shape", [(6, 3), (12, 6)], ids=["n6m3", "n12m6"])
def test_per_instance_request_of_65_segments_is_refused(gpu, shape, N):
    """The documented limit is on the request: a horizon shorter than 65 stages must not cap it into range."""
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(_pi_problem(shape, N, 9, False), pkg.Options(rho=0.3, segments=65))
    assert e.value.code == INVALID and "at most 64" in str(e.value)
