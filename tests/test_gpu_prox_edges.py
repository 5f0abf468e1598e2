"""Every copy of the z-update projection at its exact edges, bit for bit.

tests/_prox_cases.py builds a decoupled problem (B = 0, R = 0, A a permutation, rho a power of two) on which the x-update returns
w_u = z_u - y_u and w_x = A^(k+1) x0 exactly for every kernel family, and lays a table of edges over its stages and QPs: control
blocks with ||v_u|| == ub, == kap, nrm - kap == ub and one ulp either side of each, zero blocks under a bound and a weight, box
rows on, one ulp inside and one ulp outside their bounds, pinned rows, bounds of -0.0 (tests/test_prox_host.py checks the table,
the reference and the host factors on the CPU).  set_state puts (z0, y0) on the handle; iteration 1 runs each family's (z, y)-form
kernels on the table, iterations 2 and 3 the v-form kernels on the full-mantissa values iteration 1 left, and get() after each runs
the read-out kernels.

Asserted after every iteration, on all rows of every QP: w equals the model's w bitwise (the injection: no lane is left out);
z and y equal the reference, np.array_equal (zeros compare by value), and hold no NaN -- the reference is the model of
_prox_cases.py in exact rationals with one rounding per fp64 operation, in the device's form of the relaxation,
fma(alpha, w, (1 - alpha) z); the residual norms within 1e-12 max(1, |ref|) of the reference in np.longdouble (sums whose order
differs by family); ||z_u|| <= ub (1 + 2^-52) at the stages with a thrust bound, z_u == 0 where the classifier says coast, y == 0
where it says interior or on the edge.  There is no tolerance on the iterates: a contracted v - c v, an approximate square root
or a division on the wrong side of an edge moves y by an ulp and fails.

The mixed-precision MFMA mode is left out: its stated accuracy is 1e-5 (tests/test_gpu_mfma.py), not bit for bit."""
import dataclasses
import itertools

import numpy as np
import pytest

import admm_library_amd as pkg
import _prox_cases as pc
from admm_library_amd import _abi
from admm_library_amd.solver import Solver
from _shapes import MFMA, PER_INSTANCE, SHARED, WIDE, sid

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]
BATCHES = (7, 67)          # idle lanes; a second wave of three QPs and an odd last column of a double2 pair
SEGMENTS = (1, 3)
UNSUPPORTED = {v: k for k, v in _abi.STATUS_NAMES.items()}["ADMM_ERR_UNSUPPORTED"]
FAMILIES = {"default": _abi.FLAG_NO_MFMA, "plain": _abi.FLAG_NO_MFMA | _abi.FLAG_NO_ALTERNATE, "unfused": _abi.FLAG_UNFUSED}


def _same(got, ref, what, ctx, nb):
    """np.array_equal, with the first differing (QP, stage, row) in the message."""
    assert not np.isnan(got).any(), (what, "NaN at", np.argwhere(np.isnan(got))[:4].tolist(), ctx)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        b, i = (int(x) for x in bad[0])
        raise AssertionError(f"{what} differs from the reference in {len(bad)} entries; first at QP {b}, stage {i // nb}, row {i % nb}: "
                             f"{got[b, i].hex()} != {ref[b, i].hex()} ({got[b, i]!r} != {ref[b, i]!r}); {ctx}")


def _check(s, case, ref, mode, first_residuals, ctx):
    """Three iterations from (z0, y0) through `mode` -- "run" (admm_run, residual_every alternating between 0 and 1), "iterate"
    (admm_iterate) or "steps" (admm_step_x, admm_step_z) -- with get() after each, against the reference."""
    p = case.p
    nb, m = p.nb, p.m
    ball = np.isfinite(case.ub)
    s.set_state(z=case.z0, y=case.y0)
    for it in (1, 2, 3):
        resid = mode != "iterate" and (it % 2 == 1) == first_residuals
        if mode == "run":
            s.run(1, residual_every=1 if resid else 0)
        elif mode == "iterate":
            s.iterate(1)
        else:
            s.step_x()
            s.step_z(residuals=resid)
        w, z, y = s.get()
        st, c = ref[it - 1], (ctx, mode, "iteration", it)
        _same(w, st["w"], "w", c, nb)
        _same(z, st["z"], "z", c, nb)
        _same(y, st["y"], "y", c, nb)
        if resid:
            for name, got, want in zip(("r", "s", "nw", "nz", "ny"), s.residuals(), st["res"]):
                err = np.abs(got.astype(np.longdouble) - want)
                assert (err <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (name, float(err.max()), c)
        zu = z.reshape(p.batch, pc.N, nb)[:, :, :m].astype(np.longdouble)
        nrm = np.sqrt((zu * zu).sum(axis=2))
        assert (nrm[:, ball] <= case.ub[ball].astype(np.longdouble) * (1 + np.longdouble(2.0) ** -52)).all(), c
        assert not z[st["coast"]].any() and not y[st["free"]].any(), c


CELLS = list(itertools.product([False, True], [True, False], [1.0, 1.5]))          # (q, state rows bounded, alpha)


@pytest.mark.parametrize("form", pc.FORMS)
@pytest.mark.parametrize("shape", SHARED, ids=sid)
def test_shared_dynamics_families(gpu, shape, form):
    """The default (alternating-direction xfze / xbze), plain fused (xb + xfz) and unfused (xb, xf, zdual / zdual_soc) kernels of
    every compiled pair: box only, thrust bound, fuel without and with a bound; with and without q; state rows bounded and unbounded
    (XFREE); alpha 1 and 1.5; batches 7 and 67 at one and three segments; through admm_run and admm_iterate, the unfused family
    also through admm_step_x + admm_step_z with zrows = 2 (n + m), so that a chunk boundary falls inside the horizon.  The fuel +
    bound form also runs at rho = 0.25."""
    n, m = shape
    cells = [c + (1.0,) for c in CELLS] + ([c + (0.25,) for c in CELLS[:2]] if form == "fuel_ball" else [])
    for idx, (with_q, xbounded, alpha, rho) in enumerate(cells):
        for batch, segments in zip(BATCHES, SEGMENTS if idx % 2 == 0 else SEGMENTS[::-1]):
            case = pc.make(n, m, batch, form, with_q=with_q, xbounded=xbounded, rho=rho)
            ref = pc.reference(n, m, batch, form, xbounded=xbounded, rho=rho, alpha=alpha)
            for family, flags in FAMILIES.items():
                ctx = (shape, form, family, dict(q=with_q, xbounded=xbounded, alpha=alpha, rho=rho, batch=batch, segments=segments))
                zrows = 2 * (n + m) if family == "unfused" else 0
                with pkg.Solver(case.p, pkg.Options(rho=rho, alpha=alpha, segments=segments, flags=flags, zrows=zrows)) as s:
                    path = s.path()
                    assert (path["alternating"], path["kernel_family"], path["segments"], path["xfree"]) == \
                        (family == "default", "one_lane_fp64", segments, not xbounded), (ctx, path)
                    _check(s, case, ref, "run", batch == 7, ctx)
                    _check(s, case, ref, "iterate", False, ctx)
                    if family == "unfused":
                        assert s.geometry()["zrows"] == zrows and s.geometry()["zchunks"] > 1, s.geometry()
                        _check(s, case, ref, "steps", batch == 67, ctx)


@pytest.mark.parametrize("shape", MFMA, ids=sid)
def test_mfma_fp64_family(gpu, shape):
    """The two projection sites of admm_mfma.hpp, box form: batches 7 and 67, 129 where the family serves it (n >= 9); a linear
    term only where it is served, (6, 3) up to 128 QPs."""
    n, m = shape
    for idx, (with_q, xbounded, alpha) in enumerate(CELLS):
        if with_q and shape != (6, 3):
            continue
        for batch, segments in zip(BATCHES + ((129,) if n >= 9 else ()), (SEGMENTS if idx % 2 == 0 else SEGMENTS[::-1]) + (3,)):
            case = pc.make(n, m, batch, "box", with_q=with_q, xbounded=xbounded)
            ref = pc.reference(n, m, batch, "box", xbounded=xbounded, alpha=alpha)
            ctx = (shape, "mfma_fp64", dict(q=with_q, xbounded=xbounded, alpha=alpha, batch=batch, segments=segments))
            with pkg.Solver(case.p, pkg.Options(rho=1.0, alpha=alpha, segments=segments, precision_mode=_abi.PRECISION_FP64_MFMA)) as s:
                path = s.path()
                assert (path["alternating"], path["kernel_family"], path["segments"]) == (True, "mfma_fp64", segments), (ctx, path)
                _check(s, case, ref, "run", batch == 7, ctx)
                _check(s, case, ref, "iterate", False, ctx)


def _pi_families(shape, form):
    """As tests/test_gpu_shapes.py: wide pairs run rows-over-lanes only, the thrust-bound forms of the narrow pairs lane-per-QP only."""
    if shape in WIDE:
        return ("ADMM_PI_ROWS",)
    return ("ADMM_PI_LANE_PER_QP",) if form == "ball" else ("ADMM_PI_LANE_PER_QP", "ADMM_PI_ROWS")


@pytest.mark.parametrize("form", ["box", "ball"])
@pytest.mark.parametrize("shape", PER_INSTANCE, ids=sid)
def test_per_instance_families(gpu, shape, form, monkeypatch):
    """Per-instance dynamics with a box per QP (the kinds of the table rotate through the QPs: a kernel that reads another QP's box
    fails): ball_factor, the sweeps and the read-out of admm_pinst.hpp, admm_pinst_rows.hpp and admm_pinst_wide.hpp; the rows
    factorisation at (6, 3).  The thrust-bound form also runs at rho = 0.25."""
    n, m = shape
    families = _pi_families(shape, form) + (("ADMM_PI_ROWS_FACTOR",) if shape == (6, 3) and form == "box" else ())
    cells = [c + (1.0,) for c in CELLS] + ([c + (0.25,) for c in CELLS[:2]] if form == "ball" else [])
    for idx, (with_q, xbounded, alpha, rho) in enumerate(cells):
        for batch, segments in zip(BATCHES, SEGMENTS if idx % 2 == 0 else SEGMENTS[::-1]):
            case = pc.make(n, m, batch, form, per_instance=True, with_q=with_q, xbounded=xbounded, rho=rho)
            ref = pc.reference(n, m, batch, form, per_instance=True, xbounded=xbounded, rho=rho, alpha=alpha)
            for family in families:
                for name in ("ADMM_PI_LANE_PER_QP", "ADMM_PI_ROWS", "ADMM_PI_ROWS_FACTOR"):
                    monkeypatch.delenv(name, raising=False)
                monkeypatch.setenv(family, "1")
                ctx = (shape, form, family, dict(q=with_q, xbounded=xbounded, alpha=alpha, rho=rho, batch=batch, segments=segments))
                with pkg.Solver(case.p, pkg.Options(rho=rho, alpha=alpha, segments=segments)) as s:
                    path = s.path()
                    assert (path["per_instance"], path["segments"], path["alternating"]) == (True, segments, False), (ctx, path)
                    _check(s, case, ref, "run", batch == 7, ctx)
                    _check(s, case, ref, "iterate", False, ctx)


def test_refusals(gpu):
    """A fuel term is refused with per-instance dynamics; admm_step_z with per-instance bounds."""
    case = pc.make(6, 3, 7, "box", per_instance=True, xbounded=False)
    free = dataclasses.replace(case.p, lo=np.full_like(case.p.lo, -np.inf), hi=np.full_like(case.p.hi, np.inf))
    with pytest.raises((ValueError, pkg.AdmmError), match="fuel"):
        pkg.Solver(dataclasses.replace(free, fuel=np.float64(0.25)), pkg.Options(rho=1.0))
    with pkg.Solver(case.p, pkg.Options(rho=1.0, segments=1)) as s:
        assert s.path()["per_instance"]
        s.set_state(z=case.z0, y=case.y0)
        s.step_x()
        with pytest.raises(pkg.AdmmError) as e:
            s.step_z()
        assert e.value.code == UNSUPPORTED


def test_single_rank_time_sharded_handle(gpu):
    """One time-sharded handle holding every segment, box form (it refuses admm_step_z and a fuel term)."""
    for batch, segments, alpha in ((7, 3, 1.0), (67, 3, 1.5), (67, 1, 1.0)):
        case = pc.make(6, 3, batch, "box", with_q=batch == 67)
        ref = pc.reference(6, 3, batch, "box", alpha=alpha)
        with Solver(case.p, pkg.Options(rho=1.0, alpha=alpha, segments=segments), timeshard=(0, 1, None)) as s:
            assert s.window()["segs_total"] == segments and s.path()["segments"] == segments
            _check(s, case, ref, "run", batch == 7, ("timeshard", batch, segments, alpha))
            _check(s, case, ref, "iterate", False, ("timeshard", batch, segments, alpha))
            s.step_x()
            with pytest.raises(pkg.AdmmError) as e:
                s.step_z()
            assert e.value.code == UNSUPPORTED
