"""Every compiled (n, m) pair in every fused form, against the C oracle (tests/_shapes.py lists the pairs).

The fused kernels are templates over RESID x RELAX x HASQ x SOC x XFREE per pair, and prefetch depth, register budget and the
mapping of a stage's n + m rows onto the lanes depend on both the pair and the form: a cell that never runs is untested.
Each sweep checks the path it names through s.path() -- the default alternating-direction kernels only run when the
problem passes the forward-elimination probe, so every problem here is chosen to pass it (tests/_shapes.py ALT_TABLE) and
the probe's fallback warning is an error in this module.  PARITY UNPINNED."""
import itertools
import re
from contextlib import nullcontext

import numpy as np
import pytest

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd import _abi
from _shapes import ALT_TABLE, MFMA, PER_INSTANCE, PLAIN_ONLY, SHARED, SWEEP_N, SWEEP_SEGMENTS, WIDE, sid
from _sweep import TOL, close as _close, schedule as _schedule

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]
UNSUPPORTED = {v: k for k, v in _abi.STATUS_NAMES.items()}["ADMM_ERR_UNSUPPORTED"]


def test_an_uncompiled_pair_is_refused_with_the_compiled_list(gpu):
    p = pkg.random_ltv(N=8, n=11, m=5, batch=3, seed=1)
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(p, pkg.Options(rho=0.3))
    assert e.value.code == UNSUPPORTED
    listed = re.search(r"supported: (.*)$", str(e.value)).group(1)
    assert sorted((int(a), int(b)) for a, b in re.findall(r"\((\d+),\s*(\d+)\)", listed)) == SHARED


COMBOS = list(itertools.product([False, True], repeat=4))      # (q, thrust bound, relaxed, state rows unbounded)
CIDS = ["".join(c for c, on in zip("qsrx", t) if on) or "plain" for t in COMBOS]
# (shape, combo) -> the status admm_setup documents for it.  The one-lane kernels have every form at every compiled pair:
# nothing is refused (the MFMA family's refusals are tested below).
REFUSED = {}


@pytest.mark.parametrize("shape", SHARED, ids=sid)
@pytest.mark.parametrize("combo", COMBOS, ids=CIDS)
def test_every_pair_and_form_matches_the_oracle(gpu, shape, combo):
    """Default one-lane path (FLAG_NO_MFMA: the alternating-direction xfze / xbze kernels) and the plain path (xb + xfz)."""
    with_q, soc, relaxed, xfree = combo
    n, m = shape
    seed, rho = ALT_TABLE[shape]
    alpha = 1.6 if relaxed else 1.0
    for batch in (7, 67):                          # one wave with idle lanes; a second wave of 3 QPs (clamped lanes)
        p = pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=batch, seed=seed, with_q=with_q, state_bounds=not xfree, thrust_norm=soc)
        rng = np.random.default_rng(batch + n)
        z0, y0 = 0.1 * rng.standard_normal((batch, p.L)), 0.1 * rng.standard_normal((batch, p.L))
        ref = oc.solve(p, rho=rho, alpha=alpha, max_iter=39, stop=False, z0=z0, y0=y0)
        for flags, alternating in ((_abi.FLAG_NO_MFMA, shape not in PLAIN_ONLY), (_abi.FLAG_NO_MFMA | _abi.FLAG_NO_ALTERNATE, False)):
            opts = pkg.Options(rho=rho, alpha=alpha, segments=SWEEP_SEGMENTS, flags=flags)
            if (shape, combo) in REFUSED:
                with pytest.raises(pkg.AdmmError) as e:
                    pkg.Solver(p, opts)
                assert e.value.code == REFUSED[(shape, combo)]
                continue
            expect_warning = shape in PLAIN_ONLY and not flags & _abi.FLAG_NO_ALTERNATE
            with pytest.warns(RuntimeWarning, match="forward-elimination") if expect_warning else nullcontext():
                s = pkg.Solver(p, opts)
            with s:
                path = s.path()
                assert (path["alternating"], path["kernel_family"], path["segments"]) == \
                    (alternating, "one_lane_fp64", SWEEP_SEGMENTS), (batch, flags, path)
                got = _schedule(s, z0, y0, first_residuals=batch == 7)
            assert _close(got, ref), (batch, flags)


MFMA_BATCHES = [1, 15, 17, 63, 64, 65, 127, 128, 129]     # around the 16-QP panels and the pitch <= 64 / <= 128 rules


def _default_family(n, batch):
    pitch = (batch + 63) // 64 * 64
    return "mfma_fp64" if pitch <= 64 or (n >= 9 and pitch <= 128) else "one_lane_fp64"


@pytest.mark.parametrize("shape", MFMA, ids=sid)
@pytest.mark.parametrize("batch", MFMA_BATCHES)
def test_mfma_family_at_its_pairs_and_batch_edges(gpu, shape, batch):
    """fp64 MFMA within 1e-10, mixed within its stated 1e-5 (tests/test_gpu_mfma.py), and the default family the batch selects."""
    n, m = shape
    seed, rho = ALT_TABLE[shape]
    p = pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=batch, seed=seed, with_q=False)
    rng = np.random.default_rng(batch)
    z0, y0 = 0.1 * rng.standard_normal((batch, p.L)), 0.1 * rng.standard_normal((batch, p.L))
    for alpha in (1.0, 1.6):
        ref = oc.solve(p, rho=rho, alpha=alpha, max_iter=39, stop=False, z0=z0, y0=y0)
        for kw, family, tol in ((dict(), _default_family(n, batch), TOL),
                                (dict(precision_mode=_abi.PRECISION_FP64_MFMA), "mfma_fp64", TOL),
                                (dict(precision_mode=_abi.PRECISION_MIXED), "mfma_mixed", 1e-5)):
            with pkg.Solver(p, pkg.Options(rho=rho, alpha=alpha, segments=SWEEP_SEGMENTS, **kw)) as s:
                path = s.path()
                assert path["kernel_family"] == family, (alpha, kw, path)
                assert path["alternating"] or kw.get("precision_mode") == _abi.PRECISION_MIXED, (alpha, kw, path)
                got = _schedule(s, z0, y0, first_residuals=alpha == 1.0)
            assert _close(got, ref, tol), (alpha, kw)


@pytest.mark.parametrize("shape", MFMA, ids=sid)
def test_mfma_linear_term_rule(gpu, shape):
    """A linear term runs on the fp64 MFMA form of (6, 3) for batches of up to 128 QPs only: refused everywhere else."""
    n, m = shape
    seed, rho = ALT_TABLE[shape]
    for batch in (1, 128, 129):
        p = pkg.random_ltv(N=SWEEP_N, n=n, m=m, batch=batch, seed=seed, with_q=True)
        for mode in (_abi.PRECISION_FP64_MFMA, _abi.PRECISION_MIXED):
            opts = pkg.Options(rho=rho, segments=SWEEP_SEGMENTS, precision_mode=mode)
            if shape == (6, 3) and batch <= 128 and mode == _abi.PRECISION_FP64_MFMA:
                rng = np.random.default_rng(batch)
                z0, y0 = 0.1 * rng.standard_normal((batch, p.L)), 0.1 * rng.standard_normal((batch, p.L))
                with pkg.Solver(p, opts) as s:
                    assert s.path()["kernel_family"] == "mfma_fp64"
                    got = _schedule(s, z0, y0, first_residuals=True)
                assert _close(got, oc.solve(p, rho=rho, max_iter=39, stop=False, z0=z0, y0=y0))
                continue
            with pytest.raises(pkg.AdmmError) as e:
                pkg.Solver(p, opts)
            assert e.value.code == UNSUPPORTED and "linear term" in str(e.value), (batch, mode, e.value)


PCOMBOS = list(itertools.product([False, True], repeat=3))     # (q, relaxed, per-instance box)


@pytest.mark.parametrize("shape", PER_INSTANCE, ids=sid)
@pytest.mark.parametrize("combo", PCOMBOS, ids=["".join(c for c, on in zip("qrb", t) if on) or "plain" for t in PCOMBOS])
def test_every_per_instance_pair_and_form_matches_the_oracle(gpu, shape, combo, monkeypatch):
    """The per-instance sweeps at every compiled pair: with and without the thrust bound, one segment and four, each of the
    lane-per-QP and the rows-over-lanes family that exists for the pair (wide pairs: rows-over-lanes only; the thrust-bound
    forms of the narrow pairs: lane-per-QP only)."""
    with_q, relaxed, pbox = combo
    n, m = shape
    alpha = 1.6 if relaxed else 1.0
    for soc in (False, True):
        for segments in (1, 4):
            batch = 9 if segments == 1 else 70
            p = pkg.random_instances(N=16, n=n, m=m, batch=batch, seed=500 + 16 * n + m, with_q=with_q, instance_bounds=pbox,
                                     thrust_norm=soc)
            rng = np.random.default_rng(batch)
            z0, y0 = 0.1 * rng.standard_normal((batch, p.L)), 0.1 * rng.standard_normal((batch, p.L))
            ref = oc.solve(p, rho=0.3, alpha=alpha, max_iter=16, stop=False, z0=z0, y0=y0)
            forms = ("ADMM_PI_ROWS",) if shape in WIDE else ("ADMM_PI_LANE_PER_QP",) if soc else ("ADMM_PI_LANE_PER_QP", "ADMM_PI_ROWS")
            for form in forms:
                monkeypatch.delenv("ADMM_PI_LANE_PER_QP", raising=False)
                monkeypatch.delenv("ADMM_PI_ROWS", raising=False)
                monkeypatch.setenv(form, "1")
                with pkg.Solver(p, pkg.Options(rho=0.3, alpha=alpha, segments=segments)) as s:
                    path = s.path()
                    assert (path["per_instance"], path["segments"], path["alternating"]) == (True, segments, False), path
                    s.set_state(z=z0, y=y0)
                    s.run(1, residual_every=1 if segments == 1 else 0)       # the (z, y)-form kernels
                    s.run(6, residual_every=3)
                    s.iterate(3)
                    s.run(6, residual_every=2)
                    got = s.get()
                assert _close(got, ref), (soc, segments, form)
