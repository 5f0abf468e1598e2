"""The decoupled problem, the exact reference and the edge table of tests/_prox_cases.py, checked on the CPU before the GPU sweep
(tests/test_gpu_prox_edges.py) relies on them.

Which form the device uses: the kernels form the relaxation as fma(alpha, w, (1 - alpha) z) and the sum of squares as an fma
chain in row order -- the reference's default (relax_fma=True, norm_fma=True).  oracle/admm_oracle.c is compiled with
-ffp-contract=off and writes alpha * w + (1 - alpha) * z: two roundings; oracle/admm_ref.py and tests/_fuel_ref.py (NumPy) do the
same and also round each square before adding.  Each oracle is compared, bit for bit, with the variant of the reference that takes
its form; at alpha = 1 and on the exact tuples of the table the variants coincide."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
import admm_ref as ar
import oracle_c as oc
import _fuel_ref as fr
import _prox_cases as pc
from admm_library_amd import _abi
from admm_library_amd.solver import host_factor, host_factor_mfma
from _shapes import MFMA, SHARED, sid


def test_exact_operations():
    """The rounded operations against hardware fp64 (IEEE add, multiply, divide and square root are correctly rounded too), and
    the fma where one rounding and two differ."""
    rng = np.random.default_rng(3)
    for a, b in rng.standard_normal((200, 2)) * 2.0 ** rng.integers(-80, 80, (200, 1)):
        a, b = float(a), float(b)
        assert pc.add(a, b) == a + b and pc.sub(a, b) == a - b and pc.mul(a, b) == a * b and pc.div(a, b) == a / b
        assert pc.sqrt(abs(a)) == np.sqrt(abs(a))
    for x in (0.0, 1.0, 2.0, 0.25, 2.0 ** 200, 2.0 ** -200, 25.0 / 64, pc.up(1.0), pc.dn(1.0), pc.up(4.0), 3.0, 2.0 ** -1000):
        assert pc.sqrt(x) == np.sqrt(x)
    e = 2.0 ** -30
    assert pc.fma(1 + e, 1 - e, -1.0) == -e * e and pc.add(pc.mul(1 + e, 1 - e), -1.0) == 0.0
    assert pc.fma(0.0, 5.0, -0.0) == 0.0 and pc.add(-0.0, 3.0) == 3.0 and pc.mul(-0.0, 3.0) == 0.0 and pc.div(0.0, 3.0) == 0.0
    assert pc.add(pc.INF, -1.0) == pc.INF and pc.sub(1.0, pc.INF) == -pc.INF


@pytest.mark.parametrize("shape", SHARED, ids=sid)
def test_the_classifier_finds_every_case_of_the_table(shape):
    """Every pair of SHARED (m = 1 among them: |v| takes the place of the norm), every form, batch 7: each block case of the form
    and -- with state rows bounded -- each box case is found in the first iteration's v, at every QP column a different one."""
    n, m = shape
    for form in pc.FORMS:
        for xbounded in (True, False):
            case = pc.make(n, m, 7, form, xbounded=xbounded)
            v = pc.iterate(case, case.z0, case.y0)[1]
            blocks, rows = pc.classify(case, v)
            found = set().union(*(blocks[b][k] for b in range(7) for k in range(pc.N)))
            assert pc.BLOCK_CASES[form] <= found, (form, pc.BLOCK_CASES[form] - found)
            box = set().union(*(rows[b][k][j] for b in range(7) for k in range(pc.N) for j in range(n + m)))
            if xbounded:
                assert pc.BOX_CASES <= box, (form, xbounded, pc.BOX_CASES - box)
            else:                      # only the control rows of the stages that keep their box
                assert box & pc.BOX_CASES, (form, box)
            for k in range(pc.N):      # the QP columns of a stage hold different blocks (m = 1 has only +r and -r on the edge)
                if case.soc[k]:
                    blk = {tuple(v.reshape(7, pc.N, n + m)[b, k, :m]) for b in range(7)}
                    assert len(blk) >= (6 if m > 1 else 5), (form, k)
            assert len({(float(case.ub[k]), float(case.kap[k])) for k in range(pc.N) if case.soc[k]}) == case.soc.sum()
    pcase = pc.make(n, m, 7, "ball", per_instance=True)          # per-QP boxes: the kinds rotate through the QPs
    assert pcase.p.lo.shape == (7, pc.N, n + m) and any(not np.array_equal(pcase.p.lo[0], pcase.p.lo[b]) for b in range(1, 7))
    rows = pc.classify(pcase, pc.iterate(pcase, pcase.z0, pcase.y0)[1])[1]
    assert pc.BOX_CASES <= set().union(*(rows[b][k][j] for b in range(7) for k in range(pc.N) for j in range(n + m)))


def test_a_case_does_not_depend_on_the_batch_size():
    a, b = pc.make(5, 2, 7, "fuel_ball", with_q=True), pc.make(5, 2, 67, "fuel_ball", with_q=True)
    for x, y in ((a.z0, b.z0), (a.y0, b.y0), (a.p.x0, b.p.x0), (a.p.q, b.p.q)):
        assert np.array_equal(x, y[:7])
    assert np.array_equal(a.p.lo, b.p.lo) and np.array_equal(a.ub, b.ub)
    ref = pc.reference(5, 2, 7, "fuel_ball")
    assert np.array_equal(ref[2]["z"], pc.run(a, 3)[2]["z"]) and not ref[0]["z"].flags.writeable


ORACLE_SHAPES = [(1, 1), (5, 2), (6, 3), (12, 6)]


@pytest.mark.parametrize("alpha", [1.0, 1.5])
@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=sid)
def test_three_iterations_equal_the_oracles(lib, shape, alpha):
    """admm_ref.solve, oracle_c.solve and -- with weights -- _fuel_ref.solve on the decoupled problem, bit for bit, against the
    reference in each oracle's form (module docstring).  The same comparison settles the injection on the CPU: the oracles'
    Riccati sweep returns w_u = z_u - y_u and w_x = A^(k+1) x0 exactly."""
    n, m = shape
    for form in pc.FORMS:
        for rho in pc.RHOS:
            case = pc.make(n, m, 7, form, with_q=True, rho=rho)
            p = case.p
            mine = {key: pc.run(case, 3, alpha, relax_fma=False, norm_fma=key) for key in (True, False)}
            for it in (1, 2, 3):
                kw = dict(rho=rho, alpha=alpha, max_iter=it, z0=case.z0, y0=case.y0, stop=False)
                outs = [("fuel_ref", False, fr.solve(p, **kw))]
                if p.fuel is None:
                    outs.append(("admm_ref", False, ar.solve(p.A, p.B, p.Q, p.R, p.QN, p.x0, p.lo, p.hi, p.N, q=p.q, unorm=p.unorm, **kw)))
                    res = oc.solve(p, **kw)
                    outs.append(("oracle_c", True, ar.Result(w=res["w"], z=res["z"], y=res["y"], iters_run=it, iters=None, status=None,
                                                             r=None, s=None, history=None)))
                for name, fused_norm, got in outs:
                    st = mine[fused_norm][it - 1]
                    for key, a in (("w", got.w), ("z", got.z), ("y", got.y)):
                        assert not np.isnan(a).any()
                        assert np.array_equal(a, st[key]), (name, form, rho, it, key, np.abs(a - st[key]).max())


def _dyadic(a):
    """Every entry an exact zero, a power of two (either sign) or an infinity."""
    a = np.asarray(a, np.float64).ravel()
    a = a[np.isfinite(a) & (a != 0.0)]
    mant, _ = np.frexp(np.abs(a))
    return bool(np.all(mant == 0.5))


@pytest.mark.parametrize("shape", SHARED, ids=sid)
def test_host_factors_of_the_decoupled_problem_are_exact(lib, shape):
    """The library's own host factor at segments 1 and 3 and both rho: the forward-elimination probe passes (so the default path
    runs the alternating kernels), and every operator of the plain, alternating and MFMA records -- the control-row operators
    among them -- is an exact zero or a power of two, so that no product of the x-update rounds.  (The records also hold the box
    and the thrust bound: the problem is given an unbounded box for this check, whose infinities pass.)"""
    n, m = shape
    for rho in pc.RHOS:
        for segments in (1, 3):
            case = pc.make(n, m, 7, "box", xbounded=False, rho=rho)
            p = dataclasses.replace(case.p, lo=np.full_like(case.p.lo, -np.inf), hi=np.full_like(case.p.hi, np.inf))
            hf = host_factor(p, rho, segments)
            assert hf["alt_ok"], (shape, rho, segments)
            for key in ("K", "Sinv", "recB", "recF", "recS", "scanW", "recFE", "recBE", "scanWB"):
                assert _dyadic(hf[key]), (shape, rho, segments, key)
            assert not hf["K"].any() and np.array_equal(hf["Sinv"], np.broadcast_to(np.eye(m) / rho, (pc.N, m, m)))
            if shape in MFMA:
                recMF, recMB, ok = host_factor_mfma(p, rho, segments, _abi.PRECISION_FP64_MFMA)
                assert ok
                for rec in (recMF, recMB):
                    assert rec.shape[1] % 8 == 0 and _dyadic(rec.view(np.float64)), (shape, rho, segments)
            for form in ("ball", "fuel_ball"):                       # the probe does not depend on the box or the bounds
                assert host_factor(pc.make(n, m, 7, form, with_q=True, rho=rho).p, rho, segments)["alt_ok"]


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/admm_prox.hpp: the single definition of the z-update that every kernel family composes, on the host
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prox_block(tmp_path_factory):
    """tests/prox_block.cpp + csrc/admm_prox.hpp as a shared object (host compiler, no contraction: the header's explicit fma
    calls are the only fused operations, as on the device)."""
    import __graft_entry__ as ge
    assert "admm_prox.hpp" in ge.HEADERS
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    so = tmp_path_factory.mktemp("prox") / "prox_block.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", ge.CSRC,
                    os.path.join(os.path.dirname(os.path.abspath(__file__)), "prox_block.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.prox_zupdate.argtypes = [C.c_int] * 7 + [dp] * 7 + [C.c_double] + [dp] * 4
    lib.prox_zupdate.restype = C.c_int
    return lib


@pytest.mark.parametrize("alpha", [1.0, 1.5])
@pytest.mark.parametrize("shape", [(2, 1), (6, 3)], ids=sid)
def test_the_header_z_update_equals_the_reference(prox_block, shape, alpha):
    """The block z-update of admm_prox.hpp on the model iterates, three iterations, batch 7: the old state from (z, y) in the first
    iteration and rebuilt from the header's own v+ afterwards (the v-form).  z and y equal the exact-rational reference of the
    GPU sweep with np.array_equal; the five sums give the reference's residual norms within 1e-12 max(1, |ref|).  The forms
    without a fuel weight also run with the per-instance kernels' factor."""
    n, m = shape
    batch = 7
    for form in pc.FORMS:
        for rho in (pc.RHOS if form == "fuel_ball" else (1.0,)):
            case = pc.make(n, m, batch, form, rho=rho)
            ref = pc.reference(n, m, batch, form, rho=rho, alpha=alpha)
            lo, hi = (np.ascontiguousarray(a.reshape(batch, -1)) for a in (case.lo, case.hi))
            for fuel in ((1,) if form.startswith("fuel") else (1, 0)):
                s0, s1, vin = case.y0, case.z0, 0
                for it, st in enumerate(ref):
                    v, z, y = (np.full_like(case.z0, np.nan) for _ in range(3))
                    sums = np.full((batch, 5), np.nan)
                    rc = prox_block.prox_zupdate(n, m, vin, int(alpha != 1.0), fuel, batch, pc.N, np.ascontiguousarray(s0),
                                                 np.ascontiguousarray(s1), np.ascontiguousarray(st["w"]), lo, hi, case.ub, case.kap,
                                                 alpha, v, z, y, sums)
                    ctx = (form, rho, fuel, it)
                    assert rc == 0
                    assert not np.isnan(z).any() and not np.isnan(y).any(), ctx
                    assert np.array_equal(z, st["z"]), (ctx, "z", np.abs(z - st["z"]).max())
                    assert np.array_equal(y, st["y"]), (ctx, "y", np.abs(y - st["y"]).max())
                    assert np.array_equal(v, st["v"]), (ctx, "v")
                    root = np.sqrt(sums.astype(np.longdouble))
                    got = (root[:, 0], rho * root[:, 1], root[:, 2], root[:, 3], rho * root[:, 4])
                    for name, g, want in zip(("r", "s", "nw", "nz", "ny"), got, st["res"]):
                        err = np.abs(g - want)
                        assert (err <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (ctx, name, float(err.max()))
                    s0, s1, vin = v, np.zeros_like(v), 1
