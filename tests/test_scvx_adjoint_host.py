"""Costates and the optimality certificate of the SCvx loop (ADMM_HIP_HAS_SCVX_ADJOINT), host side: scvx.adjoint
against extended-precision central differences of the nonlinear cost, with a mutation check of the tolerance; the violation rule on
hand-made cases; the loop end to end with certify=True; the ABI surface, the struct's layout, the refusals that need no GPU, the
kernel's resource report; and that the constants the GPU test takes its bounds from are current.  No GPU."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd import scvx as sc

import _scvx_adjoint_case as ac
import _scvx_case as case
import _scvx_device_case as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (-case.U_MAX, case.U_MAX)
FD_SHAPES = [(3, 7), (3, case.N)]

# max |scvx.adjoint - long-double central differences (h = 1e-3)| of (grad, dJdx0), absolute, as this file printed it (rounded up to
# two digits), by (B, N, point).  It does not move with h over 1e-2 .. 1e-5 (1.686e-4 +- 1e-8 at (3, 7)): it is not the truncation
# of the differences but the adjoint's own error, that of A, B (fp64 central differences at eps = 1e-6, ~5e-8 per entry) times
# costates up to 7.6e3 (N = 7) and 4.4e4 (N = 80); entries of grad reach 257 and 1.8e3, of dJdx0 7.6e3 and 4.4e4.
# The tolerance of the test is 10 x the recorded figure.
FD_OBSERVED = {
    (3, 7, "zero"): (1.7e-4, 5.2e-4), (3, 7, "interior"): (2.0e-4, 4.5e-4), (3, 7, "clipped"): (1.5e-4, 4.8e-4),
    (3, 80, "zero"): (7.6e-4, 1.7e-2), (3, 80, "interior"): (6.4e-4, 1.3e-2), (3, 80, "clipped"): (2.4e-4, 3.8e-3),
}


def _adjoint(x0, u, x, **kw):
    return sc.adjoint(x0, u, x, dc.DT, case.Q, case.R, case.QN, *BOX, **kw)


def _fd_errors(B, N, point, got=None):
    x0, u, x, g, g0 = ac.fd_case(B, N, point)
    if got is None:
        c = _adjoint(x0, u, x)
        got = dict(grad=c.grad, dJdx0=c.dJdx0)
    return float(np.abs(got["grad"] - g).max()), float(np.abs(got["dJdx0"] - g0).max())


@pytest.mark.parametrize("point", ac.FD_POINTS)
@pytest.mark.parametrize("B,N", FD_SHAPES)
def test_grad_and_dJdx0_match_extended_precision_central_differences(B, N, point):
    """grad and dJdx0 of scvx.adjoint against central differences of dc.ld_trajectory_cost(dc.ld_rollout(...)) in long double at
    u = 0, a random interior u and a clipped random u, at (3, 7) and on the scenario's horizon: within 10 x FD_OBSERVED (above:
    1.5e-4 .. 7.6e-4 on grad, 4.5e-4 .. 1.7e-2 on dJdx0 -- relative 7e-7 and below)."""
    eg, e0 = _fd_errors(B, N, point)
    og, o0 = FD_OBSERVED[B, N, point]
    print(f"adjoint vs central differences, B={B} N={N} {point}: grad {eg:.3e} (recorded {og:.1e}), dJdx0 {e0:.3e} (recorded {o0:.1e})")
    assert eg <= 10.0 * og and e0 <= 10.0 * o0
    assert og <= 2.0 * eg and o0 <= 2.0 * e0, "FD_OBSERVED is stale: more than twice today's difference"


@pytest.mark.parametrize("wrong", ac.WRONG)
def test_the_tolerance_tells_a_wrong_recursion_from_a_right_one(wrong):
    """One deliberate error in the recursion at a time (ac.recursion, fp64, the Jacobians of scvx.linearise): A not transposed, B
    indexed as if stored 3 x 6, Q used for QN, the stage index off by one (stage k pairs B_k with nu_{k+2}).  On every input of the
    test above the erroneous grad or dJdx0 is at least 100 x that test's tolerance away from the central differences (measured: 4.2e3 x
    and more), while the unmutated restatement passes.
    A fifth error, A_k read for A_{k+1}, is the one the kernel's layout invites (its A runs one stage behind B, q, u).  A varies
    slowly along the horizon, so this test cannot see it 100-fold: it exceeds the tolerance by 71 x (N = 7) to 525 x (N = 80), mostly in
    dJdx0 -- asserted: by more than 10 x.  What holds the kernel to the right A is the GPU test against scvx.adjoint at 1e-13."""
    for B, N in FD_SHAPES:
        for point in ac.FD_POINTS:
            x0, u, x, g, g0 = ac.fd_case(B, N, point)
            A, Bm = sc.linearise(np.concatenate([x0[:, None, :], x[:, :-1, :]], axis=1), u, dc.DT)
            tg, t0 = (10.0 * v for v in FD_OBSERVED[B, N, point])
            eg, e0 = _fd_errors(B, N, point, ac.recursion(A, Bm, x, u, case.Q, case.R, case.QN))
            assert eg <= tg and e0 <= t0
            eg, e0 = _fd_errors(B, N, point, ac.recursion(A, Bm, x, u, case.Q, case.R, case.QN, wrong=wrong))
            factor = max(eg / tg, e0 / t0)
            print(f"{wrong}, B={B} N={N} {point}: {factor:.3g} x the tolerance")
            assert factor >= (10.0 if wrong == "A_one_stage_late" else 100.0), (B, N, point, factor)


def test_stat_and_n_bound_on_hand_made_cases():
    """Every branch of the violation rule: a fixed component (u_lo == u_hi) counts 0 whatever its gradient, and is on a bound; on
    the lower bound only a negative gradient violates, on the upper only a positive one; in the interior |g|; a NaN anywhere in a
    trajectory's grad makes its stat NaN and leaves n_bound alone; infinite bounds are never met."""
    lo, hi = np.array([-1.0, 2.0, -np.inf]), np.array([1.0, 2.0, np.inf])
    u = np.array([[[-1.0, 2.0, 5.0], [1.0, 2.0, -7.0]],          # lower | fixed | interior;  upper | fixed | interior
                  [[-1.0, 2.0, 0.0], [1.0, 2.0, 0.0]],
                  [[0.5, 2.0, 0.0], [-0.5, 2.0, 0.0]],
                  [[-1.0, 2.0, 0.0], [0.0, 2.0, 0.0]]])
    g = np.array([[[3.0, -50.0, -0.25], [-4.0, 60.0, 0.125]],    # pushes inwards on both bounds: only the interior counts
                  [[-3.0, 9.0, 0.0], [4.5, -9.0, 0.0]],          # pushes outwards: max(-g, 0) = 3 below, max(g, 0) = 4.5 above
                  [[-0.75, 1e9, 0.0], [0.5, 0.0, 0.0]],          # interior: |g|
                  [[1.0, 0.0, 0.0], [0.0, np.nan, 0.0]]])        # a NaN, in a fixed component of all places
    stat, nb = sc.stationarity(g, u, lo, hi)
    np.testing.assert_array_equal(stat, [0.25, 4.5, 0.75, np.nan])
    np.testing.assert_array_equal(nb, [4, 4, 2, 3])
    assert nb.dtype == np.int32
    s1, n1 = sc.stationarity(g[1], u[1], lo, hi)                   # one trajectory, no batch axis
    assert float(s1) == 4.5 and int(n1) == 4
    # through adjoint: the same rule on its own grad, with and without the batch axis
    x0, uu, x = ac.scattered_clipped(3, 7)
    c = _adjoint(x0, uu, x)
    s, n = sc.stationarity(c.grad, uu, *BOX)
    np.testing.assert_array_equal(c.stat, s)
    np.testing.assert_array_equal(c.n_bound, n)
    assert (c.n_bound == (np.abs(uu) == case.U_MAX).sum(axis=(1, 2))).all() and c.n_bound.min() >= 7
    one = _adjoint(x0[1], uu[1], x[1])
    assert isinstance(one.stat, float) and one.stat == c.stat[1] and one.n_bound == c.n_bound[1]
    for k in ("nu", "primer", "grad", "dJdx0"):
        np.testing.assert_array_equal(getattr(one, k), getattr(c, k)[1])
    assert c.nu.shape == (3, 7, 6) and c.primer.shape == c.grad.shape == (3, 7, 3) and c.dJdx0.shape == (3, 6)
    with pytest.raises(ValueError, match="A and B go together"):
        _adjoint(x0, uu, x, A=ac.host_jacobians(3, 7)[0])


def test_scvx_end_to_end_with_the_certificate():
    """The scenario with the CPU oracle as QP solver: certify=True changes nothing else in the result; the certificate is
    scvx.adjoint at the returned trajectory; stat falls from its value at u = 0 by at least 1e3 (measured: 767.8 -> 1.9e-2), and at
    least 200 of the 240 control components end on a bound (217).  scvx_batch the same way on two trajectories."""
    args = (case.X0, case.N, case.DT, case.Q, case.R, case.QN, *BOX)
    plain = sc.scvx(*args, qp_solver=case.oracle_qp_solver(**case.QP), **case.SCVX)
    res = sc.scvx(*args, qp_solver=case.oracle_qp_solver(**case.QP), certify=True, **case.SCVX)
    assert plain.certificate is None and plain.converged
    for f in dataclasses.fields(sc.ScvxResult):
        if f.name in ("u", "x"):
            np.testing.assert_array_equal(getattr(res, f.name), getattr(plain, f.name))
        elif f.name != "certificate":
            assert getattr(res, f.name) == getattr(plain, f.name), f.name
    c = res.certificate
    u0 = np.zeros((case.N, 3))
    start = sc.adjoint(case.X0, u0, sc.rollout(case.X0, u0, case.DT), case.DT, case.Q, case.R, case.QN, *BOX)
    print(f"scvx with the oracle: stat {start.stat:.4g} -> {c.stat:.3e} ({c.stat / start.stat:.2e}), {c.n_bound} of {3 * case.N} "
          f"components on a bound, {res.outer_iterations} outer iterations")
    assert c.stat <= 1e-3 * start.stat
    assert c.n_bound >= 200
    again = sc.adjoint(case.X0, res.u, res.x, case.DT, case.Q, case.R, case.QN, *BOX)
    for k in ("nu", "primer", "grad", "dJdx0", "stat", "n_bound"):
        np.testing.assert_array_equal(getattr(c, k), getattr(again, k))
    # Lawden's condition on the nonlinear solution: interior components satisfy R u = primer to stat, bounded ones carry its sign
    inside = np.abs(res.u) < case.U_MAX
    assert np.abs((res.u @ case.R.T - c.primer)[inside]).max() <= c.stat
    pushing = ~inside & (np.abs(c.grad) > c.stat)
    assert (np.sign(res.u[pushing]) == np.sign(c.primer[pushing])).all()

    x0s = case.X0[None] * np.array([[1.0], [1.02]])
    kw = dict(case.SCVX, max_outer=3)
    pb = sc.scvx_batch(x0s, 12, case.DT, *args[3:], qp_solver=case.oracle_qp_solver(**case.QP), **kw)
    rb = sc.scvx_batch(x0s, 12, case.DT, *args[3:], qp_solver=case.oracle_qp_solver(**case.QP), certify=True, **kw)
    for r, p in zip(rb, pb):
        np.testing.assert_array_equal(r.u, p.u)
        np.testing.assert_array_equal(r.x, p.x)
        assert (r.cost, r.accepted, r.converged, r.history) == (p.cost, p.accepted, p.converged, p.history) and p.certificate is None
    whole = sc.adjoint(x0s, np.stack([r.u for r in rb]), np.stack([r.x for r in rb]), case.DT, case.Q, case.R, case.QN, *BOX)
    for b, r in enumerate(rb):
        np.testing.assert_array_equal(r.certificate.grad, whole.grad[b])
        assert r.certificate.stat == whole.stat[b] and r.certificate.n_bound == whole.n_bound[b]


def test_abi_surface(lib):
    hdr = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert "#define ADMM_HIP_HAS_SCVX_ADJOINT 1" in hdr
    assert "#define ADMM_HIP_ABI_VERSION 9" in hdr and lib.admm_abi_version() == 9
    assert "admm_scvx_adjoint_device" in pkg.solver._SIGNATURES and hasattr(lib, "admm_scvx_adjoint_device")


def test_ctypes_struct_has_the_c_size(tmp_path):
    """sizeof and the offset of the last field of admm_scvx_adjoint_out, from a C program compiled against the header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "admm_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu\\n\", sizeof(admm_scvx_adjoint_out), offsetof(admm_scvx_adjoint_out, n_bound)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_abi.CScvxAdjointOut), _abi.CScvxAdjointOut.n_bound.offset] == [48, 40]


def test_argument_checks_come_before_any_hip_call(lib):
    """Every ADMM_ERR_INVALID case that needs no GPU, with the argument's name, on a machine without a GPU too: these checks
    precede the first HIP call.  The pointers that are not NULL are host arrays the call never reads."""
    params = _abi.CScvxParams(fd_eps=1e-6, tol=1e-6, rho_reject=0.1, rho_expand=0.7)
    buf = np.full(4 * 2 * 36, 3.0)
    nb = np.full(4, 3, np.int32)
    d, null = _abi.dptr(buf), _abi.c_double_p()
    full = _abi.CScvxAdjointOut(nu=d, primer=d, grad=d, dJdx0=d, stat=d, n_bound=_abi.iptr(nb))
    name = "admm_scvx_adjoint_device"

    def refused(word, N=2, batch=4, params=C.byref(params), ub=d, A=d, B=d, q=d, out=C.byref(full)):
        assert lib.admm_scvx_adjoint_device(0, N, batch, params, ub, A, B, q, out, None) == 1, word
        assert lib.admm_last_error().decode() == f"{name}: {word}"

    refused("N must be >= 1", N=0)
    refused("N must be >= 1", N=-3)
    refused("batch must be >= 1", batch=0)
    refused("batch must be >= 1", batch=-1)
    refused("N must be <= 900000", N=900001)
    refused("params is NULL", params=None)
    for arg in ("ub", "A", "B", "q"):
        refused(f"{arg} is NULL", **{arg: null})
    refused("out is NULL", out=None)
    refused("every field of out is NULL", out=C.byref(_abi.CScvxAdjointOut()))
    assert (buf == 3.0).all() and (nb == 3).all()


def test_the_adjoint_kernel_does_not_spill(tmp_path):
    """csrc/admm_scvx_adjoint.hip compiled on its own with the library's flags and the compiler's resource report: exactly one
    scvx_adjoint_kernel, no scratch, no spills, LDS within 64 KB."""
    import __graft_entry__ as ge
    assert "admm_scvx_adjoint.hip" in ge.RUNTIME_UNITS and "admm_scvx_adjoint_kernels.hpp" in ge.HEADERS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_scvx_adjoint.hip"), "-o", str(tmp_path / "admm_scvx_adjoint.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "scvx_" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, LDS {x["lds"]} B, scratch {x["scratch"]} B, '
              f'occupancy {x["occupancy"]}')
    assert [x["name"].split("<")[0].split("::")[-1] for x in mine] == ["scvx_adjoint_kernel"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 and x["sgpr_spill"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"]]
    assert all(x["lds"] <= 65536 for x in rows) and mine[0]["lds"] > 0


# ---- the inputs of tests/test_gpu_scvx_adjoint.py
@pytest.mark.parametrize("B,N", dc.SHAPES)
def test_recorded_fp64_vs_long_double_constants_are_current(B, N):
    """ac.FP64_VS_LD[B, N] bounds what scvx.adjoint (fp64) differs from the long-double recursion per output on
    scattered_clipped(B, N) today and is no more than twice it: the GPU bounds (dc.GPU_MARGIN x the constant) are neither stale nor
    padded.  stat differs by no more than grad does (it is one of grad's entries or 0).  About a third of the controls sit on each
    bound."""
    got = ac.fp64_vs_ld(B, N)
    print(f"adjoint fp64 vs long double, B={B} N={N}:", {k: f"{v:.3e}" for k, v in got.items()})
    for k, c in ac.FP64_VS_LD[B, N].items():
        assert got[k] <= c <= 2.0 * got[k], (k, got[k], c)
    assert got["stat"] <= ac.FP64_VS_LD[B, N]["grad"]
    u = ac.scattered_clipped(B, N)[1]
    if u.size >= 100:
        assert 0.25 <= (u == -case.U_MAX).mean() <= 0.42 and 0.25 <= (u == case.U_MAX).mean() <= 0.42


def test_the_linearisation_bound_covers_a_perturbation_of_that_size():
    """ac.linearisation_bound, from which the GPU test of certify() takes its tolerance: A, B moved by +-5e-7 per entry (random
    signs) move every output of the long-double recursion by less than the bound and by more than a hundredth of it -- the bound is
    first order and worst case, not padding (measured at (65, 64): nu 8.4e-5 of 1.0e-3, grad 4.0e-6 of 4.5e-5)."""
    for B, N in dc.SHAPES[1:3]:
        x0, u, x = ac.scattered_clipped(B, N)
        A, Bm = ac.host_jacobians(B, N)
        ld = ac.recursion(A, Bm, x, u, case.Q, case.R, case.QN, ac.LD)
        bound = ac.linearisation_bound(A, Bm, ld["nu"])
        rng = np.random.default_rng(1)
        moved = ac.recursion(A + ac.LIN_BOUND * rng.choice([-1.0, 1.0], A.shape), Bm + ac.LIN_BOUND * rng.choice([-1.0, 1.0], Bm.shape), x, u,
                             case.Q, case.R, case.QN, ac.LD)
        err = ac.scaled_errors(moved, ld, ac.nu_scale(ld["nu"]))
        print(f"B={B} N={N}: bound", {k: f"{v:.3e}" for k, v in bound.items()}, "moved", {k: f"{v:.3e}" for k, v in err.items()})
        for k, v in err.items():
            assert 0.01 * bound[k] <= v <= bound[k], (k, v, bound[k])
