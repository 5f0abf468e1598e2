"""Receding-horizon step (ADMM_HIP_HAS_MPC), host side: the ABI surface, the ctypes mirror of admm_mpc_step, the
register report of the two kernels, the host shift helper against an explicit loop over blocks, and the closed loop driven by the
CPU oracle: a warm start from the shifted solution beats a cold start at every step.  No GPU."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi
from admm_library_amd import mpc

import oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("admm_mpc_advance", "admm_mpc_advance_device")


def test_abi_surface(lib):
    hdr = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert "#define ADMM_HIP_HAS_MPC 1" in hdr
    assert "#define ADMM_HIP_ABI_VERSION 9" in hdr and lib.admm_abi_version() == 9
    for name in SYMBOLS:
        assert name in pkg.solver._SIGNATURES and hasattr(lib, name)
    assert pkg.mpc_batch is mpc.mpc_batch and pkg.shift_horizon is mpc.shift_horizon and hasattr(pkg.Solver, "mpc_advance")


def test_null_handle_is_invalid(lib):
    step = _abi.CMpcStep()
    assert lib.admm_mpc_advance(None, C.byref(step), None, None) == 1
    assert lib.admm_mpc_advance_device(None, C.byref(step), None, None, None) == 1
    assert "NULL handle" in lib.admm_last_error().decode()


def test_ctypes_struct_has_the_c_size(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "admm_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu %d %d\\n\", sizeof(admm_mpc_step), offsetof(admm_mpc_step, q_tail),\n"
                   "  offsetof(admm_mpc_step, tail), offsetof(admm_mpc_step, reserved), ADMM_MPC_TAIL_COPY, ADMM_MPC_TAIL_ZERO); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_abi.CMpcStep), _abi.CMpcStep.q_tail.offset, _abi.CMpcStep.tail.offset, _abi.CMpcStep.reserved.offset,
                   _abi.MPC_TAIL_COPY, _abi.MPC_TAIL_ZERO]
    assert C.sizeof(_abi.CMpcStep) == 6 * 8 + 2 * 4


def test_the_new_kernels_do_not_spill(tmp_path):
    """csrc/admm_mpc.hip compiled on its own with the library's flags and the compiler's resource report: both kernels are there
    and neither uses scratch memory or LDS (DESIGN.md §2.11 records the table this prints)."""
    import __graft_entry__ as ge
    assert "admm_mpc.hip" in ge.RUNTIME_UNITS and "admm_mpc_kernels.hpp" in ge.HEADERS
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_mpc.hip"), "-o", str(tmp_path / "admm_mpc.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "mpc_" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, LDS {x["lds"]} B, scratch {x["scratch"]} B, '
              f'occupancy {x["occupancy"]}')
    assert sorted(x["name"].split("::")[-1] for x in mine) == ["mpc_edges_kernel", "mpc_shift_kernel"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 and x["lds"] == 0 for x in mine), mine
    assert all(x["scratch"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"]]


@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("tail", ["copy", "zero"])
@pytest.mark.parametrize("fill", [False, True])
def test_shift_helper_against_a_loop_over_blocks(N, tail, fill):
    rng = np.random.default_rng(100 * N + fill)
    nb, batch = 3, 4
    a = rng.standard_normal((batch, N * nb))
    keep = a.copy()
    q_tail = rng.standard_normal((batch, nb)) if fill else None
    want = np.empty_like(a)
    for b in range(batch):
        for k in range(N - 1):
            for i in range(nb):
                want[b, k * nb + i] = a[b, (k + 1) * nb + i]
        for i in range(nb):
            want[b, (N - 1) * nb + i] = q_tail[b, i] if fill else (a[b, (N - 1) * nb + i] if tail == "copy" else 0.0)
    got = mpc.shift_horizon(a, nb, tail, q_tail)
    assert np.array_equal(got, want) and np.array_equal(a, keep) and got is not a
    with pytest.raises(ValueError):
        mpc.shift_horizon(a, nb, "circular")
    with pytest.raises(ValueError):
        mpc.shift_horizon(a[:, :-1], nb)


QP = dict(rho=1.0, check_interval=5, max_iter=2000)


def _oracle(p, z0, y0):
    r = oracle_c.solve(p, z0=z0, y0=y0, **QP)
    return r["w"], r["z"], r["y"], r["iters_run"], int(np.sum(r["status"]))


@pytest.mark.parametrize("tail,noise", [("copy", None), ("zero", None), ("copy", 1e-3)])
def test_warm_starts_beat_cold_starts_on_the_oracle(tail, noise):
    """mpc_batch(on_device=False, qp_solver=oracle) on double_integrator(N=30, batch=8), 6 steps, rho = 1, check_interval 5: every
    warm solve of steps 1 .. 5 takes strictly fewer iterations than a cold solve of the same QP (45 against 90-95 with tail copy
    and no noise; 45-55 with tail zero or process noise 1e-3)."""
    p = pkg.double_integrator(N=30, batch=8)
    res = pkg.mpc_batch(p, 6, tail=tail, noise=noise, on_device=False, qp_solver=_oracle)
    assert res.X.shape == (7, 8, 2) and res.U.shape == (6, 8, 1) and res.iterations.shape == (6,) and res.converged.shape == (6,)
    assert np.array_equal(res.X[0], p.x0) and (res.converged == 8).all()
    cold = [_oracle(dataclasses.replace(p, x0=res.X[t].copy()), None, None)[3] for t in range(6)]
    print(f"tail {tail}, noise {noise}: warm {res.iterations.tolist()}, cold {cold}")
    assert res.iterations[0] == cold[0]
    for t in range(1, 6):
        assert res.iterations[t] < cold[t], (t, res.iterations.tolist(), cold)
    # the loop is the plant: X[t + 1] = A X[t] + B U[t] (+ noise), and replaying the recorded states reproduces the run
    dx = None if noise is None else noise * np.random.default_rng(0).standard_normal((6, 8, 2))
    for t in range(6):
        assert np.array_equal(res.X[t + 1], mpc.plant_step(res.X[t], res.U[t], p.A, p.B, None if dx is None else dx[t]))
    again = pkg.mpc_batch(p, 6, tail=tail, on_device=False, qp_solver=_oracle, replay=res.X)
    assert np.array_equal(again.U, res.U) and np.array_equal(again.X, res.X) and np.array_equal(again.iterations, res.iterations)
