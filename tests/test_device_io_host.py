"""CPU side of the device-memory entry points (ABI v9): the header declares them and the library exports them, the ABI version
moved, the Python wrapper refuses what is not a contiguous fp64 CUDA tensor with ValueError before the library is called, and
every *_device call refuses a NULL handle.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import admm_library_amd as pkg
from admm_library_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_FNS = ["admm_setup_device", "admm_update_problem_device", "admm_update_instances_device", "admm_set_state_device",
              "admm_get_device"]
CODE = {v: k for k, v in _abi.STATUS_NAMES.items()}


def test_header_declares_and_library_exports_the_device_forms(lib):
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    for fn in DEVICE_FNS:
        assert re.search(r"\bint " + fn + r"\([^)]*void\* hip_stream\);", header), fn
        assert getattr(lib, fn) is not None


def test_abi_version_is_9(lib):
    header = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert "#define ADMM_HIP_ABI_VERSION 9" in header
    assert _abi.ABI_VERSION == 9 == lib.admm_abi_version()


def test_device_forms_refuse_a_null_handle(lib):
    assert lib.admm_setup_device(None, None, None, None) == CODE["ADMM_ERR_INVALID"]
    assert lib.admm_update_problem_device(None, None, None) == CODE["ADMM_ERR_INVALID"]
    assert lib.admm_update_instances_device(None, None, None, None) == CODE["ADMM_ERR_INVALID"]
    assert lib.admm_set_state_device(None, None, None, None, None) == CODE["ADMM_ERR_INVALID"]
    assert lib.admm_get_device(None, None, None, None, None) == CODE["ADMM_ERR_INVALID"]
    assert "NULL" in lib.admm_last_error().decode()


def _cpu_device_problem(p):
    """A DeviceProblem whose tensors are still in host memory (what the wrapper must refuse)."""
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float64))    # noqa: E731
    return pkg.DeviceProblem(N=p.N, A=t(p.A), B=t(p.B), Q=t(p.Q), R=t(p.R), QN=t(p.QN), x0=t(p.x0), lo=t(p.lo), hi=t(p.hi), q=t(p.q))


@pytest.mark.parametrize("what", ["cpu", "float32", "non_contiguous", "wrong_shape", "pinned"])
def test_wrapper_refuses_bad_tensors_before_the_library(lib, what, monkeypatch):
    p = pkg.random_instances(N=6, n=6, m=3, batch=4, seed=3)
    dp = _cpu_device_problem(p)
    if what == "float32":
        dp.A = dp.A.float()
    elif what == "non_contiguous":
        dp.B = dp.B.transpose(-1, -2).contiguous().transpose(-1, -2)
    elif what == "wrong_shape":
        dp.x0 = dp.x0[:, :5].contiguous()
    elif what == "pinned" and torch.cuda.is_available():
        dp.lo = dp.lo.pin_memory()
    called = []
    for fn in ("admm_setup", "admm_setup_device"):
        monkeypatch.setattr(lib, fn, lambda *a, fn=fn: called.append(fn) or 0)
    with pytest.raises(ValueError):
        pkg.Solver(dp, pkg.Options(rho=0.3))
    assert called == []
    # the problem's shape checks hold for the device form as for Problem
    assert dp.batch == 4 and dp.L == p.L and dp.per_instance and dp.per_instance_bounds


def test_device_problem_from_problem_keeps_fields_and_shapes():
    p = pkg.random_ltv(N=8, n=6, m=3, batch=5, seed=2, thrust_norm=True)
    assert [f.name for f in pkg.DeviceProblem.__dataclass_fields__.values()] == \
           [f.name for f in pkg.Problem.__dataclass_fields__.values()]
    if not torch.cuda.is_available():
        return
    dp = pkg.DeviceProblem.from_problem(p, "cuda:0")
    dp.validate()
    for name in ("A", "B", "Q", "R", "QN", "x0", "lo", "hi", "q", "unorm"):
        np.testing.assert_array_equal(getattr(dp, name).cpu().numpy(), np.asarray(getattr(p, name)))
