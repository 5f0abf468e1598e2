"""What a handle's z-update kind refuses after set-up: admm_profile of a fused path on every kind, the
receding-horizon step and the infeasibility probe on consensus and half-space handles, and each kind's read-outs on a handle of
another kind.  Every refusal is an argument check: it returns its status and its sentence -- compared for equality -- and leaves the
handle's state bit for bit as it was."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch  # (before the library is loaded, as in tests/test_gpu_device_io.py: both then share one HIP runtime)

import admm_library_amd as pkg
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2
INF = np.inf
N, n, m, BATCH, GROUP = 8, 6, 3, 4, 2

PROFILE = {"consensus": "a scenario-consensus handle", "soft": "a handle with soft weights", "halfspace": "a handle with half-spaces"}
MPC = {"consensus": "a scenario-consensus handle (a per-QP plant step is not the coupled problem's)",
       "halfspace": "a handle with half-spaces (a per-QP plane is not window-relative: it would have to shift with the horizon)"}
PROBE = {"consensus": "a scenario-consensus handle (a per-QP Farkas certificate is not the coupled problem's)",
         "halfspace": "a handle with half-spaces (the Farkas certificate is written for boxes and the thrust ball)"}


def problem(kind):
    p = pkg.random_ltv(N=N, n=n, m=m, batch=BATCH, seed=41, state_bounds=kind != "halfspace")
    rng = np.random.default_rng(7)
    if kind == "consensus":
        return dataclasses.replace(p, consensus=GROUP)
    if kind == "soft":
        soft = np.full((N, n + m), INF)
        soft[:, m:] = rng.uniform(0.5, 2.0, (N, n))
        return dataclasses.replace(p, soft=soft)
    if kind == "halfspace":
        a = rng.standard_normal((BATCH, N, 3))
        return dataclasses.replace(p, hs_a=a, hs_b=0.15 * np.linalg.norm(a, axis=2) * rng.standard_normal((BATCH, N)))
    return p


@pytest.fixture(scope="module")
def handles(gpu):
    hs = {k: pkg.Solver(problem(k), pkg.Options(rho=0.3)) for k in ("plain", "consensus", "soft", "halfspace")}
    for s in hs.values():
        s.iterate(5)
    yield hs
    for s in hs.values():
        s.close()


def refused(s, rc, status, message):
    assert (rc, s._lib.admm_last_error().decode()) == (status, message)


def tensors():
    t = {k: torch.zeros(BATCH, dtype=torch.float64, device="cuda:0") for k in ("a", "b", "c")}
    t["u"] = torch.zeros((BATCH, m), dtype=torch.float64, device="cuda:0")
    t["x"] = torch.zeros((BATCH, n), dtype=torch.float64, device="cuda:0")
    t["flag"] = torch.zeros(BATCH, dtype=torch.int32, device="cuda:0")
    return t


def tptr(t, ctype=_abi.c_double_p):
    return C.cast(C.c_void_p(t.data_ptr()), ctype)


@pytest.mark.parametrize("kind", ["consensus", "soft", "halfspace"])
def test_a_kind_refuses_what_its_z_update_cannot_serve(handles, kind):
    s = handles[kind]
    lib, h = s._lib, s._h
    before = s.get()
    ms = np.zeros(6)
    for fused_path in (1, 2, 3, 4):
        for residuals in (0, 1):
            refused(s, lib.admm_profile(h, 3, residuals, fused_path, _abi.dptr(ms)), UNSUPPORTED,
                    f"admm_profile: {PROFILE[kind]} runs the unfused path only (fused_path = 0)")
    if kind != "soft":                       # (a soft handle has a receding-horizon step and a probe: tests/test_gpu_soft.py)
        t = tensors()
        step = _abi.CMpcStep(tail=_abi.MPC_TAILS["copy"], reserved=0)
        u, x = np.zeros((BATCH, m)), np.zeros((BATCH, n))
        refused(s, lib.admm_mpc_advance(h, C.byref(step), _abi.dptr(u), _abi.dptr(x)), UNSUPPORTED,
                f"admm_mpc_advance: not available on {MPC[kind]}")
        refused(s, lib.admm_mpc_advance_device(h, C.byref(step), tptr(t["u"]), tptr(t["x"]), None), UNSUPPORTED,
                f"admm_mpc_advance_device: not available on {MPC[kind]}")
        sep, drift, defect, flag = np.zeros(BATCH), np.zeros(BATCH), np.zeros(BATCH), np.zeros(BATCH, np.int32)
        refused(s, lib.admm_probe_infeasibility(h, 4, 1e-6, _abi.dptr(sep), _abi.dptr(drift), _abi.dptr(defect), _abi.iptr(flag), None),
                UNSUPPORTED, f"admm_probe_infeasibility: not available on {PROBE[kind]}")
        refused(s, lib.admm_probe_infeasibility_device(h, 4, 1e-6, tptr(t["a"]), tptr(t["b"]), tptr(t["c"]),
                                                       tptr(t["flag"], _abi.c_int32_p), None, None),
                UNSUPPORTED, f"admm_probe_infeasibility_device: not available on {PROBE[kind]}")
    after = s.get()
    for name, a, b in zip("wzy", before, after):
        assert np.array_equal(a, b), name


def test_a_plain_handle_has_none_of_the_read_outs(handles):
    s = handles["plain"]
    lib, h = s._lib, s._h
    before = s.get()
    t = tensors()
    d, i = np.zeros(BATCH * N * n), np.zeros(BATCH, np.int32)
    dp, ip = _abi.dptr(d), _abi.iptr(i)
    ta, tb, tf = tptr(t["a"]), tptr(t["b"]), tptr(t["flag"], _abi.c_int32_p)
    groups = "the handle has no scenario groups (set it up with admm_setup_consensus)"
    weights = "the handle has no soft weights (set it up with admm_setup_soft)"
    planes = "the handle has no half-spaces (set it up with admm_setup_halfspace)"
    refused(s, lib.admm_get_consensus(h, dp), INVALID, "admm_get_consensus: " + groups)
    refused(s, lib.admm_get_consensus_device(h, ta, None), INVALID, "admm_get_consensus_device: " + groups)
    refused(s, lib.admm_get_soft_report(h, dp, dp, ip), INVALID, "admm_get_soft_report: " + weights)
    refused(s, lib.admm_get_soft_report_device(h, ta, tb, tf, None), INVALID, "admm_get_soft_report_device: " + weights)
    refused(s, lib.admm_get_halfspace(h, dp, dp), INVALID, "admm_get_halfspace: " + planes)
    refused(s, lib.admm_get_halfspace_report(h, dp, ip, None), INVALID, "admm_get_halfspace_report: " + planes)
    refused(s, lib.admm_get_halfspace_report_device(h, ta, tf, None, None), INVALID, "admm_get_halfspace_report_device: " + planes)
    # ... and nothing can be added to it
    refused(s, lib.admm_set_soft(h, dp), INVALID, "admm_set_soft: soft weights cannot be added to a handle (set it up with admm_setup_soft)")
    added = "half-spaces cannot be added to a handle (set it up with admm_setup_halfspace)"
    refused(s, lib.admm_set_halfspace(h, dp, dp), INVALID, "admm_set_halfspace: " + added)
    refused(s, lib.admm_set_halfspace_device(h, ta, tb, None), INVALID, "admm_set_halfspace_device: " + added)
    after = s.get()
    for name, a, b in zip("wzy", before, after):
        assert np.array_equal(a, b), name
