"""matlab/admm_mex.cpp on the GPU: the gateway and the MEX stand-in of tests/mex_shim (it restates MathWorks' documented behaviour;
it is not MATLAB) are linked against libadmm_hip.so, loaded next to the ctypes host and compared with Solver BIT FOR BIT -- it
is the same library on the same data, so there is no tolerance.  The arrays go in as MATLAB lays them out: column-major, with
the dimensions MATLAB would give them."""
import dataclasses
import os

import numpy as np
import pytest

import _mex
import admm_library_amd as pkg
from _mex import Ref, mx, raw
from admm_library_amd import _abi

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:.*forward-elimination form failed:RuntimeWarning")]

CASES = {
    "cw": (lambda: pkg.cw_rendezvous(N=20, batch=5), dict(rho=0.05, adapt_interval=20)),                  # shared LTI (6, 3)
    "ltv": (lambda: pkg.random_ltv(N=12, n=4, m=2, batch=70, seed=3, with_q=False), dict(rho=0.3)),      # more than one wave
    "pinst": (lambda: pkg.random_instances(N=10, n=6, m=3, batch=9, seed=4, with_q=False), dict(rho=0.3, adapt_interval=20)),
    "pinst_wide": (lambda: pkg.random_instances(N=8, n=9, m=3, batch=5, seed=5, with_q=False), dict(rho=0.3)),
    "unorm": (lambda: pkg.cw_rendezvous(N=20, batch=5, thrust_norm=True), dict(rho=0.05)),
    "fuel": (lambda: pkg.cw_rendezvous_fuel(N=20, batch=5), dict(rho=0.05)),
    "q": (lambda: pkg.random_ltv(N=12, n=6, m=3, batch=7, seed=6, with_q=True), dict(rho=0.3)),
}
SOLVE = dict(max_iter=300, check_interval=10, eps_abs=1e-5, eps_rel=1e-5)


@pytest.fixture(scope="module")
def gateway(gpu, tmp_path_factory):
    """gateway + stand-in + bridge, linked against the library the ctypes host has loaded."""
    libpath = os.path.abspath(pkg.library_path())
    so = _mex.compile_shared(tmp_path_factory.mktemp("mex") / "admm_mex_gpu.so", extra_flags=[libpath, "-Wl,-rpath," + os.path.dirname(libpath)])
    return _mex.Bridge(so)


@pytest.fixture
def mexf(gateway, monkeypatch):
    """A gateway without handles; the Solver lays per-instance dynamics out column-major on the host, as MATLAB holds them."""
    monkeypatch.setenv("ADMM_PY_COLMAJOR", "1")
    gateway.fire_at_exit()
    gateway.saved.clear()
    yield gateway
    gateway.fire_at_exit()
    assert gateway.live() == 0


def matlab_problem(p):
    """The MATLAB struct of a Problem: the buffers the ctypes host hands to the C ABI, under MATLAB's dimensions."""
    cp, keep = _abi.marshal_problem(p)
    N, n, m, b, nb = p.N, p.n, p.m, p.batch, p.nb
    tail = {0: (), 1: (N,), 2: (N, b)}
    s = {"N": mx(float(N)), "A": raw(keep["A"], (n, n) + tail[cp.time_varying]), "B": raw(keep["B"], (n, m) + tail[cp.time_varying]),
         "Q": raw(keep["Q"], (n, n)), "R": raw(keep["R"], (m, m)), "QN": raw(keep["QN"], (n, n)), "x0": raw(keep["x0"], (n, b)),
         "lo": raw(keep["lo"], (nb,) + (tail[cp.stage_bounds] or (1,))), "hi": raw(keep["hi"], (nb,) + (tail[cp.stage_bounds] or (1,)))}
    if p.per_instance:
        s["per_instance"] = mx(1, "logical")
    if p.per_instance_bounds:
        s["per_instance_bounds"] = mx(1, "logical")
    if p.q is not None:
        s["q"] = raw(keep["q"], (N * nb, b))
    if p.unorm is not None:
        s["unorm"] = raw(keep["unorm"], (keep["unorm"].size, 1))
    if p.fuel is not None:
        f = _abi.marshal_fuel(p)
        s["fuel"] = raw(f, (f.size, 1))
    return s


def both(b, name, **extra):
    """The same problem and options on a gateway handle (saved as "h") and on a Solver."""
    make, opt = CASES[name]
    p = make()
    opt = dict(opt, **extra)
    r = b.call(1, "setup", matlab_problem(p), {k: mx(float(v)) for k, v in opt.items()}, save="h")
    assert r.rc == 0 and r.warnings == [], (r.error_text, r.warnings)
    return p, pkg.Solver(p, pkg.Options(**opt))


def state(b, p):
    r = b.call(3, "get", Ref("h"))
    assert r.rc == 0 and r.warnings == [] and all(o.dims == (p.L, p.batch) for o in r.outputs)
    return [o.data.reshape(p.batch, p.L) for o in r.outputs]          # L x batch column-major = (batch, L) in C order


def same_state(b, p, s):
    for got, want in zip(state(b, p), s.get()):
        assert np.array_equal(got, want)


def same_info(r, s, info):
    assert r.rc == 0, r.error_text
    o = r.outputs[0].data
    for k in ("iters_run", "n_converged", "max_r", "max_s", "rho", "rho_updates", "mixed_iters"):
        assert o[k].data[0] == getattr(info, k), k
    assert np.isfinite(o["solve_ms"].data[0]) and o["solve_ms"].data[0] >= 0          # a wall-clock time: the one field that differs
    for k in ("iters", "status", "r", "s"):
        assert o[k].data.dtype == getattr(info, k).dtype and np.array_equal(o[k].data, getattr(info, k)), k
    assert np.array_equal(o["rho_per_qp"].data, s.rho_per_qp())


def column(a, p):
    return mx(np.ascontiguousarray(a).T)          # (batch, L) -> L x batch


@pytest.mark.parametrize("name", list(CASES))
def test_iterate_and_get_equal_the_ctypes_host(mexf, name):
    b = mexf
    p, s = both(b, name)
    with s:
        same_state(b, p, s)                                     # z = y = w = 0 after setup
        for k in (7, 2):
            r = b.call(0, "iterate", Ref("h"), mx(float(k)))
            assert r.rc == 0 and r.warnings == []
            s.run(k)
            same_state(b, p, s)


@pytest.mark.parametrize("name", list(CASES))
def test_solve_cold_and_warm_equals_the_ctypes_host(mexf, name):
    b = mexf
    p, s = both(b, name, **SOLVE)
    with s:
        r = b.call(1, "solve", Ref("h"))
        info = s.solve()
        assert info.iters_run > 0
        same_info(r, s, info)
        same_state(b, p, s)
        _, z, y = s.get()
        z0, y0 = 0.5 * z, 0.25 * y
        same_info(b.call(1, "solve", Ref("h"), column(z0, p), column(y0, p)), s, s.solve(z0, y0))
        same_state(b, p, s)
        same_info(b.call(1, "solve", Ref("h"), _mex.EMPTY, column(y0, p)), s, s.solve(None, y0))      # [] = keep the handle's z
        same_state(b, p, s)


@pytest.mark.parametrize("name", list(CASES))
def test_update_then_solve_equals_update_problem(mexf, name):
    b = mexf
    p, s = both(b, name, **SOLVE)
    with s:
        b.call(0, "iterate", Ref("h"), mx(5.0))
        s.run(5)
        p2 = dataclasses.replace(p, x0=0.9 * p.x0, Q=1.25 * p.Q, A=p.A * (1.0 - 1e-3), q=None if p.q is None else 0.5 * p.q)
        r = b.call(0, "update", Ref("h"), matlab_problem(p2))
        assert r.rc == 0 and r.warnings == [], r.error_text
        s.update_problem(p2)
        same_state(b, p, s)
        same_info(b.call(1, "solve", Ref("h")), s, s.solve())
        same_state(b, p, s)


@pytest.mark.parametrize("name", list(CASES))
def test_history_and_path_equal_the_ctypes_host(mexf, name):
    b = mexf
    p, s = both(b, name, flags=_abi.FLAG_HISTORY, **SOLVE)
    with s:
        h0 = b.call(1, "history", Ref("h")).outputs[0].data          # before any solve: no records
        assert all(v.dims == (0, 1) for v in h0.values())
        same_info(b.call(1, "solve", Ref("h")), s, s.solve())
        want = s.history()
        got = b.call(1, "history", Ref("h")).outputs[0].data
        assert list(got) == list(want) and len(want["iteration"]) > 0
        for k in want:
            assert got[k].dims == (len(want[k]), 1) and got[k].data.dtype == want[k].dtype and np.array_equal(got[k].data, want[k]), k
        path = {k: v.data[0] for k, v in b.call(1, "path", Ref("h")).outputs[0].data.items()}
        sp = s.path()
        assert len(path) == 11
        assert {k: bool(path[k]) for k in ("alternating", "alt_requested", "xfree", "auto_segments", "per_instance")} == \
               {k: sp[k] for k in ("alternating", "alt_requested", "xfree", "auto_segments", "per_instance")}
        assert _abi.KERNEL_FAMILIES[int(path["mfma"])] == sp["kernel_family"] and _abi.SCAN_FORMS[int(path["scan_form"])] == sp["scan_form"]
        assert (path["segments"], path["alt_gate"], path["scan_growth"]) == (sp["segments"], sp["alt_gate"], sp["scan_growth"])
        assert path["alt_check"] == sp["alt_check"] or (np.isnan(path["alt_check"]) and np.isnan(sp["alt_check"]))
        assert sp["per_instance"] == p.per_instance


def test_the_fall_back_warning_arrives_once(mexf):
    """The singular-A_k problem of test_gpu_alternating: setup leaves the alternating kernels and says so -- once, at setup."""
    b = mexf
    p = pkg.random_ltv(N=12, n=3, m=2, batch=5, seed=77, with_q=False)
    A = np.array(p.A)
    A[5] = np.diag([1.0, 0.0, 0.5])
    p = dataclasses.replace(p, A=A)
    opt = dict(rho=0.3, segments=3)
    r = b.call(1, "setup", matlab_problem(p), {k: mx(float(v)) for k, v in opt.items()}, save="h")
    assert r.rc == 0 and len(r.warnings) == 1
    assert r.warnings[0][0] == "admm:path" and "forward-elimination" in r.warnings[0][1]
    with pytest.warns(RuntimeWarning, match="forward-elimination"):
        s = pkg.Solver(p, pkg.Options(**opt))
    with s:
        assert r.warnings[0][1] == s.last_warning
        later = []
        for nlhs, args in ((0, ("iterate", Ref("h"), mx(9.0))), (3, ("get", Ref("h"))), (1, ("path", Ref("h"))),
                           (1, ("history", Ref("h"))), (0, ("iterate", Ref("h"), mx(1.0)))):
            rr = b.call(nlhs, *args)
            assert rr.rc == 0
            later += rr.warnings
        assert later == []
        s.run(10)
        same_state(b, p, s)
        path = b.call(1, "path", Ref("h")).outputs[0].data
        assert path["alternating"].data[0] == 0 and path["alt_requested"].data[0] == 1


def test_a_library_refusal_arrives_as_admm_library(mexf):
    b = mexf
    p = pkg.random_ltv(N=8, n=11, m=5, batch=3, seed=1)          # (11, 5) is not compiled
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(p, pkg.Options(rho=0.3))
    text = str(e.value).split(": ", 1)[1]
    r = b.call(1, "setup", matlab_problem(p), {"rho": mx(0.3)})
    assert (r.rc, r.error_id) == (1, "admm:library") and r.outputs == [] and r.warnings == []
    assert text in r.error_text and "supported:" in r.error_text and f"error {e.value.code}" in r.error_text
    assert b.live() == 0
    assert b.call(1, "get", mx(1, "uint64")).error_id == "admm:input"          # no handle came of it


def test_the_at_exit_hook_frees_live_handles_and_returns(mexf):
    b = mexf
    for k, name in enumerate(("cw", "pinst", "fuel")):
        make, opt = CASES[name]
        assert b.call(1, "setup", matlab_problem(make()), {k2: mx(float(v)) for k2, v in opt.items()}, save=f"h{k}").rc == 0
    assert b.call(0, "free", Ref("h1")).rc == 0
    assert b.fire_at_exit() == 1
    for k in range(3):
        r = b.call(1, "get", Ref(f"h{k}"))
        assert (r.rc, r.error_id) == (1, "admm:input")
    make, opt = CASES["cw"]                                       # and the gateway still works afterwards
    assert b.call(1, "setup", matlab_problem(make()), {k2: mx(float(v)) for k2, v in opt.items()}, save="h").rc == 0
    assert b.call(0, "iterate", Ref("h"), mx(3.0)).rc == 0
