"""Every device allocation made for a handle is recorded in the handle and freed with it.

The library counts the live handle-owned device allocations of the process and their bytes (admm_debug_handle_memory: an internal
export, read here through the raw ctypes library; free-memory queries cannot serve, other processes allocate on the same GPU).  For
every kind of handle -- each takes another path through the allocation code -- the count and the bytes rise at set-up, never fall
while the handle is alive and its calls allocate their lazy buffers, and return EXACTLY to their values before set-up at close();
a set-up that is refused, before or after its allocations, leaves them where they were.

Not covered here, by reading only: a FAILED allocation (nothing in this file exhausts memory), and the label of the
check_record_alloc messages at set-up ("admm_setup, recFE"), which no problem reaches -- the check passes whenever the set-up
allocated the array it checks."""
import ctypes as C
import dataclasses
import gc
import warnings

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi

import _timeshard
import test_gpu_consensus
import test_gpu_fuel
import test_gpu_soft

pytestmark = pytest.mark.gpu


def _counter():
    """(live allocations, bytes)"""
    fn = pkg.load_library().admm_debug_handle_memory
    fn.restype, fn.argtypes = None, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    count, nbytes = C.c_int64(-1), C.c_int64(-1)
    fn(C.byref(count), C.byref(nbytes))
    return count.value, nbytes.value


class _Watch:
    """The counter around one handle: step() after every call asserts that neither figure fell and returns the new reading."""

    def __init__(self):
        gc.collect()                       # (a solver some earlier test dropped without close() is freed now, not under the watch)
        self.start = self.last = _counter()

    def step(self, what):
        now = _counter()
        assert now[0] >= self.last[0] and now[1] >= self.last[1], (what, self.last, now)
        self.last = now
        return now

    def opened(self):
        now = self.step("set-up")
        assert now[0] > self.start[0] and now[1] > self.start[1], (self.start, now)

    def closed(self):
        assert _counter() == self.start, (self.start, _counter())


def _rendezvous_calls(s, w, monkeypatch):
    p = s.problem
    s.iterate(3)
    w.step("iterate")
    s.get()
    w.step("get")
    s.certificate(costates=True)
    w.step("certificate")
    s.infeasibility(costates=True)
    w.step("infeasibility")
    # two steps with a growing chunk count: the edge buffer [3 arrays][chunks - 1][nb][pitch] is freed and allocated again
    monkeypatch.setenv("ADMM_MPC_CHUNKS", "2")
    s.mpc_advance()
    first = w.step("mpc_advance, 2 chunks")
    monkeypatch.setenv("ADMM_MPC_CHUNKS", "5")
    s.mpc_advance()
    second = w.step("mpc_advance, 5 chunks")
    monkeypatch.delenv("ADMM_MPC_CHUNKS")
    assert second[0] == first[0] and second[1] - first[1] == 3 * ((5 - 1) - (2 - 1)) * p.nb * 64 * 8, (first, second)
    s.set_rho(0.1)
    w.step("set_rho")
    s.update_problem(_timeshard.second_problem(p))
    w.step("update_problem")


def _pinst_calls(s, w, monkeypatch):
    s.iterate(2)
    s.set_rho(0.5)                                                     # trial K / S, verdict arrays
    w.step("set_rho")
    s.update_problem(pkg.random_instances(N=10, n=6, m=3, batch=4, seed=2))     # trial A / B / weights, pointer swaps
    w.step("update_problem")
    s.set_rho(0.3)
    w.step("set_rho back")


def _soft_calls(s, w, monkeypatch):
    s.iterate(2)
    s.soft_report()
    w.step("soft_report")


def _consensus_calls(s, w, monkeypatch):
    s.iterate(2)
    s.consensus()
    w.step("consensus")


def _fuel_case():
    p, rho = test_gpu_fuel.make_case((3, 1), 4, "scalar_bounded", False)
    return p, dict(rho=rho, segments=test_gpu_fuel.SWEEP_SEGMENTS)


def _first_two(made):
    return made[0], made[1]


KINDS = {
    # name: (problem and options, calls while alive)
    "default": (lambda: (pkg.cw_rendezvous(N=40, batch=5), dict(rho=0.05)), _rendezvous_calls),
    "batch4_dense_scan": (lambda: (pkg.cw_rendezvous(N=40, batch=4), dict(rho=0.05)), None),
    "batch130_no_mfma": (lambda: (pkg.cw_rendezvous(N=40, batch=130), dict(rho=0.05)), None),
    "mixed_6_3": (lambda: (pkg.cw_rendezvous(N=40, batch=5), dict(rho=0.05, precision_mode=_abi.PRECISION_MIXED)), None),
    "unfused": (lambda: (pkg.cw_rendezvous(N=40, batch=5), dict(rho=0.05, flags=_abi.FLAG_UNFUSED)), None),
    "fuel": (_fuel_case, None),
    "soft": (lambda: _first_two(test_gpu_soft.make_problem("noresid", 4, 2, 1, False)), _soft_calls),
    "consensus": (lambda: _first_two(test_gpu_consensus.make_problem("noresid", 4, 2, 2, 3, False)), _consensus_calls),
    "pinst_6_3_segments": (lambda: (pkg.random_instances(N=10, n=6, m=3, batch=4, seed=1), dict(rho=0.3, segments=2)), _pinst_calls),
    "pinst_12_6_tiled": (lambda: (pkg.random_instances(N=10, n=12, m=6, batch=4, seed=55), dict(rho=0.3)), None),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_handle_frees_what_it_allocated(gpu, kind, monkeypatch):
    make, calls = KINDS[kind]
    p, opts = make()
    w = _Watch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the kernel path is not this file's subject)
        s = pkg.Solver(p, pkg.Options(**opts))
    with s:
        w.opened()
        if kind == "batch4_dense_scan":
            assert s.path()["scan_form"] == "matrix_vector"
        if kind == "mixed_6_3":
            assert s.path()["kernel_family"] == "mfma_mixed"
        if kind == "pinst_6_3_segments":
            assert s.geometry()["segments"] == 2 and p.per_instance_bounds
        if calls:
            calls(s, w, monkeypatch)
    w.closed()


def test_two_time_shard_ranks_free_their_windows(gpu):
    """Windowed arrays: the handle's fields hold them biased by the window's first row, the record holds the allocation itself."""
    p = pkg.cw_rendezvous(N=30, batch=9)
    w = _Watch()

    def script(s, rank):
        return _counter(), s.window()

    run = _timeshard.run_ranks(p, dict(rho=0.05, segments=4), 2, script)
    for (count, nbytes), win in run.outs:
        assert count > w.start[0] and nbytes > w.start[1]
        assert (win["stage_lo"], win["stage_hi"]) != (0, p.N)                 # a window, so biased pointers
    assert run.wins[1]["stage_lo"] > 0
    w.closed()


def _indefinite():
    p = pkg.random_instances(N=10, n=6, m=3, batch=4, seed=1)
    return dataclasses.replace(p, R=-0.5 * np.eye(3)), dict(rho=0.3)


@pytest.mark.parametrize("make,status", [
    (_indefinite, "ADMM_ERR_NUMERIC"),               # refused by the device factorisation, after every buffer exists
    (lambda: (pkg.random_instances(N=10, n=6, m=3, batch=4, seed=1), dict(rho=0.3, precision_mode=_abi.PRECISION_MIXED)),
     "ADMM_ERR_UNSUPPORTED"),                        # refused before any device allocation
], ids=["after_allocations", "before_allocations"])
def test_a_refused_setup_frees_what_it_allocated(gpu, make, status):
    p, opts = make()
    w = _Watch()
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(p, pkg.Options(**opts))
    assert e.value.code == {v: k for k, v in _abi.STATUS_NAMES.items()}[status] and str(e.value)
    w.closed()


def test_setup_warns_once_about_the_gate(gpu):
    """A problem whose forward-elimination form fails its host check (tests/test_gpu_guards.py): set-up uploads its factor through
    the routine of the refactors, and still says so once, as admm_setup."""
    p = pkg.random_ltv(N=40, n=6, m=1, batch=2, seed=5)
    w = _Watch()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        s = pkg.Solver(p, pkg.Options(rho=0.05, segments=4))
    with s:
        gate = [r for r in rec if issubclass(r.category, RuntimeWarning) and "forward-elimination" in str(r.message)]
        assert len(gate) == 1 and str(gate[0].message) == s.last_warning
        assert s.last_warning.startswith("admm_setup: the forward-elimination form failed its host check")
        assert s.last_warning.count("forward-elimination") == 1
        assert s.path()["alt_requested"] and not s.path()["alternating"]
    w.closed()
