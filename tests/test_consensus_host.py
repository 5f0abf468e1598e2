"""Scenario consensus, the part that needs no GPU: the interface (header, exported symbols, NULL handle), and
the reference the GPU tests compare against (tests/_consensus_ref.py) -- against _fuel_ref.solve (group size 1), against SciPy's
bounded least squares on the group-mean x0 (open state rows: the consensus profile is the nominal solution of the mean), against
the optimality conditions of the coupled problem, and the margins of the adaptive-rho case the GPU test replays."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import admm_library_amd as pkg
import _consensus_ref as cr
import _fuel_ref as fr
import _indep as ind
from admm_library_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
SYMBOLS = ("admm_setup_consensus", "admm_get_consensus", "admm_get_consensus_device")


# ---- the cases the GPU tests share (tests/test_gpu_consensus.py imports them) ----

def di_scenarios():
    """double_integrator(N = 50): 3 group nominals (the generator's instances), each dispersed into 5 scenarios."""
    base = pkg.double_integrator(N=50, batch=3)
    rng = np.random.default_rng(7)
    x0 = np.repeat(base.x0, 5, axis=0) + rng.uniform(-0.5, 0.5, (15, 2))
    return dataclasses.replace(base, x0=x0, consensus=5)


# rho 10 with alpha 1.6: the scenario deviations converge at rate lambda / (lambda + rho) over the eigenvalues lambda of the
# condensed Hessian, so consensus wants a larger rho than the single QP (rho = 1: r = 2e-2 after 5000 iterations; rho = 10: 1650
# iterations to eps = 1e-10)
DI_OPTS = dict(rho=10.0, alpha=1.6, eps_abs=1e-10, eps_rel=1e-10, max_iter=20000, check_interval=10)

POS_BOX = (0.15, np.inf, np.inf)       # radial corridor: the open solution's excursion is 0.2 km, every x0 starts inside 0.1 km


def boxed_scenarios(groups=2, group_size=4):
    return pkg.cw_rendezvous_scenarios(N=12, groups=groups, group_size=group_size, spread=0.05, pos_box=POS_BOX)


BOXED_OPTS = dict(rho=100.0, alpha=1.6, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, check_interval=10)   # 2470 iterations on the CPU

# the adaptive-rho case: a rho far too large, which the rule halves eight times in 150 iterations
ADAPT_OPTS = dict(rho=3000.0, eps_abs=0.0, eps_rel=0.0, max_iter=150, check_interval=10, adapt_interval=10, adapt_max=16)


def adapt_scenarios():
    return boxed_scenarios(groups=3, group_size=5)


def mean_problem(p, g):
    """The single QP of group g's mean x0."""
    G = p.consensus
    return dataclasses.replace(p, x0=p.x0[g * G:(g + 1) * G].mean(axis=0, keepdims=True), consensus=None)


# ---- interface ----

def test_header_announces_the_symbols_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert re.search(r"^#define ADMM_HIP_HAS_CONSENSUS 1$", h, re.M)
    assert re.search(r"^#define ADMM_HIP_ABI_VERSION 9$", h, re.M)
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", h, re.M), name


def test_symbols_are_exported_and_null_handles_are_refused(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.admm_abi_version() == 9
    out = np.zeros(4)
    assert lib.admm_get_consensus(None, _abi.dptr(out)) == INVALID and b"NULL" in lib.admm_last_error()
    assert lib.admm_get_consensus_device(None, _abi.dptr(out), None) == INVALID and b"NULL" in lib.admm_last_error()
    h = C.c_void_p()
    assert lib.admm_setup_consensus(C.byref(h), None, None, None, 2) == INVALID and not h.value
    # the group size is checked before a device is looked for
    p = pkg.double_integrator(N=10, batch=6)
    cp, keep = _abi.marshal_problem(p)
    for G in (0, -3, 4):
        assert lib.admm_setup_consensus(C.byref(h), C.byref(cp), None, None, G) == INVALID and not h.value
        assert b"group_size" in lib.admm_last_error()
    # more control rows than the kernel's LDS arrays are sized for: refused, before a device is looked for
    wide = pkg.random_ltv(N=4, n=8, m=7, batch=4, seed=1)
    cw, keep_w = _abi.marshal_problem(wide)
    assert lib.admm_setup_consensus(C.byref(h), C.byref(cw), None, None, 2) == 2 and not h.value and b"control rows" in lib.admm_last_error()


def test_the_kernel_does_not_spill(tmp_path):
    """csrc/admm_consensus.hip compiled on its own with the library's flags and the compiler's resource report: the four forms of
    zdual_consensus_kernel are there and none uses scratch memory (the build's spill gate reads the reports of the (n, m) units
    only; DESIGN.md §2.12 records the registers this prints)."""
    import __graft_entry__ as ge
    assert "admm_consensus.hip" in ge.RUNTIME_UNITS and "admm_consensus_kernels.hpp" in ge.HEADERS and "admm_consensus.hpp" in ge.HEADERS
    assert "admm_consensus.hip" in ge.NO_SCRATCH_UNITS            # the build itself refuses scratch in this unit
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-Rpass-analysis=kernel-resource-usage"] + ge.HIPCC_FLAGS +
                       ["-c", os.path.join(ge.CSRC, "admm_consensus.hip"), "-o", str(tmp_path / "admm_consensus.o")],
                       cwd=ge.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = ge.parse_resource_usage(r.stderr)
    mine = [x for x in rows if "zdual_consensus_kernel" in x["name"]]
    for x in mine:
        print(f'{x["name"]}: {x["vgpr"]} VGPRs, {x["agpr"]} AGPRs, {x["sgpr"]} SGPRs, scratch {x["scratch"]} B, occupancy {x["occupancy"]}')
    assert sorted(x["name"].split("<")[1] for x in mine) == ["false, false>", "false, true>", "true, false>", "true, true>"]
    assert all(x["scratch"] == 0 and x["vgpr_spill"] == 0 for x in mine), mine
    assert all(x["occupancy"] >= 2 for x in mine), mine          # two workgroups per CU: the chunk rule of admm_setup_consensus counts on it
    assert all(x["scratch"] == 0 for x in rows), [x["name"] for x in rows if x["scratch"]]


def test_problem_validate_checks_the_group_size():
    p = pkg.double_integrator(N=10, batch=6)
    dataclasses.replace(p, consensus=3).validate()
    for G in (0, 4, 2.5):
        with pytest.raises(ValueError, match="consensus"):
            dataclasses.replace(p, consensus=G).validate()
    inst = pkg.random_instances(N=6, n=4, m=2, batch=4, seed=2)
    with pytest.raises(ValueError, match="consensus"):
        dataclasses.replace(inst, consensus=2).validate()
    s = pkg.cw_rendezvous_scenarios(N=12, groups=3, group_size=4, spread=0.1, pos_box=0.5)
    s.validate()
    assert s.consensus == 4 and s.batch == 12 and (s.hi[3:6] == 0.5).all() and np.isinf(s.hi[6:]).all()
    assert np.array_equal(pkg.cw_rendezvous_scenarios(N=12, groups=3, group_size=4, spread=0.0).x0[::4], pkg.cw_rendezvous(N=12, batch=3).x0)


# ---- the reference ----

@pytest.mark.parametrize("make,kw", [
    (lambda: fr_case("soc"), dict(rho=0.4, alpha=1.5, max_iter=40, stop=False)),
    (lambda: fr_case("fuel"), dict(rho=0.4, max_iter=60, check_interval=5, adapt_interval=10)),
    (lambda: pkg.random_ltv(N=15, n=4, m=2, batch=4, seed=8), dict(rho=0.3, max_iter=300, adapt_interval=10, check_interval=5)),
    (lambda: pkg.double_integrator(N=30, batch=3), dict(rho=1.0, alpha=1.2, max_iter=200)),
], ids=["soc_ltv", "fuel_ltv_adaptive", "box_ltv_adaptive", "box_di"])
def test_group_size_one_is_the_fuel_helper_bit_for_bit(make, kw):
    p = make()
    ref = fr.solve(p, **kw)
    got = cr.solve(p, group=1, **kw)
    assert got.iters_run == ref.iters_run and got.rho == ref.rho and got.rho_updates == ref.rho_updates
    for name in ("w", "z", "y", "r", "s", "iters", "status"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name


def fr_case(kind):
    p = pkg.random_ltv(N=23, n=6, m=3, batch=5, seed=3, thrust_norm=True)
    if kind == "fuel":
        p = dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), 0.3, 0.0))
    return p


def test_prox_is_the_projection_onto_the_coupled_set():
    """Control rows equal within a group and equal to prox(mean); state rows per QP; the group's sum of v - z on the control rows is
    G (vbar - prox(vbar)): the per-QP parts cancel."""
    rng = np.random.default_rng(3)
    N, n, m, G, ng = 4, 3, 2, 3, 2
    nb = n + m
    v = rng.standard_normal((G * ng, N * nb))
    lo, hi = np.tile(np.r_[-0.3, -0.2, -np.inf, -0.5, -np.inf], N), np.tile(np.r_[0.4, 0.1, 0.7, np.inf, np.inf], N)
    un, kap = np.full(N, np.inf), np.zeros(N)
    z = cr.prox(v, lo, hi, un, kap, m, G)
    Z, V = z.reshape(ng, G, N, nb), v.reshape(ng, G, N, nb)
    assert (Z[:, :, :, :m] == Z[:, :1, :, :m]).all()
    vbar = V[:, :, :, :m].mean(axis=1)
    lou, hiu = lo.reshape(N, nb)[:, :m], hi.reshape(N, nb)[:, :m]
    assert np.array_equal(Z[:, 0, :, :m], np.clip(vbar, lou, hiu))
    assert np.array_equal(Z[:, :, :, m:], np.clip(V[:, :, :, m:], lo.reshape(N, nb)[:, m:], hi.reshape(N, nb)[:, m:]))
    assert np.abs((V - Z)[:, :, :, :m].sum(axis=1) - G * (vbar - Z[:, 0, :, :m])).max() < 1e-14


def test_open_states_give_the_solution_of_the_group_mean():
    """double_integrator(N = 50), 3 groups x 5 dispersed x0, converged to eps = 1e-10: each group's profile equals SciPy's bounded
    least squares for the group-mean x0 within 1e-6 (the eps and tolerance of test_config0_gpu_solve_vs_scipy_bvls)."""
    p = di_scenarios()
    ref = cr.solve(p, **DI_OPTS)
    assert ref.status.all() and ref.iters_run < DI_OPTS["max_iter"]
    ubar = cr.consensus_of(p, ref.z)
    n_active = 0
    for g in range(3):
        u_ref = ind.condensed_bvls(mean_problem(p, g), 0)
        assert np.abs(ubar[g].reshape(-1) - u_ref).max() < 1e-6
        n_active += int((np.abs(np.abs(u_ref) - 1.0) < 1e-9).sum())
    assert n_active >= 10
    X = ref.z.reshape(3, 5, p.N, p.nb)[:, :, :, p.m:]
    assert np.abs(X - X[:, :1]).max() > 0.1                      # the scenarios' states differ


def test_state_boxed_scenarios_meet_the_coupled_optimality_conditions():
    p = boxed_scenarios()
    ref = cr.solve(p, **BOXED_OPTS)
    assert ref.status.all() and ref.iters_run < BOXED_OPTS["max_iter"]
    c, n_active = cr.coupled_conditions(p, ref.z, ref.y, ref.rho)
    worst = {k: float(np.max(v)) for k, v in c.items()}
    assert c["spread"] == 0.0 and c["feas_box"].max() == 0.0, worst
    assert c["feas_dyn"].max() < 1e-6 and c["stat"].max() < 1e-6 and c["comp"].max() < 1e-6, worst
    # the corridor is active on some scenario and not on all: it is the cloud that makes it bind
    on = (np.abs(ref.z.reshape(p.batch, p.N, p.nb)[:, :, p.m]) >= POS_BOX[0] - 1e-9).any(axis=1)
    assert on.any() and not on.all()
    # ... and the per-QP multipliers of the control rows are not zero inside the box: only their sum over the group is
    yu = ref.y.reshape(2, 4, p.N, p.nb)[:, :, :, :p.m]
    inside = np.abs(cr.consensus_of(p, ref.z)) < 0.2 - 1e-6
    assert inside.any() and np.abs(yu).max(axis=1)[inside].max() > 1e-4 and np.abs(yu.sum(axis=1)[inside]).max() < 1e-8


def test_adaptive_case_decides_with_a_margin():
    """At every decision of the reference R / S is further than a factor 1.5 from mu^2 and from 1 / mu^2: a last-bit difference in
    a mean cannot flip a rho decision on the GPU."""
    dec = []
    ref = cr.solve(adapt_scenarios(), stop=False, decisions=dec, **ADAPT_OPTS)
    assert len(dec) == 14 and ref.rho_updates == 8 and ref.rho == 3000.0 / 256
    assert [d[3] for d in dec][-1] == ref.rho
    for it, R, S, _ in dec:
        for edge in (100.0, 0.01):
            assert not (edge / 1.5 <= R / S <= edge * 1.5), (it, R / S)
