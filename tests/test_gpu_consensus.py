"""Scenario consensus on the GPU (csrc/admm_consensus_kernels.hpp) against tests/_consensus_ref.py -- the fuel
helper's loop with the group prox (tests/test_consensus_host.py checks that reference on the CPU and holds the solve cases).

The group sizes are chosen for the kernel's geometry (a workgroup's tile is 512 columns for m <= 3 and 256 above): groups that
start at odd columns (3, 65), a batch of 195 in a pitch of 256 (pad columns next to the last group), 650 columns (the whole
groups of a tile do not fill it: 7 x 65, 3 x 130), a group wider than a tile (600: the two-pass route), and G = 1."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded, as in tests/test_gpu_device_io.py)

import admm_library_amd as pkg
import _cert_ref
import _consensus_ref as cr
import _indep as ind
import _readout_cases as rc
import test_consensus_host as host
from admm_library_amd import _abi

pytestmark = pytest.mark.gpu
TOL = 1e-10            # x max(1, |.|): the project's iterate tolerance
INVALID, UNSUPPORTED = 1, 2
DEV = "cuda:0"
PAIRS = [(4, 2), (6, 3), (12, 6)]
GROUPS = [(2, 3), (3, 5), (64, 2), (65, 3), (130, 5), (600, 1), (1, 70)]      # (G, ngroups)
FORMS = ["noresid", "relax", "thrust", "fuel", "lti_box", "seg1", "seg4"]
RHO = 0.3


def make_problem(form, n, m, G, ngroups, with_q, seed=None):
    """(problem, options, residual_every) of a form; N between 6 and 17."""
    N = 17 if form == "seg4" else 9 if (n, m) != (12, 6) else 6
    p = pkg.random_ltv(N=N, n=n, m=m, batch=G * ngroups, seed=1000 + 16 * n + m if seed is None else seed, with_q=with_q,
                       thrust_norm=form in ("thrust", "fuel"))
    if form == "fuel":
        p = rc.stage_fuel(p)
    if form == "lti_box":
        p = rc.lti(p)
    kw = dict(rho=RHO)
    if form == "relax":
        kw["alpha"] = 1.6
    if form in ("seg1", "seg4"):
        kw["segments"] = int(form[3:])
    return dataclasses.replace(p, consensus=G), kw, (0 if form == "noresid" else 1)


def _close(a, b, tol=TOL):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


def _ref(p, kw, k, every, **more):
    return cr.solve(p, rho=kw["rho"], alpha=kw.get("alpha", 1.0), max_iter=k, check_interval=max(every, 1), eps_abs=0, eps_rel=0,
                    stop=False, **more)


def _solver(p, **kw):
    s = pkg.Solver(p, pkg.Options(**kw))
    path = s.path()
    assert not path["alternating"] and not path["alt_requested"] and path["kernel_family"] == "one_lane_fp64", path
    return s


def _equal_in_groups(p, z):
    U = z.reshape(p.batch // p.consensus, p.consensus, p.N, p.nb)[:, :, :, :p.m]
    return np.array_equal(U, np.broadcast_to(U[:, :1], U.shape))


# ---- 1. iterates against the reference ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("G,ngroups", GROUPS, ids=[f"G{g}x{k}" for g, k in GROUPS])
def test_iterates_match_the_reference(gpu, G, ngroups, form):
    for n, m in PAIRS:
        for with_q in (False, True):
            p, kw, every = make_problem(form, n, m, G, ngroups, with_q)
            with _solver(p, **kw) as s:
                if form in ("seg1", "seg4"):
                    assert s.geometry()["segments"] == kw["segments"]
                done = 0
                for k in (1, 2, 7):
                    s.run(k - done, residual_every=every)
                    done = k
                    w, z, y = s.get()
                    ref = _ref(p, kw, k, every)
                    for name, a, b in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
                        assert _close(a, b), (n, m, with_q, k, name, np.abs(a - b).max())
                    if every:
                        r, sd, *_ = s.residuals()
                        assert _close(r, ref.r) and _close(sd, ref.s), (n, m, with_q, k, np.abs(r - ref.r).max(), np.abs(sd - ref.s).max())
                    assert _equal_in_groups(p, z)


@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("form", ["relax", "fuel", "noresid"])
@pytest.mark.parametrize("G,ngroups,pair", [(600, 1, (6, 3)), (600, 2, (12, 6)), (300, 2, (12, 6)), (4500, 1, (6, 3)), (4500, 2, (4, 2))],
                         ids=["G600", "G600x2_m6", "G300x2_m6", "G4500", "G4500x2"])
def test_wide_groups_with_several_blocks_per_chunk(gpu, G, ngroups, pair, form, blocks):
    """The two-pass route (a group wider than a tile: 512 columns, 256 at m = 6) with two and three blocks per chunk: the five
    residual sums of a column continue through the partial-sum array from block to block.  4500 columns are nine tiles: the tile
    sums are carried up two levels of the tree.  The automatic chunks of these short horizons hold one block only."""
    n, m = pair
    p, kw, every = make_problem(form, n, m, G, ngroups, True)
    kw = dict(zrows=blocks * p.nb, **kw)
    with _solver(p, **kw) as s:
        assert s.geometry()["zrows"] == blocks * p.nb and s.geometry()["zchunks"] == -(-p.N // blocks)
        done = 0
        for k in (1, 2, 7):
            s.run(k - done, residual_every=every)
            done = k
            w, z, y = s.get()
            ref = _ref(p, kw, k, every)
            for name, a, b in (("w", w, ref.w), ("z", z, ref.z), ("y", y, ref.y)):
                assert _close(a, b), (k, name, np.abs(a - b).max())
            if every:
                r, sd, nw, nz, ny = s.residuals()
                assert _close(r, ref.r) and _close(sd, ref.s), (k, np.abs(r - ref.r).max(), np.abs(sd - ref.s).max())
                Z, Y = z.reshape(p.batch, -1), y.reshape(p.batch, -1)
                assert _close(nw, np.linalg.norm(w, axis=1)) and _close(nz, np.linalg.norm(Z, axis=1)) and _close(ny, kw["rho"] * np.linalg.norm(Y, axis=1))
            assert _equal_in_groups(p, z)


# ---- 2. consensus is exact ----

@pytest.mark.parametrize("G,ngroups", [(3, 5), (65, 3), (600, 1)], ids=["G3", "G65", "G600"])
@pytest.mark.parametrize("form", ["relax", "fuel"])
def test_control_rows_are_bitwise_equal_within_a_group(gpu, G, ngroups, form):
    p, kw, every = make_problem(form, 6, 3, G, ngroups, True)
    with _solver(p, **kw) as s:
        for k in (1, 4):
            s.run(k, residual_every=2)
            _, z, y = s.get()
            assert _equal_in_groups(p, z)
            ubar = s.consensus()
            assert ubar.shape == (ngroups, p.N, p.m) and np.array_equal(ubar, cr.consensus_of(p, z))
            X = z.reshape(ngroups, G, p.N, p.nb)[:, :, :, p.m:]
            assert (np.abs(X - X[:, :1]).reshape(ngroups, G, -1).max(axis=2)[:, 1:] > 0).all()       # every scenario's own states
            Y = y.reshape(ngroups, G, p.N, p.nb)[:, :, :, :p.m]
            assert (np.abs(Y - Y[:, :1]).reshape(ngroups, G, -1).max(axis=2)[:, 1:] > 0).all()       # ... and its own multipliers


# ---- 3. G = 1 is the unfused path ----

@pytest.mark.parametrize("alpha", [1.0, 1.6])
@pytest.mark.parametrize("kind", ["box", "thrust", "fuel"])
@pytest.mark.parametrize("batch", [70, 195])
def test_group_size_one_is_the_unfused_handle_bit_for_bit(gpu, batch, kind, alpha):
    """zdual_kernel (box) / zdual_soc_kernel (thrust, fuel) against the consensus kernel with G = 1, residuals included.  The
    residual sums are added chunk by chunk, so both handles get the same rows per chunk (two blocks): left to itself the
    consensus handle rounds the chunk of a box problem up to whole blocks and the plain handle does not."""
    p = pkg.random_ltv(N=9, n=6, m=3, batch=batch, seed=77, thrust_norm=kind != "box")
    if kind == "fuel":
        p = rc.stage_fuel(p)
    kw = dict(rho=RHO, alpha=alpha, zrows=2 * p.nb)
    out = []
    with pkg.Solver(p, pkg.Options(flags=_abi.FLAG_UNFUSED, **kw)) as plain, _solver(dataclasses.replace(p, consensus=1), **kw) as s:
        assert plain.geometry() == s.geometry()
        for h in (plain, s):
            h.run(9, residual_every=3)
            out.append(h.get() + tuple(h.residuals()))
    for i, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a, b), i


# ---- 4. placement independence and repeatability ----

@pytest.mark.parametrize("G", [64, 65])
def test_a_group_does_not_depend_on_its_place_in_the_batch(gpu, G):
    """Group 3 of 5 against the same group alone in a batch: one z-update from the same (w, z, y) -- the kernel alone --, then five
    whole iterations.  And two handles on the same problem agree bitwise.  (Rows per chunk and segments are given: left to
    themselves they follow the pitch -- a batch of 64 gets shorter x-update segments than one of 320 --, and another partition is
    another summation order in the residual sums and in the x-update, whatever the z kernel does.)"""
    p5, kw, _ = make_problem("relax", 6, 3, G, 5, True)
    p1 = dataclasses.replace(p5.slice(3 * G, 4 * G), consensus=G)
    kw = dict(zrows=2 * p5.nb, segments=2, **kw)
    rng = np.random.default_rng(5)
    st = [rng.standard_normal((p5.batch, p5.L)) for _ in range(3)]
    with _solver(p5, **kw) as s5, _solver(p1, **kw) as s1, _solver(p5, **kw) as twin:
        assert s5.scan_geometry()["split"] == s1.scan_geometry()["split"]
        s5.set_state(*st)
        twin.set_state(*st)
        s1.set_state(*[a[3 * G:4 * G] for a in st])
        for h in (s5, s1, twin):
            h.step_z(residuals=True)
        got5, got1, gott = (h.get() + tuple(h.residuals()) for h in (s5, s1, twin))
        for i, (a, b, c) in enumerate(zip(got5, got1, gott)):
            assert np.array_equal(a[3 * G:4 * G], b), ("step_z", i)
            assert np.array_equal(a, c), ("twin", i)
        for h in (s5, s1, twin):
            h.run(5, residual_every=2)
        got5, got1, gott = (h.get() + tuple(h.residuals()) for h in (s5, s1, twin))
        for i, (a, b, c) in enumerate(zip(got5, got1, gott)):
            assert np.array_equal(a[3 * G:4 * G], b), ("run", i)
            assert np.array_equal(a, c), ("twin run", i)


# ---- 5. pad columns ----

@pytest.mark.parametrize("form", ["relax", "fuel"])
def test_pad_columns_stay_out_of_the_means(gpu, form):
    """Batch 195 in a pitch of 256: the result equals the reference whatever finite junk set_state left in z, y, and nothing
    non-finite comes back."""
    p, kw, every = make_problem(form, 6, 3, 65, 3, True)
    rng = np.random.default_rng(9)
    z0 = 1e3 * rng.standard_normal((p.batch, p.L))
    y0 = -1e3 * rng.standard_normal((p.batch, p.L))
    with _solver(p, **kw) as s:
        assert s.geometry()["pitch"] == 256
        s.set_state(z=z0, y=y0)
        s.run(3, residual_every=1)
        w, z, y = s.get()
        res = s.residuals()
    ref = _ref(p, kw, 3, 1, z0=z0, y0=y0)
    for a in (w, z, y) + tuple(res):
        assert np.isfinite(a).all()
    assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y) and _close(res[0], ref.r) and _close(res[1], ref.s)


# ---- 6. solves ----

def test_open_states_converge_to_the_solution_of_the_group_mean(gpu):
    p = host.di_scenarios()
    with _solver(p, **host.DI_OPTS) as s:
        info = s.solve()
        ubar = s.consensus()
    assert info.status.all()
    for g in range(3):
        u_ref = ind.condensed_bvls(host.mean_problem(p, g), 0)
        assert np.abs(ubar[g].reshape(-1) - u_ref).max() < 1e-6


def test_state_boxed_scenarios_meet_the_coupled_optimality_conditions(gpu):
    """The conditions of the host test on the GPU's (z, y), at the bounds tests/test_gpu_independent.py applies to
    kkt_certificate_batch; Solver.certificate() against tests/_cert_ref.py on the scales of tests/test_gpu_cert.py."""
    p = host.boxed_scenarios()
    with _solver(p, **host.BOXED_OPTS) as s:
        info = s.solve()
        c = s.certificate(costates=True)
        _, z, y = s.get()
    assert info.status.all() and int(info.n_converged) == p.batch
    cond, n_active = cr.coupled_conditions(p, z, y, float(info.rho))
    worst = {k: float(np.max(v)) for k, v in cond.items()}
    print("iterations", info.iters_run, worst, "active", n_active)
    assert cond["spread"] == 0.0 and cond["feas_box"].max() == 0.0, worst
    assert cond["feas_dyn"].max() < 1e-6 and cond["stat"].max() < 1e-6 and cond["comp"].max() < 1e-6, worst
    on = (np.abs(z.reshape(p.batch, p.N, p.nb)[:, :, p.m]) >= host.POS_BOX[0] - 1e-9).any(axis=1)
    assert on.any() and not on.all()
    ref = _cert_ref.certificate(p, z, y, float(info.rho))
    b = p.batch
    s_nu = np.maximum(1.0, np.abs(ref["nu"]).reshape(b, -1).max(axis=1))
    s_obj, s_z = np.maximum(1.0, ref["obj_abs"]), np.maximum(1.0, np.abs(z).reshape(b, -1).max(axis=1))
    assert (np.abs(c.nu - ref["nu"]).reshape(b, -1).max(axis=1) <= TOL * s_nu).all()
    assert (np.abs(c.stat - ref["stat"]) <= TOL * s_nu).all() and (np.abs(c.obj - ref["obj"]) <= TOL * s_obj).all()
    assert (np.abs(c.feas_dyn - ref["feas_dyn"]) <= TOL * s_z).all()


def test_adaptive_rho_follows_the_reference(gpu):
    """The case whose decisions tests/test_consensus_host.py shows to be clear of the thresholds: 150 iterations, the rho of every
    stopping test equals the reference's, the iterates agree."""
    p = host.adapt_scenarios()
    dec = []
    ref = cr.solve(p, stop=False, decisions=dec, **host.ADAPT_OPTS)
    trajectory = [host.ADAPT_OPTS["rho"]] + [d[3] for d in dec]
    with _solver(p, flags=_abi.FLAG_HISTORY, **host.ADAPT_OPTS) as s:
        info = s.solve()
        w, z, y = s.get()
        hist = s.history()
    assert (info.iters_run, info.rho_updates, info.rho) == (ref.iters_run, ref.rho_updates, ref.rho)
    assert hist["iteration"].tolist() == list(range(10, 151, 10)) and hist["rho"].tolist() == trajectory
    assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)


# ---- 7. state handling ----

def test_reading_the_state_does_not_change_the_iterates(gpu):
    p, kw, _ = make_problem("fuel", 6, 3, 65, 3, True)
    with _solver(p, **kw) as a, _solver(p, **kw) as b:
        a.run(4, residual_every=2)
        a.get()
        a.consensus()
        a.certificate()
        a.run(3, residual_every=1)
        b.run(4, residual_every=2)
        b.run(3, residual_every=1)
        for x, yv in zip(a.get() + tuple(a.residuals()), b.get() + tuple(b.residuals())):
            assert np.array_equal(x, yv)


def test_set_state_update_instances_and_set_rho(gpu):
    p, kw, _ = make_problem("relax", 4, 2, 3, 5, True)
    rng = np.random.default_rng(11)
    z0, y0 = rng.standard_normal((p.batch, p.L)), 0.3 * rng.standard_normal((p.batch, p.L))
    with _solver(p, **kw) as s:
        s.set_state(z=z0, y=y0)
        s.run(4, residual_every=2)
        _, z, y = s.get()
        ref = _ref(p, kw, 4, 2, z0=z0, y0=y0)
        assert _close(z, ref.z) and _close(y, ref.y)
        # new x0 and q: the next iteration uses them
        p2 = dataclasses.replace(p, x0=-0.5 * p.x0, q=2.0 * p.q)
        s.update_instances(x0=p2.x0, q=p2.q)
        s.run(1)
        w, z, y = s.get()
        ref = _ref(p2, kw, 1, 0, z0=ref.z, y0=ref.y)
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y)
        # new rho: y is rescaled, the factor rebuilt
        rho2 = 0.8
        s.set_rho(rho2)
        s.run(3, residual_every=3)
        w, z, y = s.get()
        ref = _ref(p2, dict(kw, rho=rho2), 3, 3, z0=ref.z, y0=ref.y * (kw["rho"] / rho2))
        assert _close(w, ref.w) and _close(z, ref.z) and _close(y, ref.y) and _close(s.residuals()[0], ref.r)
        assert _equal_in_groups(p, z)


@pytest.mark.parametrize("G,ngroups", [(65, 3), (600, 1)], ids=["G65", "G600"])
def test_graph_replay_gives_the_bits_of_direct_launches(gpu, G, ngroups):
    p, kw, _ = make_problem("fuel", 6, 3, G, ngroups, True)
    out = []
    for flags in (0, _abi.FLAG_GRAPH):
        with _solver(p, flags=flags, **kw) as s:
            s.run(7, residual_every=2)
            out.append(s.get() + tuple(s.residuals()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 8. refusals ----

def test_setup_refusals(gpu):
    lib, h = pkg.load_library(), C.c_void_p()
    p = pkg.random_ltv(N=6, n=4, m=2, batch=6, seed=2)
    cp, keep = _abi.marshal_problem(p)
    for G in (0, -1, 4, 7):
        assert lib.admm_setup_consensus(C.byref(h), C.byref(cp), None, None, G) == INVALID and not h.value
        assert b"group_size" in lib.admm_last_error()
    inst = pkg.random_instances(N=6, n=4, m=2, batch=4, seed=2)
    ci, keep_i = _abi.marshal_problem(inst)
    assert lib.admm_setup_consensus(C.byref(h), C.byref(ci), None, None, 2) == UNSUPPORTED and not h.value
    assert b"batch-shared" in lib.admm_last_error()
    pc = dataclasses.replace(p, consensus=3)
    for mode in (_abi.PRECISION_MIXED, _abi.PRECISION_FP64_MFMA):
        with pytest.raises(pkg.AdmmError) as e:
            pkg.Solver(pc, pkg.Options(rho=RHO, precision_mode=mode))
        assert e.value.code == UNSUPPORTED and "precision_mode" in str(e.value) and "consensus" in str(e.value)
    with pytest.raises(pkg.AdmmError) as e:
        pkg.Solver(pc, pkg.Options(rho=RHO, segments=2), timeshard=(0, 1, None))
    assert e.value.code == UNSUPPORTED and "time-sharded" in str(e.value)
    d = pkg.DeviceProblem.from_problem(pc, DEV)
    assert d.consensus == 3
    with pytest.raises(ValueError, match="consensus"):
        pkg.Solver(d, pkg.Options(rho=RHO))
    # a handle without groups
    with pkg.Solver(p, pkg.Options(rho=RHO)) as s:
        out = np.zeros(p.batch * p.N * p.m)
        assert lib.admm_get_consensus(s._h, _abi.dptr(out)) == INVALID and b"no scenario groups" in lib.admm_last_error()
        assert lib.admm_get_consensus_device(s._h, _abi.dptr(out), None) == INVALID and b"no scenario groups" in lib.admm_last_error()
        with pytest.raises(pkg.AdmmError):
            s.consensus()
        assert not out.any()


def test_refusals_leave_the_handle_alone(gpu):
    """admm_probe_infeasibility* and admm_mpc_advance*: ADMM_ERR_UNSUPPORTED naming the reason; a following run matches a twin that
    never made the call."""
    lib = pkg.load_library()
    p, kw, _ = make_problem("relax", 6, 3, 3, 5, True)
    out = np.zeros(p.batch)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        with pytest.raises(pkg.AdmmError) as e:
            s.infeasibility(span=10, eps=1e-6)
        assert e.value.code == UNSUPPORTED and "scenario-consensus" in str(e.value)
        assert lib.admm_probe_infeasibility_device(s._h, 10, 1e-6, _abi.dptr(out), None, None, None, None, None) == UNSUPPORTED
        assert b"scenario-consensus" in lib.admm_last_error()
        with pytest.raises(pkg.AdmmError) as e:
            s.mpc_advance()
        assert e.value.code == UNSUPPORTED and "scenario-consensus" in str(e.value)
        step = _abi.CMpcStep()
        assert lib.admm_mpc_advance_device(s._h, C.byref(step), None, None, None) == UNSUPPORTED
        assert b"scenario-consensus" in lib.admm_last_error()
        assert not out.any()
        # admm_profile in a fused mode would iterate the per-QP z-update and leave the v-form behind: only the unfused mode runs
        for mode_kw in (dict(), dict(fused=True), dict(alternating=True), dict(alternating=True, back_to_back=True), dict(alternating=True, lean=True)):
            with pytest.raises(pkg.AdmmError) as e:
                s.profile(3, **mode_kw)
            assert e.value.code == UNSUPPORTED and "unfused path only" in str(e.value), (mode_kw, str(e.value))
        s.run(4, residual_every=2)
        twin.run(4, residual_every=2)
        for a, b in zip(s.get() + tuple(s.residuals()), twin.get() + tuple(twin.residuals())):
            assert np.array_equal(a, b)
        # ... and that one is four plain iterations of the handle's own kernels: consensus holds afterwards, bit for bit with the twin
        ms = s.profile(4, residuals=True, fused=False)
        assert ms["zdual_ms"] > 0
        twin.run(4, residual_every=1)
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)
        assert _equal_in_groups(p, s.get()[1])


def test_device_form_of_the_read_out(gpu):
    lib = pkg.load_library()
    p, kw, _ = make_problem("fuel", 6, 3, 65, 3, True)
    count = 3 * p.N * p.m

    def dp(t):
        return C.cast(C.c_void_p(t.data_ptr()), _abi.c_double_p)
    with _solver(p, **kw) as s, _solver(p, **kw) as twin:
        s.run(5)
        twin.run(5)
        t = torch.zeros(count + 1, dtype=torch.float64, device=DEV)
        assert lib.admm_get_consensus_device(s._h, dp(t[1:]), pkg.solver._stream(DEV)) == 0         # a view at an 8-byte offset
        torch.cuda.synchronize()
        assert np.array_equal(t[1:].cpu().numpy().reshape(3, p.N, p.m), s.consensus()) and t[0] == 0
        hostv = np.zeros(count)
        pinned = torch.zeros(count, dtype=torch.float64).pin_memory()
        for ptr in (_abi.dptr(hostv), dp(pinned)):
            assert lib.admm_get_consensus_device(s._h, ptr, None) == INVALID
            assert "admm_get_consensus_device: ubar is not device memory" in lib.admm_last_error().decode()
        assert not hostv.any() and not pinned.any()
        big = torch.zeros(3 * 2 ** 20, dtype=torch.float64, device=DEV)       # a block of its own in torch's allocator
        assert lib.admm_get_consensus_device(s._h, dp(big[big.numel() - (count - 1):]), None) == INVALID
        assert f"admm_get_consensus_device: ubar ends before its {count} doubles" in lib.admm_last_error().decode()
        torch.cuda.synchronize()
        assert (big == 0).all()
        s.run(3)
        twin.run(3)
        for a, b in zip(s.get(), twin.get()):
            assert np.array_equal(a, b)
