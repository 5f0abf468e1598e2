"""The set-up refusals of the z-update extensions (scenario consensus, soft box, half-spaces) and of the fuel term,
without a GPU: every refusal returns before a device is asked for, with its status and its message -- compared here for EQUALITY
with the sentence written out, so that folding the extensions' shared rules into one place cannot reword one of them.  The order of
the checks is behaviour too: the first failing one decides the message."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import admm_library_amd as pkg
from admm_library_amd import _abi

INVALID, UNSUPPORTED = 1, 2
INF = np.inf
N, n, m, BATCH = 8, 6, 3, 4
MODES = (_abi.PRECISION_MIXED, _abi.PRECISION_FP64_MFMA)        # 1, 2: the number is part of the message

MFMA = "not supported by the MFMA forms (use ADMM_PRECISION_FP64)"


@pytest.fixture(scope="module")
def cases():
    """Problems of one shape: `box` (control box, open states), `open_u` (control rows open too: a fuel weight is allowed), `thrust`
    (thrust ball on most stages), `inst` (per-instance dynamics: time_varying = 2); marshalled once, kept alive by the dict."""
    box = pkg.random_ltv(N=N, n=n, m=m, batch=BATCH, seed=3, state_bounds=False)
    open_u = dataclasses.replace(box, lo=box.lo.copy(), hi=box.hi.copy())
    open_u.lo[:, :m], open_u.hi[:, :m] = -INF, INF
    thrust = pkg.random_ltv(N=N, n=n, m=m, batch=BATCH, seed=3, state_bounds=False, thrust_norm=True)
    inst = pkg.random_instances(N=N, n=n, m=m, batch=BATCH, seed=3)
    out = {}
    for name, p in (("box", box), ("open_u", open_u), ("thrust", thrust), ("inst", inst)):
        out[name] = (p,) + _abi.marshal_problem(p)
    return out


def opt_of(mode):
    return _abi.make_options(rho=0.3, precision_mode=mode)


def call(lib, fn, cp, opt, *args):
    h = C.c_void_p()
    rc = getattr(lib, fn)(C.byref(h), C.byref(cp), None if opt is None else C.byref(opt), *args)
    assert not h.value, fn
    return rc, lib.admm_last_error().decode()


def test_consensus_refusals(lib, cases):
    def setup(case, G, opt=None, fuel=None):
        return call(lib, "admm_setup_consensus", cases[case][1], opt, _abi.dptr(fuel), G)

    fn = "admm_setup_consensus: "
    for G in (0, -3):
        assert setup("box", G) == (INVALID, fn + f"group_size {G} must be >= 1 and divide batch")
    assert setup("box", 3) == (INVALID, fn + "group_size 3 must be >= 1 and divide batch = 4")
    # the order: the group size is reported before the shared rules ...
    assert setup("inst", 3) == (INVALID, fn + "group_size 3 must be >= 1 and divide batch = 4")
    assert setup("box", 3, opt_of(1)) == (INVALID, fn + "group_size 3 must be >= 1 and divide batch = 4")
    assert setup("inst", 2) == (UNSUPPORTED, fn + "scenario consensus needs batch-shared dynamics (time_varying = 0 or 1)")
    for mode in MODES:
        assert setup("box", 2, opt_of(mode)) == (UNSUPPORTED, fn + f"precision_mode {mode}: scenario consensus is {MFMA}")
    # ... and the shared rules before the width of the group projection
    wide = pkg.random_ltv(N=4, n=8, m=7, batch=4, seed=1)
    cw, keep = _abi.marshal_problem(wide)
    lds = "exceeds 6 control rows (the LDS arrays of the group projection are sized for the compiled shapes)"
    assert call(lib, "admm_setup_consensus", cw, None, None, 2) == (UNSUPPORTED, fn + "m = 7 " + lds)
    assert call(lib, "admm_setup_consensus", cw, opt_of(2), None, 2) == \
        (UNSUPPORTED, fn + f"precision_mode 2: scenario consensus is {MFMA}")
    # the fuel term's checks come first, without a prefix
    assert setup("box", 2, fuel=np.full(N, 0.1)) == (INVALID, "control rows must be unbounded (-inf, inf) where fuel is positive")


def test_soft_refusals(lib, cases):
    def setup(case, soft, opt=None, fuel=None):
        return call(lib, "admm_setup_soft", cases[case][1], opt, _abi.dptr(fuel), _abi.dptr(soft))

    fn = "admm_setup_soft: "
    hard = np.full((N, n + m), INF)
    neg = hard.copy()
    neg[2, 4] = -1.0
    assert setup("box", None) == (INVALID, fn + "soft must not be NULL (admm_setup / admm_setup_fuel set up a handle without weights)")
    assert setup("inst", hard) == (UNSUPPORTED, fn + "soft constraints need batch-shared dynamics (time_varying = 0 or 1)")
    for mode in MODES:
        assert setup("box", hard, opt_of(mode)) == (UNSUPPORTED, fn + f"precision_mode {mode}: soft constraints are {MFMA}")
        assert setup("box", neg, opt_of(mode)) == (UNSUPPORTED, fn + f"precision_mode {mode}: soft constraints are {MFMA}")
    # the order: the shared rules before the weights are read
    assert setup("inst", neg) == (UNSUPPORTED, fn + "soft constraints need batch-shared dynamics (time_varying = 0 or 1)")
    for bad in (-1.0, np.nan, -INF):
        sw = hard.copy()
        sw[2, 4] = bad
        assert setup("box", sw) == (INVALID, "soft entries must be >= 0 (+inf = a hard row) and not NaN")
    ctl = "soft entries of the control rows must be +inf where unorm is finite or fuel is positive"
    k = int(np.nonzero(np.isfinite(cases["thrust"][0].unorm))[0][0])
    sw = hard.copy()
    sw[k, 0] = 1.0
    assert setup("thrust", sw) == (INVALID, ctl)
    fuel = np.zeros(N)
    fuel[5] = 0.2
    sw = hard.copy()
    sw[5, 1] = 0.0
    assert setup("open_u", sw, fuel=fuel) == (INVALID, ctl)
    fuel[5] = -0.2                                # the fuel term's checks come first
    assert setup("open_u", sw, fuel=fuel) == (INVALID, "fuel entries must be finite and >= 0")


def test_halfspace_refusals(lib, cases):
    rng = np.random.default_rng(5)
    nh = 3
    a, b = rng.standard_normal((BATCH, N, nh)), rng.standard_normal((BATCH, N))

    def setup(case, a_, b_, nh_=nh, per=1, opt=None, fuel=None):
        return call(lib, "admm_setup_halfspace", cases[case][1], opt, _abi.dptr(fuel), _abi.dptr(a_), _abi.dptr(b_), nh_, per)

    fn = "admm_setup_halfspace: "
    null = fn + "a and b must not be NULL (admm_setup / admm_setup_fuel set up a handle without half-spaces)"
    assert setup("box", None, b) == (INVALID, null) and setup("box", a, None) == (INVALID, null)
    for bad in (0, -1):
        assert setup("box", a, b, nh_=bad) == (INVALID, fn + f"nh = {bad} must lie in 1 .. n")
    assert setup("box", a, b, nh_=7) == (INVALID, fn + "nh = 7 must lie in 1 .. n = 6")
    assert setup("inst", a, b) == (UNSUPPORTED, fn + "half-spaces need batch-shared dynamics (time_varying = 0 or 1)")
    for mode in MODES:
        assert setup("box", a, b, opt=opt_of(mode)) == (UNSUPPORTED, fn + f"precision_mode {mode}: half-spaces are {MFMA}")
    # the order: the shared rules before nh against n and before the planes are read
    assert setup("inst", a, b, nh_=7) == (UNSUPPORTED, fn + "half-spaces need batch-shared dynamics (time_varying = 0 or 1)")
    assert setup("box", a, b, nh_=7, opt=opt_of(2)) == (UNSUPPORTED, fn + f"precision_mode 2: half-spaces are {MFMA}")
    for which in (0, 1):
        for bad in (np.nan, INF):
            aa, bb = a.copy(), b.copy()
            (aa if which == 0 else bb).reshape(-1)[7] = bad
            assert setup("box", aa, bb) == (INVALID, fn + "non-finite entry in a or b")
    aa = a.copy()
    aa[2, 3] = (1e-170, 0.0, 0.0)
    assert setup("box", aa, b) == (INVALID, fn + "a'a of stage 3 is not a normal number (scale the row)")
    closed = cases["box"][0]
    closed = dataclasses.replace(closed, lo=closed.lo.copy())
    closed.lo[1, m + 1] = -2.0
    cc, keep = _abi.marshal_problem(closed)
    box_msg = fn + "state rows 0 .. nh - 1 must be unbounded (-inf, inf) at a stage with a half-space (stage 1)"
    assert call(lib, "admm_setup_halfspace", cc, None, None, _abi.dptr(a), _abi.dptr(b), nh, 1) == (INVALID, box_msg)
    a0, b0 = np.ascontiguousarray(a[0]), np.ascontiguousarray(b[0])
    assert call(lib, "admm_setup_halfspace", cc, None, None, _abi.dptr(a0), _abi.dptr(b0), nh, 0) == (INVALID, box_msg)
    # the fuel term's checks come first, without a prefix
    assert setup("box", a, b, fuel=np.full(N, np.nan)) == (INVALID, "fuel entries must be finite and >= 0")


def test_fuel_refusals(lib, cases):
    """The fuel term composes with every kind; its messages carry no function prefix.  (Its fourth sentence, about time-sharded
    handles, cannot be reached through the C interface: admm_setup_timeshard takes no weights.  The Python wrapper says it.)"""
    def setup(case, fuel, opt=None):
        return call(lib, "admm_setup_fuel", cases[case][1], opt, _abi.dptr(fuel))

    assert setup("inst", np.zeros(N)) == (UNSUPPORTED, "a fuel term needs batch-shared dynamics (time_varying = 0 or 1)")
    for mode in MODES:
        assert setup("open_u", np.full(N, 0.1), opt_of(mode)) == \
            (UNSUPPORTED, f"precision_mode {mode}: a fuel term is {MFMA}")
    for bad in (-1.0, np.nan, INF):
        fuel = np.zeros(N)
        fuel[6] = bad
        assert setup("open_u", fuel) == (INVALID, "fuel entries must be finite and >= 0")
    assert setup("box", np.full(N, 0.1)) == (INVALID, "control rows must be unbounded (-inf, inf) where fuel is positive")
    # the order: the weights are read before the dynamics and the precision mode are looked at
    assert setup("open_u", np.full(N, -1.0), opt_of(1)) == (INVALID, "fuel entries must be finite and >= 0")
