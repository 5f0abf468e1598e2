"""Shared harness of the time-shard tests (admm_setup_timeshard): several 'ranks' as THREADS of one process with a
hand-written all-gather (barrier + device-to-device copies), the case table of tests/test_gpu_timeshard_ranks.py -- which the host
suite reads as well (tests/test_shapes.py: every case stays inside the conditioning bound) -- and the oracle chain the state
changes of a handle are compared with.  Nothing here needs a GPU to be imported."""
import collections
import threading
import time

import numpy as np

import admm_library_amd as pkg
import oracle_c as oc
from admm_library_amd import _abi
from admm_library_amd.solver import Options, Solver

SENTINEL = -3.0e77           # what read_into() pre-fills the caller's arrays with: no iterate of any case comes near it
BARRIER_TIMEOUT = 20.0       # seconds a rank of run_ranks waits for its peers inside an exchange
JOIN_TIMEOUT = 120.0         # seconds run_ranks waits for all rank threads together


class ThreadExchange:
    """`world` 'ranks' in one process: each handle's exchange publishes its buffer, waits for the peers, copies the peers' slices."""

    def __init__(self, world, timeout=60):
        self.world = world
        self.timeout = timeout
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.calls = 0

    def make(self, rank):
        import torch

        def fn(ctx, stream, op, buf, count):
            try:
                ext = torch.cuda.ExternalStream(stream, device="cuda:0")
                ext.synchronize()                                     # my slice is complete
                self.slots[rank] = (buf, count)
                self.barrier.wait(timeout=self.timeout)
                full = pkg.device_tensor(buf, count * self.world, "cuda:0")
                with torch.cuda.stream(ext):
                    for r in range(self.world):
                        if r != rank:
                            pb, pc = self.slots[r]
                            assert pc == count
                            peer = pkg.device_tensor(pb, count * self.world, "cuda:0")
                            full[r * count:(r + 1) * count].copy_(peer[r * count:(r + 1) * count])
                ext.synchronize()
                self.barrier.wait(timeout=self.timeout)               # nobody overwrites a buffer a peer is still reading
                if rank == 0:
                    self.calls += 1
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                self.barrier.abort()
                return 1
        return _abi.EXCHANGE_FN(fn)


RankRun = collections.namedtuple("RankRun", "outs wins calls paths")


def run_ranks(p, opts, world, script):
    """`world` time shards of p (Options(**opts)) set up on the calling thread; script(solver, rank) on one thread per rank.  Every
    script makes the same sequence of collective calls (run, iterate, solve); set_rho, update_problem, update_instances, set_state
    and get are local.  Returns RankRun(what each rank's script returned, each rank's window(), exchanges counted on rank 0, each
    rank's path()); the first exception of any rank is raised again, after every handle has been closed."""
    ex = ThreadExchange(world, timeout=BARRIER_TIMEOUT)
    fns = [ex.make(r) for r in range(world)]
    solvers = []
    try:
        for r in range(world):
            solvers.append(Solver(p, Options(**opts), timeshard=(r, world, fns[r])))
        wins = [s.window() for s in solvers]
        paths = [s.path() for s in solvers]
        outs, errs, lock = [None] * world, [], threading.Lock()

        def work(r):
            try:
                outs[r] = script(solvers[r], r)
            except BaseException as e:                   # noqa: BLE001
                with lock:
                    errs.append((r, e))
                ex.barrier.abort()                       # the peers leave their exchange with an error instead of waiting

        th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
        for t in th:
            t.start()
        t0 = time.monotonic()
        for t in th:
            t.join(max(0.0, JOIN_TIMEOUT - (time.monotonic() - t0)))
        alive = [r for r, t in enumerate(th) if t.is_alive()]
        if alive:
            ex.barrier.abort()
            solvers = []                                 # (a handle a stuck thread is inside is not freed under it)
            raise AssertionError(f"ranks {alive} still running after {JOIN_TIMEOUT:.0f} s")
    finally:
        for s in solvers:
            s.close()
    if errs:
        raise errs[0][1]
    return RankRun(outs, wins, ex.calls, paths)


def assemble(outs, wins, nb):
    """outs[r] = the (batch, L) arrays rank r read (w, z, y, ...): the full arrays, rows [stage_lo * nb, stage_hi * nb) from rank r."""
    full = [np.full_like(a, np.nan) for a in outs[0]]
    for o, win in zip(outs, wins):
        lo, hi = win["stage_lo"] * nb, win["stage_hi"] * nb
        for f, a in zip(full, o):
            f[:, lo:hi] = a[:, lo:hi]
    return full


def read_into(solver, fill=SENTINEL):
    """admm_get into arrays pre-filled with `fill`: (w, z, y).  What the call leaves alone still holds `fill`."""
    outs = [np.full((solver.batch, solver.L), fill) for _ in range(3)]
    rc = solver._lib.admm_get(solver._h, *[_abi.dptr(o) for o in outs])
    assert rc == 0, solver._lib.admm_last_error().decode()
    return tuple(outs)


def outside_window(a, win, nb):
    """The columns of a (batch, L) array that are NOT rows of the window."""
    return np.concatenate([a[:, :win["stage_lo"] * nb], a[:, win["stage_hi"] * nb:]], axis=1)


def inside_window(a, win, nb):
    return a[:, win["stage_lo"] * nb:win["stage_hi"] * nb]


class OracleChain:
    """The host-side twin of a handle's life: every leg is one oracle_c.solve warm-started (z0, y0) from the state the previous
    leg left, with the handle's rho, alpha and problem at that time."""

    def __init__(self, p, rho, alpha=1.0):
        self.p, self.rho, self.alpha = p, rho, alpha
        self.w = self.z = self.y = self.r = self.s = None

    def run(self, iters):
        """`iters` iterations; r, s are the last iteration's."""
        ref = oc.solve(self.p, rho=self.rho, alpha=self.alpha, max_iter=iters, check_interval=iters, stop=False, z0=self.z, y0=self.y)
        self.w, self.z, self.y, self.r, self.s = ref["w"], ref["z"], ref["y"], ref["r"], ref["s"]
        return self

    def set_state(self, z=None, y=None):
        B, L = self.p.batch, self.p.L
        self.z = (np.zeros((B, L)) if self.z is None else self.z) if z is None else np.array(z, np.float64)
        self.y = (np.zeros((B, L)) if self.y is None else self.y) if y is None else np.array(y, np.float64)
        return self

    def set_rho(self, rho):
        """admm_set_rho: refactor, y *= rho_old / rho_new (the multiplier rho y is kept)."""
        self.set_state()
        self.y = self.y * (self.rho / rho)
        self.rho = rho
        return self

    def set_problem(self, p):
        self.p = p
        return self

    def solve(self, **kw):
        ref = oc.solve(self.p, rho=self.rho, alpha=self.alpha, z0=self.z, y0=self.y, **kw)
        self.w, self.z, self.y, self.r, self.s, self.rho = ref["w"], ref["z"], ref["y"], ref["r"], ref["s"], ref["rho"]
        return ref


# ---- the cases of tests/test_gpu_timeshard_ranks.py --------------------------------------------------------------------------------
# make() -> Problem; opts: Options fields (alpha is the test's); world: ranks; alternating: the path the handles take (asserted on
# every rank: True = the forward-elimination probe passes and the alternating kernels run, False = the plain fused path);
# uneven: the windows of the ranks differ in length (asserted, with the tiling and an interior rank)
Case = collections.namedtuple("Case", "make opts world alternating uneven")

LTV_SEED = 77


def _ltv(batch):
    return lambda: pkg.random_ltv(N=61, n=6, m=3, batch=batch, seed=LTV_SEED)


CASES = {
    "A": Case(lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=6), 3, True, True),
    "B": Case(lambda: pkg.cw_rendezvous(N=50, batch=70), dict(rho=0.05, segments=6, flags=_abi.FLAG_NO_ALTERNATE), 3, False, True),
    "C": Case(_ltv(5), dict(rho=0.3, segments=8), 4, True, True),            # pitch 64: the fp64 MFMA form with a linear term
    "C1": Case(_ltv(67), dict(rho=0.3, segments=8), 4, True, True),          # (C' of the issue) one-lane kernels
    "D": Case(lambda: pkg.cw_formation(N=64, batch=40), dict(rho=0.05, segments=8), 4, True, False),
    "E": Case(lambda: pkg.cw_rendezvous(N=50, batch=20, thrust_norm=True), dict(rho=0.05, segments=6), 3, True, True),
    "F1": Case(lambda: pkg.cw_rendezvous(N=50, batch=1), dict(rho=0.05, segments=6), 3, True, True),     # matrix-vector scan, NC = 1
    "F2": Case(lambda: pkg.cw_rendezvous(N=50, batch=2), dict(rho=0.05, segments=6), 3, True, True),     # NC = 2
    "F3": Case(lambda: pkg.cw_rendezvous(N=50, batch=3), dict(rho=0.05, segments=6), 3, True, True),     # NC = 4
    "G": Case(lambda: pkg.cw_rendezvous(N=30, batch=9), dict(rho=0.05, segments=3), 3, True, False),     # one segment per rank
    "H": Case(lambda: pkg.cw_rendezvous(N=12, batch=9), dict(rho=0.05, segments=6), 3, True, False),     # two-stage segments
    "I": Case(lambda: pkg.cw_rendezvous(N=120, batch=70), dict(rho=0.05, segments=0), 3, True, False),   # automatic segment count
}
ALPHAS = (1.0, 1.6)
RHO_FACTOR = 3.0                       # test_set_rho_mid_run moves a handle to RHO_FACTOR * rho and back
UPDATE_CASES = ("A", "C1", "E")        # the cases whose handles are moved to second_problem() by admm_update_problem
LTV_SEED2 = 78
# test_adaptive_solve_on_three_ranks: the first rho and the iteration budget per case (eps 1e-6, check_interval 10, adapt_interval
# 20, alpha 1.6).  The rule doubles rho four times from either start (the oracle, asserted there); A ends at its budget with a
# part of the batch converged, C1 converges.  ADAPT_DOUBLINGS bounds the rho values the host suite checks the growth bound at.
ADAPT = {"A": dict(rho=0.05, max_iter=300), "C1": dict(rho=0.04, max_iter=600)}
ADAPT_DOUBLINGS = 5


def second_problem(p):
    """A problem of p's shape with other dynamics, box, thrust bounds, x0 and q (where p has one): what admm_update_problem moves a
    handle to.  A thrust bound becomes PER STAGE (every stage another radius), so that a stage offset lost on a windowed handle
    shows."""
    import dataclasses
    if p.q is not None:                                                       # the random LTV cases
        return pkg.random_ltv(N=p.N, n=p.n, m=p.m, batch=p.batch, seed=LTV_SEED2)
    assert (p.n, p.m) == (6, 3)
    A, B = pkg.problems.cw_matrices(1.15 * 2.0 * np.pi / p.N)
    rng = np.random.default_rng(5)
    x0 = p.x0 * rng.uniform(0.5, 1.2, p.x0.shape)
    if p.unorm is not None:
        unorm = 0.12 + 0.1 * rng.uniform(0.0, 1.0, p.N)
        return dataclasses.replace(p, A=A, B=B, x0=x0, lo=np.full((p.N, p.nb), -np.inf), hi=np.full((p.N, p.nb), np.inf), unorm=unorm)
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[:p.m], hi[:p.m] = -0.13, 0.16
    return dataclasses.replace(p, A=A, B=B, x0=x0, lo=lo, hi=hi)


def host_scan_timeshard(p, rho, segments, ranks):
    """admm_host_scan_matrices_timeshard: (W, WB, ok) -- the dense scan matrices with their input columns rank by rank."""
    import ctypes as C
    lib = pkg.load_library()
    cp, keep = _abi.marshal_problem(p)
    M, Mt, K = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.admm_host_scan_matrix(C.byref(cp), float(rho), int(segments), None, C.byref(M), C.byref(Mt), C.byref(K)) == 0
    W, WB, ok = np.zeros((M.value, K.value)), np.zeros((M.value, K.value)), C.c_int32()
    rc = lib.admm_host_scan_matrices_timeshard(C.byref(cp), float(rho), int(segments), int(ranks), _abi.dptr(W), _abi.dptr(WB), C.byref(ok))
    assert rc == 0, lib.admm_last_error().decode()
    del keep
    return W, WB, bool(ok.value)


def host_segments(case):
    """The total segment count a case's handles run with, without a GPU: options.segments, or -- automatic, case I -- what
    admm_setup_timeshard's rule gives on a 256-CU device for a batch of up to 256 QPs (one column block)."""
    S = case.opts["segments"]
    if S:
        return S
    p = case.make()
    assert p.batch <= 256 and p.N >= 16
    per_rank = min(256, p.N // 8, 64)                                    # CUs per column block, stages per segment, the cap
    return max(1, min(per_rank, (p.N // 8) // case.world)) * case.world
