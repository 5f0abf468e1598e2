"""Problem setup for the batched optimal-control QPs (host side, NumPy).

The reference (README.md:1-2) names only the subject -- ADMM for astrodynamics
problems -- and ships no problem-setup code, so the generators here are this
repository's own specification.  They produce plain arrays that
are handed unchanged to the HIP solver and to the CPU oracle; neither path
generates its own inputs.

Array conventions: "QP-major" C-order arrays, shape (batch, L) etc., which is
MATLAB's column-major L x batch seen from C.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

MU_EARTH = 3.986004418e14      # m^3 / s^2
A_REF = 6_778_137.0            # m, circular reference orbit radius (400 km altitude)
SEED0 = 20231004               # fixed base seed of the synthetic workloads


@dataclasses.dataclass
class Problem:
    """One batch of QPs sharing dynamics, weights and box; differing in x0 (and q).

    minimise   1/2 sum_k [u_k' R u_k + x_{k+1}' Q_{k+1} x_{k+1}] + q' w  [+ sum_k fuel_k ||u_k||_2]
    subject to x_{k+1} = A_k x_k + B_k u_k,  x_0 given,  lo <= w <= hi
    with w = (u_0, x_1, ..., u_{N-1}, x_N), block k = (u_k, x_{k+1}).
    """
    N: int
    A: np.ndarray                 # (n, n) LTI, (N, n, n) LTV, or (batch, N, n, n) per-instance LTV
    B: np.ndarray                 # (n, m), (N, n, m) or (batch, N, n, m)
    Q: np.ndarray                 # (n, n)
    R: np.ndarray                 # (m, m)
    QN: np.ndarray                # (n, n)
    x0: np.ndarray                # (batch, n)
    lo: np.ndarray                # (m + n,), (N, m + n), or (batch, N, m + n) per instance; -inf allowed
    hi: np.ndarray                # likewise; +inf allowed
    q: Optional[np.ndarray] = None  # (batch, L) or None
    # thrust-magnitude bound ||u_k||_2 <= unorm (scalar, or (N,) when the box is per stage); None = off.
    # Where finite, the box of the control rows must be (-inf, inf).
    unorm: Optional[np.ndarray] = None
    name: str = ""
    # scenario consensus: the batch is batch / consensus consecutive groups of `consensus` QPs which share ONE
    # control profile (u_{b,k} equal within a group; x0 and q stay per QP).  None = every QP on its own.  Batch-shared dynamics only.
    # (keyword only in practice: it sits before `fuel`, which stays the last field)
    consensus: Optional[int] = None
    # soft box: weights s >= 0 in the shape of lo / hi ((n + m,), or (N, n + m) with per-stage bounds); the cost gains
    # sum_rows s_i max(lo_i - w_i, 0, w_i - hi_i) and the row's box is no longer enforced absolutely.  +inf = a hard row, 0 = its box is
    # ignored.  None = every row hard.  +inf on the control rows where unorm is finite or fuel positive.  Batch-shared dynamics only.
    soft: Optional[np.ndarray] = None
    # one approach cone per stage:  r <= cone_g[k] s  on xi_k, the first nh state rows of block k, with e = c / |c|,
    # s = e . (xi_k - p), r = |(xi_k - p) - s e|: axis cone_c[k], apex cone_p[k], slope cone_g[k] > 0 (the tangent of the half-angle).
    # cone_c and cone_p are (N, nh) with cone_g (N,) -- shared by the batch -- or (batch, N, nh) with (batch, N) -- one set per QP;
    # nh = cone_c.shape[-1], 1 <= nh <= n.  cone_c[k] = 0 exactly: no cone at that stage.  Where a stage has one for any QP, state rows
    # 0 .. nh - 1 of the stage must have the box (-inf, inf).  All three or none; finite.  Batch-shared dynamics only; not with soft,
    # consensus or half-spaces.  (They sit before `fuel`, which stays the last field.)
    cone_c: Optional[np.ndarray] = None
    cone_p: Optional[np.ndarray] = None
    cone_g: Optional[np.ndarray] = None
    # one half-space per stage:  hs_a[k] . xi_k <= hs_b[k]  on xi_k, the first nh state rows of block k.  hs_a is
    # (N, nh) with hs_b (N,) -- shared by the batch -- or (batch, N, nh) with (batch, N) -- one set per QP; nh = hs_a.shape[-1],
    # 1 <= nh <= n.  hs_a[k] = 0 exactly: no half-space at that stage.  Where a stage has one for any QP, state rows 0 .. nh - 1 of the
    # stage must have the box (-inf, inf).  Both or neither; finite.  Batch-shared dynamics only; not with soft or consensus.
    hs_a: Optional[np.ndarray] = None
    hs_b: Optional[np.ndarray] = None
    # minimum-fuel cost  + sum_k fuel_k ||u_k||_2  (fuel >= 0: scalar, or (N,) when the box is per stage); None = off.
    # Where positive, the box of the control rows must be (-inf, inf).  Batch-shared dynamics only.
    fuel: Optional[np.ndarray] = None

    @property
    def n(self) -> int:
        return int(self.B.shape[-2])

    @property
    def m(self) -> int:
        return int(self.B.shape[-1])

    @property
    def nb(self) -> int:
        return self.n + self.m

    @property
    def L(self) -> int:
        return self.N * self.nb

    @property
    def batch(self) -> int:
        return int(self.x0.shape[0])

    @property
    def time_varying(self) -> bool:
        return self.A.ndim >= 3

    @property
    def per_instance(self) -> bool:
        """Every QP has its own dynamics (admm_problem.time_varying = 2)."""
        return self.A.ndim == 4

    @property
    def per_instance_bounds(self) -> bool:
        """Every QP has its own per-stage box (admm_problem.stage_bounds = 2)."""
        return self.lo.ndim == 3

    @property
    def z_kind(self) -> Optional[str]:
        """The extension of the z-update the problem asks for: "consensus", "soft", "halfspace", "cone", or None.
        validate() admits at most one; a fuel term and a thrust bound compose with each and are not one."""
        if self.cone_c is not None:
            return "cone"
        if self.hs_a is not None:
            return "halfspace"
        if self.soft is not None:
            return "soft"
        return "consensus" if self.consensus is not None else None

    def slice(self, start: int, stop: int) -> "Problem":
        """Contiguous sub-batch [start, stop): the sharding unit."""
        rep = dict(x0=np.ascontiguousarray(self.x0[start:stop]),
                   q=None if self.q is None else np.ascontiguousarray(self.q[start:stop]))
        if self.per_instance:
            rep.update(A=np.ascontiguousarray(self.A[start:stop]), B=np.ascontiguousarray(self.B[start:stop]))
        if self.per_instance_bounds:
            rep.update(lo=np.ascontiguousarray(self.lo[start:stop]), hi=np.ascontiguousarray(self.hi[start:stop]))
        if self.hs_a is not None and np.ndim(self.hs_a) == 3:
            rep.update(hs_a=np.ascontiguousarray(self.hs_a[start:stop]), hs_b=np.ascontiguousarray(self.hs_b[start:stop]))
        if self.cone_c is not None and np.ndim(self.cone_c) == 3:
            rep.update({k: np.ascontiguousarray(getattr(self, k)[start:stop]) for k in ("cone_c", "cone_p", "cone_g")})
        return dataclasses.replace(self, **rep)

    def validate(self) -> None:
        n, m, N = self.n, self.m, self.N
        if N < 1 or n < 1 or m < 1:
            raise ValueError("N, n, m must be positive")
        if self.A.shape[-2:] != (n, n) or self.B.shape[-2:] != (n, m):
            raise ValueError("A/B shape mismatch")
        if self.A.ndim == 3 and self.A.shape[0] != N:
            raise ValueError("time-varying A must have N stages")
        if self.B.ndim == 3 and self.B.shape[0] != N:
            raise ValueError("time-varying B must have N stages")
        if self.A.ndim != self.B.ndim:
            raise ValueError("A and B must both be LTI, both LTV or both per-instance")
        if self.A.ndim == 4 and (self.A.shape[:2] != (self.x0.shape[0], N) or self.B.shape[:2] != (self.x0.shape[0], N)):
            raise ValueError("per-instance A / B must be (batch, N, n, n) / (batch, N, n, m)")
        if self.Q.shape != (n, n) or self.QN.shape != (n, n) or self.R.shape != (m, m):
            raise ValueError("weight shape mismatch")
        if self.x0.ndim != 2 or self.x0.shape[1] != n:
            raise ValueError("x0 must be (batch, n)")
        for b in (self.lo, self.hi):
            if b.shape not in ((n + m,), (N, n + m), (self.x0.shape[0], N, n + m)):
                raise ValueError("bounds must be (n+m,), (N, n+m) or (batch, N, n+m)")
        if self.lo.shape != self.hi.shape:
            raise ValueError("lo and hi must have the same shape")
        if self.lo.ndim == 3 and not self.per_instance:
            raise ValueError("per-instance bounds need per-instance dynamics")
        if np.any(np.isnan(self.lo)) or np.any(np.isnan(self.hi)) or np.any(self.lo > self.hi):
            raise ValueError("bounds must satisfy lo <= hi and contain no NaN")
        if self.q is not None and self.q.shape != (self.batch, self.L):
            raise ValueError("q must be (batch, L)")
        if self.unorm is not None:
            un = np.asarray(self.unorm, np.float64)
            if un.ndim > 1 or (un.ndim == 1 and (self.lo.ndim < 2 or un.shape != (N,))):
                raise ValueError("unorm must be a scalar, or (N,) together with per-stage bounds")
            if np.any(np.isnan(un)) or np.any(un <= 0):
                raise ValueError("unorm must be positive (inf = off)")
            # (stages, m) control-row bounds of every QP: (1 | N, m) shared, (batch, N, m) per instance
            lo_u = (self.lo if self.lo.ndim == 3 else np.atleast_2d(self.lo)[None])[..., :m]
            hi_u = (self.hi if self.hi.ndim == 3 else np.atleast_2d(self.hi)[None])[..., :m]
            fin = np.isfinite(np.broadcast_to(un, (lo_u.shape[1],)))
            if np.any(np.isfinite(lo_u[:, fin])) or np.any(np.isfinite(hi_u[:, fin])):
                raise ValueError("control rows must be unbounded (-inf, inf) where unorm is finite")
        if self.fuel is not None:
            fu = np.asarray(self.fuel, np.float64)
            if fu.ndim > 1 or (fu.ndim == 1 and (self.lo.ndim < 2 or fu.shape != (N,))):
                raise ValueError("fuel must be a scalar, or (N,) together with per-stage bounds")
            if not np.all(np.isfinite(fu)) or np.any(fu < 0):
                raise ValueError("fuel must be finite and >= 0")
            if self.per_instance:
                raise ValueError("fuel needs batch-shared dynamics (A, B LTI or LTV)")
            lo_u, hi_u = np.atleast_2d(self.lo)[:, :m], np.atleast_2d(self.hi)[:, :m]
            pos = np.broadcast_to(fu, (lo_u.shape[0],)) > 0
            if np.any(np.isfinite(lo_u[pos])) or np.any(np.isfinite(hi_u[pos])):
                raise ValueError("control rows must be unbounded (-inf, inf) where fuel is positive")
        if self.soft is not None:
            so = np.asarray(self.soft, np.float64)
            if self.per_instance or self.lo.ndim == 3:
                raise ValueError("soft needs batch-shared dynamics and a batch-shared box (A, B LTI or LTV)")
            if so.shape not in ((n + m,), self.lo.shape):
                raise ValueError("soft must have the shape of lo / hi: (n+m,), or (N, n+m) together with per-stage bounds")
            if np.any(np.isnan(so)) or np.any(so < 0):
                raise ValueError("soft must be >= 0 (inf = a hard row) and contain no NaN")
            if self.consensus is not None:
                raise ValueError("soft cannot be combined with consensus")
            su = np.broadcast_to(so, self.lo.shape).reshape(-1, n + m)[:, :m]
            hard = np.zeros(su.shape[0], bool)
            if self.unorm is not None:
                hard |= np.isfinite(np.broadcast_to(np.asarray(self.unorm, np.float64), hard.shape))
            if self.fuel is not None:
                hard |= np.broadcast_to(np.asarray(self.fuel, np.float64), hard.shape) > 0
            if np.any(su[hard] != np.inf):
                raise ValueError("soft must be inf on the control rows where unorm is finite or fuel is positive")
        if (self.hs_a is None) != (self.hs_b is None):
            raise ValueError("hs_a and hs_b must be given together")
        if self.hs_a is not None and not hasattr(self.hs_a, "is_cuda"):
            # (CUDA tensors: what Solver.set_halfspace left here after the device form; the library has checked them on the device)
            check_halfspaces(self, self.hs_a, self.hs_b)
        if len({self.cone_c is None, self.cone_p is None, self.cone_g is None}) != 1:
            raise ValueError("cone_c, cone_p and cone_g must be given together")
        if self.cone_c is not None and not hasattr(self.cone_c, "is_cuda"):
            # (CUDA tensors: what Solver.set_cone left here after the device form; the library has checked them on the device)
            check_cones(self, self.cone_c, self.cone_p, self.cone_g)
        if self.consensus is not None:
            G = int(self.consensus)
            if G != self.consensus or G < 1 or self.batch % G != 0:
                raise ValueError("consensus (the group size) must be an integer >= 1 that divides batch")
            if self.per_instance:
                raise ValueError("consensus needs batch-shared dynamics (A, B LTI or LTV)")
        for a in (self.A, self.B, self.Q, self.R, self.QN, self.x0):
            # (stacks of hundreds of MB -- per-instance dynamics -- are left to the library's own threaded check at admm_setup /
            #  admm_update_problem, which Solver reports as the same ValueError: NumPy's pass over 7 GB costs 0.4 s per call)
            if a.nbytes <= (256 << 20) and not np.all(np.isfinite(a)):
                raise ValueError("non-finite problem data")



def halfspace_form(a, b, N: int, n: int, batch: int):
    """(nh, per_qp) of half-space arrays by their shapes: (N, nh) with (N,), or (batch, N, nh) with (batch, N).  ValueError otherwise.
    (With batch = 1 a 3-d array is the per-QP form.)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 2 and a.shape[0] == N and b.shape == (N,):
        per_qp = False
    elif a.ndim == 3 and a.shape[:2] == (batch, N) and b.shape == (batch, N):
        per_qp = True
    else:
        raise ValueError(f"hs_a / hs_b must be (N, nh) with (N,), or (batch, N, nh) with (batch, N); got {a.shape} with {b.shape}")
    nh = int(a.shape[-1])
    if not 1 <= nh <= n:
        raise ValueError(f"hs_a: nh = {nh} must lie in 1 .. n = {n}")
    return nh, per_qp


def check_halfspaces(p, a, b) -> None:
    """The rules of Problem.hs_a / hs_b against the rest of p (ValueError): shapes, finite entries, a normal a.a where a != 0,
    an open box on state rows 0 .. nh - 1 of every stage that has a half-space for some QP."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nh, _ = halfspace_form(a, b, p.N, p.n, p.batch)
    if p.per_instance or p.lo.ndim == 3:
        raise ValueError("half-spaces need batch-shared dynamics and a batch-shared box (A, B LTI or LTV)")
    if p.soft is not None or p.consensus is not None:
        raise ValueError("half-spaces cannot be combined with soft or consensus")
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        raise ValueError("hs_a and hs_b must be finite")
    a3 = a.reshape(-1, p.N, nh)
    nz = np.any(a3 != 0, axis=2)
    with np.errstate(over="ignore", under="ignore"):
        nn = np.sum(a3 * a3, axis=2)
    if np.any(nz & ~((nn >= np.finfo(np.float64).tiny) & np.isfinite(nn))):
        raise ValueError("hs_a: a.a of a stage with a half-space must be a normal number (scale the row)")
    active = np.any(nz, axis=0)                                            # (N,)
    lo_x = np.broadcast_to(np.atleast_2d(p.lo), (p.N, p.nb))[:, p.m:p.m + nh]
    hi_x = np.broadcast_to(np.atleast_2d(p.hi), (p.N, p.nb))[:, p.m:p.m + nh]
    if np.any(lo_x[active] != -np.inf) or np.any(hi_x[active] != np.inf):
        raise ValueError("state rows 0 .. nh - 1 must be unbounded (-inf, inf) at a stage with a half-space")


def cone_form(c, apex, g, N: int, n: int, batch: int):
    """(nh, per_qp) of cone arrays by their shapes: (N, nh) twice with (N,), or (batch, N, nh) twice with (batch, N).  ValueError
    otherwise.  (With batch = 1 a 3-d array is the per-QP form.)"""
    c, apex, g = np.asarray(c), np.asarray(apex), np.asarray(g)
    if c.ndim == 2 and c.shape[0] == N and apex.shape == c.shape and g.shape == (N,):
        per_qp = False
    elif c.ndim == 3 and c.shape[:2] == (batch, N) and apex.shape == c.shape and g.shape == (batch, N):
        per_qp = True
    else:
        raise ValueError("cone_c / cone_p / cone_g must be (N, nh) twice with (N,), or (batch, N, nh) twice with (batch, N); "
                         f"got {c.shape}, {apex.shape} with {g.shape}")
    nh = int(c.shape[-1])
    if not 1 <= nh <= n:
        raise ValueError(f"cone_c: nh = {nh} must lie in 1 .. n = {n}")
    return nh, per_qp


def check_cones(p, c, apex, g) -> None:
    """The rules of Problem.cone_c / cone_p / cone_g against the rest of p (ValueError): shapes, finite entries, where c != 0 a normal
    c.c and a positive normal slope with 1 + g^2 finite, an open box on state rows 0 .. nh - 1 of every stage that has a cone for some
    QP."""
    c, apex, g = (np.asarray(x, np.float64) for x in (c, apex, g))
    nh, _ = cone_form(c, apex, g, p.N, p.n, p.batch)
    if p.per_instance or p.lo.ndim == 3:
        raise ValueError("approach cones need batch-shared dynamics and a batch-shared box (A, B LTI or LTV)")
    if p.soft is not None or p.consensus is not None or p.hs_a is not None:
        raise ValueError("approach cones cannot be combined with soft, consensus or half-spaces")
    if not (np.all(np.isfinite(c)) and np.all(np.isfinite(apex)) and np.all(np.isfinite(g))):
        raise ValueError("cone_c, cone_p and cone_g must be finite")
    c3, g2 = c.reshape(-1, p.N, nh), g.reshape(-1, p.N)
    nz = np.any(c3 != 0, axis=2)
    tiny = np.finfo(np.float64).tiny
    with np.errstate(over="ignore", under="ignore"):
        nn = np.sum(c3 * c3, axis=2)
        gg = 1.0 + g2 * g2
    if np.any(nz & ~((nn >= tiny) & np.isfinite(nn))):
        raise ValueError("cone_c: c.c of a stage with a cone must be a normal number (scale the axis)")
    if np.any(nz & ~((g2 >= tiny) & np.isfinite(gg))):
        raise ValueError("cone_g: the slope of a stage with a cone must be a positive normal number with 1 + g^2 finite")
    active = np.any(nz, axis=0)                                            # (N,)
    lo_x = np.broadcast_to(np.atleast_2d(p.lo), (p.N, p.nb))[:, p.m:p.m + nh]
    hi_x = np.broadcast_to(np.atleast_2d(p.hi), (p.N, p.nb))[:, p.m:p.m + nh]
    if np.any(lo_x[active] != -np.inf) or np.any(hi_x[active] != np.inf):
        raise ValueError("state rows 0 .. nh - 1 must be unbounded (-inf, inf) at a stage with a cone")


@dataclasses.dataclass
class DeviceProblem:
    """A Problem whose arrays are fp64 torch tensors in the memory of ONE GPU (same fields, same shapes, same C order as Problem):
    what Solver hands to the device-memory entry points (admm_setup_device, admm_update_problem_device) -- a
    caller that builds its QP data on the GPU (scvx.linearise_device) gives it to the library without a trip through host memory.
    The data themselves are checked by the library, on the device; validate() checks types, devices, shapes and layout."""
    N: int
    A: "torch.Tensor"
    B: "torch.Tensor"
    Q: "torch.Tensor"
    R: "torch.Tensor"
    QN: "torch.Tensor"
    x0: "torch.Tensor"
    lo: "torch.Tensor"
    hi: "torch.Tensor"
    q: Optional["torch.Tensor"] = None
    unorm: Optional["torch.Tensor"] = None      # 0-d, or (N,) with per-stage bounds
    name: str = ""
    consensus: Optional[int] = None             # Problem's field; scenario consensus has no device-memory setup (Solver refuses it)
    soft: Optional["torch.Tensor"] = None       # Problem's field; soft constraints have no device-memory setup (Solver refuses it)
    cone_c: Optional["torch.Tensor"] = None     # Problem's fields; approach cones have no device-memory setup (Solver refuses it): the
    cone_p: Optional["torch.Tensor"] = None     # device-memory route is Solver.set_cone with CUDA tensors
    cone_g: Optional["torch.Tensor"] = None
    hs_a: Optional["torch.Tensor"] = None       # Problem's fields; half-spaces have no device-memory setup (Solver refuses it): the
    hs_b: Optional["torch.Tensor"] = None       # device-memory route is Solver.set_halfspace with CUDA tensors
    fuel: Optional["torch.Tensor"] = None      # Problem's field; the device entry points have no fuel term (Solver refuses it)

    n = Problem.n
    m = Problem.m
    nb = Problem.nb
    L = Problem.L
    batch = Problem.batch
    time_varying = Problem.time_varying
    per_instance = Problem.per_instance
    per_instance_bounds = Problem.per_instance_bounds

    @property
    def device(self):
        return self.x0.device

    @classmethod
    def from_problem(cls, p: Problem, device="cuda:0") -> "DeviceProblem":
        """The same data, copied to `device` (bit for bit)."""
        import torch

        def t(a):
            return None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float64), device=device)
        return cls(N=p.N, A=t(p.A), B=t(p.B), Q=t(p.Q), R=t(p.R), QN=t(p.QN), x0=t(p.x0), lo=t(p.lo), hi=t(p.hi), q=t(p.q),
                   unorm=None if p.unorm is None else t(np.asarray(p.unorm, np.float64)), name=p.name,
                   fuel=None if p.fuel is None else t(np.asarray(p.fuel, np.float64)), consensus=p.consensus,
                   soft=None if p.soft is None else t(np.asarray(p.soft, np.float64)), hs_a=t(p.hs_a), hs_b=t(p.hs_b),
                   cone_c=t(p.cone_c), cone_p=t(p.cone_p), cone_g=t(p.cone_g))

    def validate(self) -> None:
        """ValueError unless every array is a contiguous fp64 CUDA tensor on the device of x0 with Problem's shapes."""
        import torch
        if self.fuel is not None:
            raise ValueError("fuel: the minimum-fuel term has no device-memory form (its weights are at most N doubles): "
                             "give a Problem with NumPy arrays")
        if self.consensus is not None:
            raise ValueError("consensus: scenario consensus has no device-memory setup: give a Problem with NumPy arrays")
        if self.soft is not None:
            raise ValueError("soft: soft constraints have no device-memory setup: give a Problem with NumPy arrays")
        if self.hs_a is not None or self.hs_b is not None:
            raise ValueError("hs_a / hs_b: half-spaces have no device-memory setup: give a Problem with NumPy arrays "
                             "(Solver.set_halfspace takes CUDA tensors)")
        if self.cone_c is not None or self.cone_p is not None or self.cone_g is not None:
            raise ValueError("cone_c / cone_p / cone_g: approach cones have no device-memory setup: give a Problem with NumPy arrays "
                             "(Solver.set_cone takes CUDA tensors)")
        dev =self.x0.device if torch.is_tensor(self.x0) else None
        for name in ("A", "B", "Q", "R", "QN", "x0", "lo", "hi", "q", "unorm"):
            a = getattr(self, name)
            if a is None and name in ("q", "unorm"):
                continue
            check_device_tensor(name, a, dev)
        n, m, N, batch = self.n, self.m, self.N, self.batch
        if N < 1 or n < 1 or m < 1:
            raise ValueError("N, n, m must be positive")
        shapes = {"A": {(n, n), (N, n, n), (batch, N, n, n)}, "B": {(n, m), (N, n, m), (batch, N, n, m)},
                  "Q": {(n, n)}, "R": {(m, m)}, "QN": {(n, n)}, "x0": {(batch, n)},
                  "lo": {(n + m,), (N, n + m), (batch, N, n + m)}, "hi": {(n + m,), (N, n + m), (batch, N, n + m)}}
        for name, ok in shapes.items():
            if tuple(getattr(self, name).shape) not in ok:
                raise ValueError(f"{name}: shape {tuple(getattr(self, name).shape)} is none of {sorted(ok)}")
        if self.A.dim() != self.B.dim():
            raise ValueError("A and B must both be LTI, both LTV or both per-instance")
        if self.lo.shape != self.hi.shape:
            raise ValueError("lo and hi must have the same shape")
        if self.lo.dim() == 3 and not self.per_instance:
            raise ValueError("per-instance bounds need per-instance dynamics")
        if self.q is not None and tuple(self.q.shape) != (batch, self.L):
            raise ValueError("q must be (batch, L)")
        if self.unorm is not None and tuple(self.unorm.shape) not in ({(), (N,)} if self.lo.dim() >= 2 else {()}):
            raise ValueError("unorm must be a scalar, or (N,) together with per-stage bounds")


def check_device_tensor(name: str, a, device=None, shape=None) -> None:
    """ValueError unless `a` is a contiguous fp64 CUDA tensor (on `device`, of `shape`, where given): what the device-memory entry
    points take.  A CPU tensor -- pinned or not -- is refused here, before the library is called."""
    import torch
    if not torch.is_tensor(a):
        raise ValueError(f"{name}: expected a torch tensor in GPU memory, got {type(a).__name__}")
    if a.dtype != torch.float64:
        raise ValueError(f"{name}: dtype {a.dtype}, expected torch.float64")
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
    if not a.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if not a.is_cuda:
        raise ValueError(f"{name}: a CPU tensor; the device-memory form takes GPU tensors")
    if device is not None and a.device != torch.device(device):
        raise ValueError(f"{name}: on {a.device}, expected {torch.device(device)}")


def double_integrator(N: int = 50, batch: int = 1, seed0: int = SEED0,
                      dt: float = 0.2, u_max: float = 1.0) -> Problem:
    """BASELINE.json configs[0]: 2-state LQR QP, box input constraint |u| <= u_max.
    m = 1 (one force input); instance 0 starts at (4, 0), further instances are
    drawn from default_rng(seed0 + instance)."""
    A = np.array([[1.0, dt], [0.0, 1.0]])
    B = np.array([[0.5 * dt * dt], [dt]])
    Q = np.diag([1.0, 0.1])
    R = np.array([[0.1]])
    QN = np.diag([10.0, 1.0])
    x0 = np.empty((batch, 2))
    for i in range(batch):
        if i == 0:
            x0[i] = (4.0, 0.0)
        else:
            rng = np.random.default_rng(seed0 + i)
            x0[i] = rng.uniform([-5.0, -1.0], [5.0, 1.0])
    inf = np.inf
    lo = np.array([-u_max, -inf, -inf])
    hi = np.array([u_max, inf, inf])
    return Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=lo, hi=hi,
                   name=f"double_integrator_N{N}_b{batch}")


def cw_matrices(dt: float):
    """Zero-order-hold discretisation of the Clohessy-Wiltshire equations in
    nondimensional form (time unit 1/mean-motion, so the mean motion is 1):

        x'' = 3 x + 2 y' + u_x,   y'' = -2 x' + u_y,   z'' = -z + u_z

    State (x, y, z, vx, vy, vz).  Closed form of expm([[Ac, Bc],[0,0]] dt)."""
    s, c = np.sin(dt), np.cos(dt)
    A = np.array([
        [4 - 3 * c,       0, 0,  s,            2 * (1 - c),      0],
        [6 * (s - dt),    1, 0, -2 * (1 - c),  4 * s - 3 * dt,   0],
        [0,               0, c,  0,            0,                s],
        [3 * s,           0, 0,  c,            2 * s,            0],
        [-6 * (1 - c),    0, 0, -2 * s,        4 * c - 3,        0],
        [0,               0, -s, 0,            0,                c],
    ])
    # B = int_0^dt Phi(tau) d tau  @ [0; I]
    B = np.array([
        [1 - c,                 2 * (dt - s),                 0],
        [-2 * (dt - s),         4 * (1 - c) - 1.5 * dt * dt,  0],
        [0,                     0,                            1 - c],
        [s,                     2 * (1 - c),                  0],
        [-2 * (1 - c),          4 * s - 3 * dt,               0],
        [0,                     0,                            s],
    ])
    return A, B


def mean_motion(mu: float = MU_EARTH, a: float = A_REF) -> float:
    """rad/s of the circular reference orbit; defines the time unit of cw_matrices."""
    return float(np.sqrt(mu / a ** 3))


def cw_rendezvous(N: int = 1000, batch: int = 1, seed0: int = SEED0,
                  u_max: float = 0.2, thrust_norm: bool = False) -> Problem:
    """BASELINE.json configs[1..3]: orbit-transfer (rendezvous) QP, n = 6, m = 3.

    Horizon = one orbital period, dt = 2 pi / N in units of 1/mean-motion; length
    unit 1 km, so velocities are km * mean-motion and thrust accelerations are
    km * mean-motion^2: all variables are O(1).  Input box |u_i| <= u_max, states
    unbounded, q = 0.  x0 of instance i ~ U(box) from default_rng(seed0 + i).
    thrust_norm=True replaces the input box by the thrust-magnitude bound ||u_k||_2 <= u_max
    (the natural constraint of a single gimballed thruster)."""
    dt = 2.0 * np.pi / N
    A, B = cw_matrices(dt)
    Q = np.diag([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]) * dt
    R = np.eye(3) * dt
    QN = np.diag([50.0, 50.0, 50.0, 20.0, 20.0, 20.0])
    box = np.array([0.3, 2.0, 1.0, 0.1, 0.1, 0.1])
    x0 = np.empty((batch, 6))
    for i in range(batch):
        rng = np.random.default_rng(seed0 + i)
        x0[i] = rng.uniform(-box, box)
    inf = np.inf
    if thrust_norm:
        return Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=np.full(9, -inf), hi=np.full(9, inf),
                       unorm=np.float64(u_max), name=f"cw_rendezvous_soc_N{N}_b{batch}")
    lo = np.array([-u_max] * 3 + [-inf] * 6)
    hi = np.array([u_max] * 3 + [inf] * 6)
    return Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=lo, hi=hi,
                   name=f"cw_rendezvous_N{N}_b{batch}")


def cw_rendezvous_fuel(N: int = 1000, batch: int = 1, seed0: int = SEED0, u_max: float = 0.2,
                       fuel: Optional[float] = None) -> Problem:
    """The fuel-optimal form of cw_rendezvous(thrust_norm=True): the same QPs with the cost term  + fuel sum_k ||u_k||_2  under
    the thrust bound ||u_k||_2 <= u_max.  fuel = None: dt = 2 pi / N, the scale of R in this generator -- the
    quadratic and the fuel term then weigh alike, and the solutions coast (u_k = 0 exactly) over a good part of the orbit and
    burn at the bound over another.  rho 0.05 ... 0.1 suits it."""
    p = cw_rendezvous(N=N, batch=batch, seed0=seed0, u_max=u_max, thrust_norm=True)
    f = 2.0 * np.pi / N if fuel is None else float(fuel)
    return dataclasses.replace(p, fuel=np.float64(f), name=f"cw_rendezvous_fuel_N{N}_b{batch}")


def keepout_halfspaces(X, radius, centre=0.0):
    """Tangent half-spaces of the keep-out sphere |r - c| >= R about positions X of shape (batch, N, 3) (or (N, 3)): with
    n_k = (X_k - c) / |X_k - c| the convexification  n_k . (r_{k+1} - c) >= R  reads  a_k . r <= b_k  with
    a = -n,  b = -(R + n . c)  (DESIGN.md §2.14).  Returns (a, b), shapes X.shape and X.shape[:-1]; a stage whose X_k sits on the
    centre has no direction and gets a = 0, b = 0: no half-space.  radius: a scalar, or one per QP."""
    X = np.asarray(X, np.float64)
    c = np.broadcast_to(np.asarray(centre, np.float64), X.shape)
    d = X - c
    nrm = np.sqrt(np.sum(d * d, axis=-1))
    ok = nrm > 0
    nhat = np.where(ok[..., None], d / np.where(ok, nrm, 1.0)[..., None], 0.0)
    R = np.asarray(radius, np.float64)
    if R.ndim == 1:
        R = R[:, None]
    b = np.where(ok, -(R + np.sum(nhat * c, axis=-1)), 0.0)
    return -nhat, b


def lqr_rollout(p: Problem) -> np.ndarray:
    """(batch, N, n): the states x_1 .. x_N of p's QPs without box, planes or q -- the finite-horizon LQR trajectory of
    (A, B, Q, R, QN) from x0, by the Riccati recursion (batch-shared LTI or LTV dynamics)."""
    N, n = p.N, p.n
    Ak = lambda k: p.A[k] if p.A.ndim == 3 else p.A
    Bk = lambda k: p.B[k] if p.B.ndim == 3 else p.B
    P = p.QN.copy()
    K = [None] * N
    for k in range(N - 1, -1, -1):
        A, B = Ak(k), Bk(k)
        K[k] = np.linalg.solve(p.R + B.T @ P @ B, B.T @ P @ A)
        Acl = A - B @ K[k]
        P = (p.Q if k > 0 else np.zeros((n, n))) + Acl.T @ P @ Acl + K[k].T @ p.R @ K[k]
    X = np.empty((p.batch, N, n))
    x = np.asarray(p.x0, np.float64)
    for k in range(N):
        x = x @ (Ak(k) - Bk(k) @ K[k]).T
        X[:, k] = x
    return X


def cw_keepout(N: int = 40, batch: int = 6, radius: Optional[float] = None, free_tail: int = 5, thrust_norm: bool = False,
               fuel: Optional[float] = None, seed0: int = SEED0) -> Problem:
    """cw_rendezvous with a keep-out sphere of `radius` about the target, convexified as one tangent half-space per stage and QP
    (DESIGN.md §2.14): the planes of keepout_halfspaces about the QPs' unconstrained trajectory (lqr_rollout), which runs straight
    through the target.  The last `free_tail` stages carry no plane (the final approach).  radius = None: half the smallest initial
    range of the batch.  thrust_norm / fuel: the thrust ball instead of the input box, and the minimum-fuel term on top of it."""
    p = cw_rendezvous(N=N, batch=batch, seed0=seed0, thrust_norm=thrust_norm or fuel is not None)
    R = 0.5 * float(np.sqrt(np.sum(p.x0[:, :3] ** 2, axis=1)).min()) if radius is None else float(radius)
    a, b = keepout_halfspaces(lqr_rollout(p)[:, :, :3], R)
    if free_tail > 0:
        a[:, N - free_tail:] = 0.0
        b[:, N - free_tail:] = 0.0
    return dataclasses.replace(p, hs_a=a, hs_b=b, fuel=None if fuel is None else np.float64(fuel),
                               name=f"cw_keepout_N{N}_b{batch}")


def plain_solution(p: Problem, rho: float = 0.5, alpha: float = 1.6, eps: float = 1e-9, max_iter: int = 20000) -> np.ndarray:
    """(batch, L): z of p's QPs with their box, thrust ball, fuel term and q -- no extension of the z-update -- by the ADMM of
    DESIGN.md §2 in NumPy (Riccati x-update, batch-shared dynamics), run until ||w - z|| and rho ||z+ - z|| fall below
    eps sqrt(L) for every QP.  What a generator needs of the unconstrained-by-its-extension trajectory; not a solver to time."""
    N, n, m, nb, L = p.N, p.n, p.m, p.nb, p.L
    A = np.broadcast_to(p.A, (N, n, n))
    B = np.broadcast_to(p.B, (N, n, m))
    P = p.QN + rho * np.eye(n)
    K, Sinv = np.empty((N, m, n)), np.empty((N, m, m))
    for k in range(N - 1, -1, -1):
        PB = P @ B[k]
        S = p.R + rho * np.eye(m) + B[k].T @ PB
        Sinv[k] = np.linalg.inv(S)
        K[k] = Sinv[k] @ (PB.T @ A[k])
        P = p.Q + rho * np.eye(n) + A[k].T @ P @ A[k] - K[k].T @ S @ K[k]
        P = 0.5 * (P + P.T)
    lo = np.broadcast_to(np.atleast_2d(p.lo), (N, nb)).reshape(L)
    hi = np.broadcast_to(np.atleast_2d(p.hi), (N, nb)).reshape(L)
    un = np.full(N, np.inf) if p.unorm is None else np.broadcast_to(np.asarray(p.unorm, np.float64), (N,))
    kap = (np.zeros(N) if p.fuel is None else np.broadcast_to(np.asarray(p.fuel, np.float64), (N,))) / rho
    soc = np.isfinite(un) | (kap > 0)
    batch = p.batch
    z, y = np.zeros((batch, L)), np.zeros((batch, L))
    for _ in range(max_iter):
        g = (-rho * (z - y) + (0.0 if p.q is None else p.q)).reshape(batch, N, nb)
        d, t = np.empty((N, batch, m)), np.zeros((batch, n))
        for k in range(N - 1, -1, -1):
            pk = g[:, k, m:] + t
            h = pk @ B[k] + g[:, k, :m]
            d[k] = h @ Sinv[k].T
            t = pk @ A[k] - h @ K[k]
        w, x = np.empty((batch, N, nb)), np.array(p.x0, np.float64)
        for k in range(N):
            u = -(x @ K[k].T) - d[k]
            x = x @ A[k].T + u @ B[k].T
            w[:, k, :m], w[:, k, m:] = u, x
        w = w.reshape(batch, L)
        v = alpha * w + (1.0 - alpha) * z + y
        zn = np.minimum(np.maximum(v, lo), hi).reshape(batch, N, nb)
        if soc.any():
            vu = v.reshape(batch, N, nb)[:, :, :m]
            nrm = np.sqrt(np.sum(vu * vu, axis=2))
            tt = np.minimum(un, np.maximum(nrm - kap, 0.0))
            zn[:, soc, :m] = (vu * np.where(nrm > tt, tt / np.where(nrm > 0, nrm, 1.0), 1.0)[:, :, None])[:, soc]
        zn = zn.reshape(batch, L)
        r, s = np.sqrt(np.sum((w - zn) ** 2, axis=1)), rho * np.sqrt(np.sum((zn - z) ** 2, axis=1))
        z, y = zn, v - zn
        if max(r.max(), s.max()) <= eps * np.sqrt(L):
            break
    return z


def cw_approach(N: int = 40, batch: int = 6, pull: float = 0.05, free_tail: int = 3, thrust_norm: bool = False,
                fuel: Optional[float] = None, seed0: int = SEED0) -> Problem:
    """cw_rendezvous with an approach cone per stage and QP on the position rows, feasible by construction: with
    the plain problem's solution (plain_solution) at hand, the axis of QP b is the direction of its initial position, the apex
    lies behind the target by 1.5 x (the deepest overshoot along the axis) + 0.1 x (the initial range), and the slope is
    1.05 x max_k r_k / s_k of that solution, which is then strictly inside.  A linear cost q = -pull t^ on the position rows, t^ a
    fixed unit vector orthogonal to the axis, pulls the trajectory into the cone's surface.  The last `free_tail` stages carry no
    cone (c = 0, apex = 0, slope 1).  thrust_norm / fuel: the thrust ball instead of the input box, and the minimum-fuel term on
    top of it (2 pi / N is cw_rendezvous_fuel's weight)."""
    p = cw_rendezvous(N=N, batch=batch, seed0=seed0, thrust_norm=thrust_norm or fuel is not None)
    if fuel is not None:
        p = dataclasses.replace(p, fuel=np.float64(fuel))
    nh = 3
    X = plain_solution(p).reshape(batch, N, p.nb)[:, :, p.m:p.m + nh]
    rng0 = np.sqrt(np.sum(p.x0[:, :nh] ** 2, axis=1))
    e = p.x0[:, :nh] / rng0[:, None]
    along = np.einsum("bki,bi->bk", X, e)
    back = 1.5 * np.maximum(-along.min(axis=1), 0.0) + 0.1 * rng0
    apex = -back[:, None] * e
    dl = X - apex[:, None, :]
    s = np.einsum("bki,bi->bk", dl, e)
    r = np.sqrt(np.maximum(np.sum(dl * dl, axis=2) - s * s, 0.0))
    gam = 1.05 * (r / s)[:, :N - free_tail].max(axis=1)
    # t^: the unit vector of e x z^ (e x x^ for an axis along z^), orthogonal to the axis
    ref = np.where((np.abs(e[:, 2]) < 0.999)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    that = np.cross(e, ref)
    that /= np.sqrt(np.sum(that * that, axis=1))[:, None]
    q = np.zeros((batch, N, p.nb))
    q[:, :, p.m:p.m + nh] = -pull * that[:, None, :]
    c = np.repeat(e[:, None, :], N, axis=1)
    ap = np.repeat(apex[:, None, :], N, axis=1)
    g = np.repeat(gam[:, None], N, axis=1)
    if free_tail > 0:
        c[:, N - free_tail:], ap[:, N - free_tail:], g[:, N - free_tail:] = 0.0, 0.0, 1.0
    return dataclasses.replace(p, q=q.reshape(batch, p.L), cone_c=c, cone_p=ap, cone_g=g,
                               name=f"cw_approach_N{N}_b{batch}" + ("_fuel" if p.fuel is not None else ""))


def cw_rendezvous_scenarios(N: int = 1000, groups: int = 1, group_size: int = 8, spread: float = 0.05, seed0: int = SEED0,
                            u_max: float = 0.2, thrust_norm: bool = False, pos_box=None) -> Problem:
    """Scenario clouds of cw_rendezvous for consensus: `groups` nominal starts x0_g -- instance g of
    cw_rendezvous, the same seeding -- each dispersed into `group_size` scenarios x0_g + spread * box * U(-1, 1)^6 (box: the
    generator's own x0 box; scenario s of group g is drawn from default_rng(seed0 + 1000003 (g + 1) + s)), with
    Problem.consensus = group_size: one thrust profile per group.  pos_box (km; a scalar or one value per axis, inf = open):
    |position| <= pos_box on the state rows of every stage -- a corridor every scenario must respect (x_1 of every scenario has
    to fit: the controls cannot tell the scenarios apart); chosen a little above the nominal trajectory's excursion, the dispersed
    cloud makes it active.  None leaves the states open, and the consensus profile is then the solution for the group's mean x0."""
    p = cw_rendezvous(N=N, batch=groups, seed0=seed0, u_max=u_max, thrust_norm=thrust_norm)
    box = np.array([0.3, 2.0, 1.0, 0.1, 0.1, 0.1])
    x0 = np.empty((groups * group_size, 6))
    for g in range(groups):
        for s in range(group_size):
            rng = np.random.default_rng(seed0 + 1000003 * (g + 1) + s)
            x0[g * group_size + s] = p.x0[g] + spread * box * rng.uniform(-1.0, 1.0, 6)
    lo, hi = p.lo.copy(), p.hi.copy()
    if pos_box is not None:
        pb = np.broadcast_to(np.asarray(pos_box, np.float64), (3,))
        lo[3:6], hi[3:6] = -pb, pb
    return dataclasses.replace(p, x0=x0, lo=lo, hi=hi, consensus=int(group_size),
                               name=f"cw_rendezvous_scenarios_N{N}_g{groups}x{group_size}")


def cw_formation(N: int = 1000, batch: int = 1, seed0: int = SEED0, u_max: float = 0.2) -> Problem:
    """BASELINE.json configs[4] shape (n = 12, m = 6): two spacecraft in Clohessy-Wiltshire
    relative motion about the same reference orbit, each with its own thrust box, coupled through
    the cost: the stage and terminal weights penalise each craft's state AND their separation, so
    Q and QN are full 12 x 12 matrices (block [[Q1+Qr, -Qr], [-Qr, Q2+Qr]])."""
    dt = 2.0 * np.pi / N
    A1, B1 = cw_matrices(dt)
    A = np.block([[A1, np.zeros((6, 6))], [np.zeros((6, 6)), A1]])
    B = np.block([[B1, np.zeros((6, 3))], [np.zeros((6, 3)), B1]])
    q1 = np.diag([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]) * dt
    qr = np.diag([2.0, 2.0, 2.0, 0.2, 0.2, 0.2]) * dt
    Q = np.block([[q1 + qr, -qr], [-qr, q1 + qr]])
    t1 = np.diag([50.0, 50.0, 50.0, 20.0, 20.0, 20.0])
    tr = np.diag([25.0, 25.0, 25.0, 10.0, 10.0, 10.0])
    QN = np.block([[t1 + tr, -tr], [-tr, t1 + tr]])
    R = np.eye(6) * dt
    box = np.array([0.3, 2.0, 1.0, 0.1, 0.1, 0.1] * 2)
    x0 = np.empty((batch, 12))
    for i in range(batch):
        rng = np.random.default_rng(seed0 + i)
        x0[i] = rng.uniform(-box, box)
    inf = np.inf
    lo = np.array([-u_max] * 6 + [-inf] * 12)
    hi = np.array([u_max] * 6 + [inf] * 12)
    return Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=lo, hi=hi,
                   name=f"cw_formation_N{N}_b{batch}")


def random_ltv(N: int, n: int, m: int, batch: int, seed: int = SEED0,
               with_q: bool = True, state_bounds: bool = True, thrust_norm: bool = False) -> Problem:
    """Random stable-ish time-varying problem with full weights, per-stage
    bounds and a linear term: exercises every code path in the parity tests."""
    rng = np.random.default_rng(seed)
    A = np.eye(n)[None] + 0.15 * rng.standard_normal((N, n, n)) / np.sqrt(n)
    B = 0.5 * rng.standard_normal((N, n, m))
    def spd(k, lo_eig):
        M = rng.standard_normal((k, k))
        return M @ M.T / k + lo_eig * np.eye(k)
    Q, R, QN = spd(n, 0.1), spd(m, 0.05), spd(n, 1.0)
    x0 = rng.uniform(-1.0, 1.0, (batch, n))
    lo = np.empty((N, n + m))
    hi = np.empty((N, n + m))
    lo[:, :m] = -rng.uniform(0.1, 0.6, (N, m))
    hi[:, :m] = rng.uniform(0.1, 0.6, (N, m))
    if state_bounds:
        lo[:, m:] = -rng.uniform(0.8, 3.0, (N, n))
        hi[:, m:] = rng.uniform(0.8, 3.0, (N, n))
        lo[::3, m] = -np.inf
        hi[1::4, m + n - 1] = np.inf
    else:
        lo[:, m:] = -np.inf
        hi[:, m:] = np.inf
    q = 0.1 * rng.standard_normal((batch, N * (n + m))) if with_q else None
    unorm = None
    if thrust_norm:      # per-stage thrust-magnitude bounds on most stages, box on the rest
        unorm = rng.uniform(0.15, 0.7, N)
        unorm[::4] = np.inf
        soc = np.isfinite(unorm)
        lo[soc, :m] = -np.inf
        hi[soc, :m] = np.inf
    return Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=lo, hi=hi, q=q, unorm=unorm,
                   name=f"random_ltv_N{N}_n{n}_m{m}_b{batch}")


def random_instances(N: int, n: int, m: int, batch: int, seed: int = SEED0, with_q: bool = True,
                     instance_bounds: bool = True, thrust_norm: bool = False) -> Problem:
    """Per-instance time-varying dynamics (admm_problem.time_varying = 2): every QP is its own
    perturbation of a common random LTV plant, with its own per-stage box (instance_bounds) and linear term --
    the QP class a batched successive-convexification loop produces."""
    base = random_ltv(N, n, m, batch, seed, with_q=with_q, thrust_norm=thrust_norm)
    rng = np.random.default_rng(seed + 7)
    A = base.A[None] + 0.05 * rng.standard_normal((batch, N, n, n)) / np.sqrt(n)
    B = base.B[None] + 0.05 * rng.standard_normal((batch, N, n, m))
    lo, hi = base.lo, base.hi
    if instance_bounds:
        wid = rng.uniform(0.7, 1.3, (batch, N, n + m))
        lo = base.lo[None] * wid
        hi = base.hi[None] * rng.uniform(0.7, 1.3, (batch, N, n + m))
    return dataclasses.replace(base, A=A, B=B, lo=lo, hi=hi, name=f"random_instances_N{N}_n{n}_m{m}_b{batch}")


def cw_rendezvous_instances(N: int = 200, batch: int = 64, seed0: int = SEED0, u_max: float = 0.2,
                            spread: float = 0.05) -> Problem:
    """cw_rendezvous with PER-INSTANCE dynamics: QP i flies about its own reference orbit (mean motion scaled by
    1 + spread * U(-1, 1), so its Clohessy-Wiltshire matrices are those of a different time step) and has its own
    input box -- the shape of a Monte-Carlo / batched successive-convexification workload."""
    base = cw_rendezvous(N=N, batch=batch, seed0=seed0, u_max=u_max)
    dt = 2.0 * np.pi / N
    A = np.empty((batch, N, 6, 6))
    B = np.empty((batch, N, 6, 3))
    lo = np.empty((batch, N, 9))
    hi = np.empty((batch, N, 9))
    for i in range(batch):
        rng = np.random.default_rng(seed0 + 100003 * (i + 1))
        Ai, Bi = cw_matrices(dt * (1.0 + spread * rng.uniform(-1.0, 1.0)))
        A[i], B[i] = Ai[None], Bi[None]
        um = u_max * (1.0 + spread * rng.uniform(-1.0, 1.0))
        lo[i] = np.array([-um] * 3 + [-np.inf] * 6)[None]
        hi[i] = np.array([um] * 3 + [np.inf] * 6)[None]
    return dataclasses.replace(base, A=A, B=B, lo=lo, hi=hi, name=f"cw_rendezvous_instances_N{N}_b{batch}")


def cw_formation_instances(N: int = 200, batch: int = 64, seed0: int = SEED0, u_max: float = 0.2,
                           spread: float = 0.05) -> Problem:
    """cw_formation (n = 12, m = 6) with PER-INSTANCE dynamics: in QP i each of the two craft flies about its own reference
    orbit (mean motion scaled by 1 + spread * U(-1, 1)) and has its own input box -- the wide-shape twin of
    cw_rendezvous_instances."""
    base = cw_formation(N=N, batch=batch, seed0=seed0, u_max=u_max)
    dt = 2.0 * np.pi / N
    A = np.zeros((batch, N, 12, 12))
    B = np.zeros((batch, N, 12, 6))
    lo = np.empty((batch, N, 18))
    hi = np.empty((batch, N, 18))
    for i in range(batch):
        rng = np.random.default_rng(seed0 + 100003 * (i + 1))
        um = np.empty(6)
        for c in range(2):
            Ai, Bi = cw_matrices(dt * (1.0 + spread * rng.uniform(-1.0, 1.0)))
            A[i, :, 6 * c:6 * c + 6, 6 * c:6 * c + 6] = Ai[None]
            B[i, :, 6 * c:6 * c + 6, 3 * c:3 * c + 3] = Bi[None]
            um[3 * c:3 * c + 3] = u_max * (1.0 + spread * rng.uniform(-1.0, 1.0))
        lo[i] = np.concatenate([-um, [-np.inf] * 12])[None]
        hi[i] = np.concatenate([um, [np.inf] * 12])[None]
    return dataclasses.replace(base, A=A, B=B, lo=lo, hi=hi, name=f"cw_formation_instances_N{N}_b{batch}")


def cw_corridor_mpc(N: int = 40, batch: int = 8, corridor: float = 0.25, disturbance: float = 0.05, soft: Optional[float] = None,
                    seed0: int = SEED0, u_max: float = 0.2, dt: float = 2.0 * np.pi / 200):
    """A receding-horizon workload for soft constraints: cw_rendezvous' dynamics, weights and input box over a
    window of N steps of length dt, with a RADIAL CORRIDOR |x| <= corridor (row m of every block: the radial position) on every
    stage, and a per-step radial disturbance for the closed loop.  Returns (problem, dx): dx is (steps = 3 N, batch, 6), a push of
    `disturbance` km on the radial position at every step, outwards (scenario b alternates its sign), drawn as
    disturbance * U(0.5, 1) from default_rng(seed0 + 7919 + b).  The corridor holds x0 with margin; a push of more than the
    controls can take back in one step (B's radial column times u_max is ~ u_max dt^2 / 2, three orders below `disturbance`) puts
    the measured state outside the corridor within a few steps, and x_1 of the next window cannot get back inside: the hard window
    QP has no solution.  soft = None: the hard corridor; a number: that weight on the corridor rows (every other row +inf)."""
    A, B = cw_matrices(dt)
    Q = np.diag([1.0, 1.0, 1.0, 0.1, 0.1, 0.1]) * dt
    R = np.eye(3) * dt
    QN = np.diag([50.0, 50.0, 50.0, 20.0, 20.0, 20.0])
    box = np.array([0.5 * corridor, 1.0, 0.5, 0.02, 0.02, 0.02])
    x0 = np.empty((batch, 6))
    steps = 3 * N
    dx = np.zeros((steps, batch, 6))
    for b in range(batch):
        rng = np.random.default_rng(seed0 + b)
        x0[b] = rng.uniform(-box, box)
        rng = np.random.default_rng(seed0 + 7919 + b)
        dx[:, b, 0] = (1.0 if b % 2 == 0 else -1.0) * disturbance * rng.uniform(0.5, 1.0, steps)
    inf = np.inf
    lo = np.array([-u_max] * 3 + [-corridor] + [-inf] * 5)
    hi = np.array([u_max] * 3 + [corridor] + [inf] * 5)
    sw = None
    if soft is not None:
        sw = np.full(9, inf)
        sw[3] = float(soft)
    p = Problem(N=N, A=A, B=B, Q=Q, R=R, QN=QN, x0=x0, lo=lo, hi=hi, soft=sw,
                name=f"cw_corridor_mpc_N{N}_b{batch}" + ("" if soft is None else "_soft"))
    return p, dx
