"""Host model of a solver handle for the call-sequence tests (tests/test_gpu_sequences.py, tests/test_handle_model_host.py).

A plain NumPy object with the public methods of admm_library_amd.Solver.  It holds what include/admm_hip.h says a handle holds
-- the problem, rho (one per QP with per-instance dynamics), alpha, the fuel weights, (w, z, y), the residual norms of the last
residual-evaluating iteration, the results of the last solve -- and NOTHING of how the library keeps them (v = z + y, stale w,
elimination direction, side data, deferred finalise, graphs): that hidden state is what the sequences are there to catch.

Built only from what the suite already trusts:
  iterations            oracle_c.solve(..., z0, y0, max_iter=k, stop=False); tests/_fuel_ref.solve on a handle with a fuel term;
                        QP by QP (oracle_c._one_instance) with per-instance dynamics, every QP with its own rho
  residual norms        admm_ref.residuals on the oracle's iterates of that iteration
  stopping / adaptive   admm_ref.converged and the rule of admm_ref.solve, applied at the checked iterations -- the host test
                        pins the loop against one oracle_c.solve with the stopping and adaptive rules
  step_x / step_z       admm_ref.factor, x_update, z_update (tests/_fuel_ref.prox with a fuel term)
  certificate           tests/_cert_ref.certificate
  soft / consensus      tests/_soft_ref.solve, prox, report; tests/_consensus_ref.solve, prox, consensus_of
  mpc_advance           admm_library_amd.mpc: shift_horizon, plant_step, model_plant
  infeasibility         tests/_infeas_ref.probe on the handle's problem with the box of every finite-weight row removed

A call the header refuses raises Refused(code) and changes nothing.  `margins` collects every comparison of the stopping and
adaptive rules the model took, as (what, lhs, threshold): the host test keeps them away from their thresholds -- and those of the
probe (sep against -eps, the open-row magnitude against eps |mu|_inf); `unclear` lists the probe's decisions mu = 0 and lambda = 0 (a
number against +inf in sep and defect) that are neither clearly nonzero nor zero by construction: there `defect` is a quotient of two
rounding errors, and the probe's read-out says so per QP (defect_clear).  `soft_rows` counts, per soft report, the finite-weight rows
that are neither clearly outside their box, nor clearly inside, nor exactly on a bound with |y| clear of s / rho.

Half-spaces and approach cones (tests/_halfspace_ref.py, tests/_cone_ref.py: solve, prox, report; the payload is the problem's hs_* /
cone_* fields, replaced by set_halfspace / set_cone under the checks of halfspace_stages / cone_stages and the open-box rule, kept by
update_problem under the open-box rule).  Their reports count EXACT decisions -- lam > 0 of a plane, y_xi != 0 of a cone (a stage
inside its cone has y_xi = 0 exactly) -- so the model keeps, per (QP, stage), whether rounding could flip the one the state holds.
The unclear-stage rule: after every call that ends on a z-update a stage is marked when that update's input v_xi = z_xi + y_xi lies
within 1e-6 max(1, |v_xi|_2) of the boundary -- |a . v - b| / |a| for a plane, |r - g s| / sqrt(1 + g^2) for a cone; the marks stay
until the next z-update, and set_state with a y clears them (the caller's y is exact on both sides).  At a report a stage with a
plane / cone is unclear when it is marked or when 0 < |lam| <= 1e-6 max(1, rho |y|_inf of its QP).  `plane_stages` receives, per
report, (stages with a plane / cone, unclear stages); `z_stage_kinds` the stage kinds of the z-updates the model ran (a half-space
handle: (active, satisfied, no plane) of the last z-update of every call; a cone handle: (inside, apex, surface, no cone) of each).
"""
import dataclasses

import numpy as np

import admm_ref as ar
import oracle_c as oc
import _cert_ref as cr
import _consensus_ref as cs
import _cone_ref as cn
import _fuel_ref as fr
import _halfspace_ref as hr
import _infeas_ref as ir
import _soft_ref as sr
from admm_library_amd import mpc

PRECISION_MIXED = 1

INVALID, UNSUPPORTED, NUMERIC = 1, 2, 5


class Refused(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"refused ({code}): {why}")
        self.code = code


_REFS = {"soft": sr, "consensus": cs, "halfspace": hr, "cone": cn}


class HandleModel:
    def __init__(self, problem, options, alternating=False, fused=True):
        """alternating: the handle runs the alternating-direction kernels (admm_profile modes 2 and 3 exist only there)."""
        problem.validate()
        self.p = problem
        self.opt = options
        self.alpha = float(options.alpha)
        self.per_qp = problem.per_instance
        B, L = problem.batch, problem.L
        self.rho = np.full(B, float(options.rho)) if self.per_qp else float(options.rho)
        self.w, self.z, self.y = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L))
        self.resid = None            # (r, s, nw, nz, ny) of the last residual-evaluating iteration
        self.info = None             # dict of the last solve
        self.alternating = alternating
        self.fused = fused and problem.z_kind is None                # (a handle with an extension of the z-update runs the unfused path only)
        self.pair_form = True        # the state is held as the (z, y) pair (admm_profile modes 2 / 3 then add one iteration)
        self.iterations = 0          # applied since set-up
        self.margins = []
        self.probes = 0              # probes so far
        self.unclear = []            # (probe, what, QP, value, rounding scale) of a zero / nonzero decision that rounding could flip
        self.soft_rows = []          # per soft report: (rows with a finite weight, rows of none of the three kinds)
        self.plane_stages = []       # per half-space / cone report: (stages with a plane / cone, unclear stages)
        self.z_stage_kinds = []      # stage kinds at the z-updates of a half-space / cone handle (the module docstring)
        self._edge = np.zeros((B, problem.N), bool)      # (QP, stage): the last z-update's input lay on the boundary, to rounding
        self._subs = None
        self._it = 0
        self._status = np.zeros(B, np.int32)
        self._iters = np.zeros(B, np.int32)
        self._nupd = np.zeros(B, np.int64)
        self._rho_updates = 0
        self._nconv = 0

    # ---- iterations -------------------------------------------------------------------------------------------------------
    def _sub(self, b):
        if self._subs is None:
            self._subs = [oc._one_instance(self.p, i) for i in range(self.p.batch)]
        return self._subs[b]

    def _oracle(self, k):
        """k iterations from (z, y), no residuals, no stop."""
        if k <= 0:
            return
        kw = dict(alpha=self.alpha, max_iter=k, check_interval=k, stop=False)
        if self.per_qp:
            outs = [oc.solve(self._sub(b), rho=float(self.rho[b]), z0=self.z[b:b + 1], y0=self.y[b:b + 1], nthreads=1, **kw)
                    for b in range(self.p.batch)]
            self.w, self.z, self.y = (np.concatenate([o[k_] for o in outs]) for k_ in ("w", "z", "y"))
        elif self.p.z_kind is not None:
            more, lv = {}, []
            if self.p.z_kind == "halfspace":
                more = dict(last_v=lv)
            elif self.p.z_kind == "cone":
                more = dict(kinds=self.z_stage_kinds)
            o = _REFS[self.p.z_kind].solve(self.p, rho=self.rho, z0=self.z, y0=self.y, **kw, **more)
            self.w, self.z, self.y = o.w, o.z, o.y
            if lv:
                self.z_stage_kinds.append(tuple(int(x.sum()) for x in hr.stage_kinds(self.p, lv[0])))
            self._mark_edges()
        elif self.p.fuel is not None:
            o = fr.solve(self.p, rho=self.rho, z0=self.z, y0=self.y, **kw)
            self.w, self.z, self.y = o.w, o.z, o.y
        else:
            o = oc.solve(self.p, rho=self.rho, z0=self.z, y0=self.y, **kw)
            self.w, self.z, self.y = o["w"], o["z"], o["y"]
        self.iterations += k
        self.pair_form = not self.fused

    def _advance(self, k, every):
        """k iterations; every `every`-th of THIS call (0: none) evaluates residuals -- the last of those is kept."""
        j = (k // every) * every if every > 0 else 0
        if j >= 1:
            self._oracle(j - 1)
            z_old = self.z.copy()
            self._oracle(1)
            self.resid = ar.residuals(self.w, z_old, self.z, self.y, self.rho)
        self._oracle(k - j)

    def iterate(self, k):
        self._advance(int(k), 0)

    def run(self, k, residual_every=0):
        self._advance(int(k), int(residual_every))

    def profile(self, iters, residuals=True, mode=1):
        """admm_profile advances the state (include/admm_hip.h): modes 0 / 1 by `iters` iterations, mode 2 by 2 iters + 1, mode 3
        by one; modes 2 and 3 by one more, first, when the state is held as the (z, y) pair.  With `residuals` the last one
        evaluates them."""
        if mode in (2, 3) and not self.alternating:
            raise Refused(UNSUPPORTED, "the alternating-direction kernels are not enabled")
        if self.per_qp and mode != 1:
            raise Refused(UNSUPPORTED, "per-instance dynamics: mode 1 only")
        if self.p.z_kind is not None and mode != 0:
            raise Refused(UNSUPPORTED, "a handle with an extension of the z-update runs the unfused path only")
        k = {0: iters, 1: iters, 2: 2 * iters + 1, 3: 1}[mode] + (1 if mode in (2, 3) and self.pair_form else 0)
        self._advance(k, k if residuals else 0)
        if mode == 0:
            self.pair_form = True
        else:
            self.pair_form = False

    # ---- single steps -----------------------------------------------------------------------------------------------------
    def _bounds(self):
        return ar.expand_bounds(self.p.lo, self.p.hi, self.p.N, self.p.nb)

    def step_x(self):
        p = self.p
        rho = self.rho
        g = -(rho[:, None] if self.per_qp else rho) * (self.z - self.y)
        if p.q is not None:
            g = g + p.q
        if self.per_qp:
            self.w = np.concatenate([ar.x_update(ar.factor(p.A[b], p.B[b], p.Q, p.R, p.QN, rho[b], p.N), g[b:b + 1], p.x0[b:b + 1])
                                     for b in range(p.batch)])
        else:
            self.w = ar.x_update(ar.factor(p.A, p.B, p.Q, p.R, p.QN, rho, p.N), g, p.x0)

    def step_z(self, residuals=False):
        p = self.p
        if p.per_instance_bounds:
            raise Refused(UNSUPPORTED, "no standalone z kernel with per-instance bounds")
        lo, hi = self._bounds()
        un = ar.expand_unorm(p.unorm, p.N)
        if p.fuel is not None or p.z_kind is not None:
            wh = self.alpha * self.w + (1.0 - self.alpha) * self.z if self.alpha != 1.0 else self.w
            v = wh + self.y
            kap = fr.expand_fuel(p.fuel, p.N) / self.rho
            if p.z_kind == "soft":
                zn = sr.prox(v, lo, hi, un, kap, p.m, sr.expand_soft(p.soft, p.N, p.nb) / self.rho)
            elif p.z_kind == "consensus":
                zn = cs.prox(v, lo, hi, un, kap, p.m, int(p.consensus))
            elif p.z_kind == "halfspace":
                zn = hr.prox(v, lo, hi, un, kap, p.m, *hr.planes(p))
                self.z_stage_kinds.append(tuple(int(x.sum()) for x in hr.stage_kinds(p, v)))
            elif p.z_kind == "cone":
                zn = cn.prox(v, lo, hi, un, kap, p.m, *cn.cones(p))
                self.z_stage_kinds.append(cn.stage_kinds(p, v))
            else:
                zn = fr.prox(v, lo, hi, un, kap, p.m)
            yn = v - zn
        else:
            zn, yn = ar.z_update(self.w, self.z, self.y, lo, hi, self.alpha, None if p.unorm is None else un, p.m)
        if residuals:
            self.resid = ar.residuals(self.w, self.z, zn, yn, self.rho)
        self.z, self.y = zn, yn
        self.iterations += 1
        self.pair_form = True
        self._mark_edges()

    # ---- state changes ----------------------------------------------------------------------------------------------------
    def set_rho(self, rho_new):
        rho_new = float(rho_new)
        if not (rho_new > 0.0 and np.isfinite(rho_new)):
            raise Refused(INVALID, "rho")
        if self.per_qp:
            self.y = self.y * (self.rho / rho_new)[:, None]
            self.rho = np.full(self.p.batch, rho_new)
        else:
            if rho_new == self.rho:
                return
            self.y = self.y * (self.rho / rho_new)
            self.rho = rho_new
        self.pair_form = True

    def set_state(self, w=None, z=None, y=None):
        given = [np.asarray(a, np.float64) for a in (w, z, y) if a is not None]
        if any(not np.all(np.isfinite(a)) for a in given):
            raise Refused(INVALID, "non-finite entry in w, z or y")
        if w is not None:
            self.w = np.array(w, np.float64)
        if z is not None:
            self.z = np.array(z, np.float64)
        if y is not None:
            self.y = np.array(y, np.float64)
            self._edge[:] = False                # (the caller's y: the same numbers on both sides)
        if z is not None or y is not None:
            self.pair_form = True

    def update_instances(self, x0=None, q=None):
        rep = {}
        if x0 is not None:
            rep["x0"] = np.array(x0, np.float64)
        if q is not None:
            if self.p.q is None:
                raise Refused(INVALID, "handle was set up without q")
            rep["q"] = np.array(q, np.float64)
        if rep:
            self.p = dataclasses.replace(self.p, **rep)
            self._subs = None

    def update_problem(self, new):
        p = self.p
        if (new.N, new.n, new.m, new.batch) != (p.N, p.n, p.m, p.batch):
            raise Refused(INVALID, "N, n, m, batch must equal those of setup")
        if np.any(np.asarray(new.lo) > np.asarray(new.hi)):
            raise Refused(INVALID, "lo > hi")
        if (new.q is None) != (p.q is None) or (new.unorm is None) != (p.unorm is None) or new.per_instance != p.per_instance:
            raise Refused(INVALID, "problem class changed")
        if p.soft is not None:
            self._check_soft(new, p.soft, p.fuel)              # the control-row rule against the new problem
        if p.z_kind in ("halfspace", "cone"):                  # the open-box rule, with the stages of the handle's planes / cones
            self._check_box_open(new, self._stages(self._payload(p)[0], p.cone_g))
        # the handle's fuel weights, soft weights, groups, planes and cones stay in force
        self.p = dataclasses.replace(new, fuel=p.fuel, soft=p.soft, consensus=p.consensus, hs_a=p.hs_a, hs_b=p.hs_b, cone_c=p.cone_c,
                                     cone_p=p.cone_p, cone_g=p.cone_g)
        self._subs = None
        self.pair_form = True

    def set_fuel(self, fuel):
        if self.p.fuel is None:
            raise Refused(INVALID, "a fuel term cannot be added to a handle")
        fuel = np.asarray(fuel, np.float64)
        if not np.all(np.isfinite(fuel)) or np.any(fuel < 0):
            raise Refused(INVALID, "fuel must be finite and >= 0")
        if self.p.soft is not None:
            self._check_soft(self.p, self.p.soft, fuel)        # a stage that gains a weight must hold no finite soft weight on its control rows
        self.p = dataclasses.replace(self.p, fuel=fuel.copy())
        self.pair_form = True

    @staticmethod
    def _check_soft(p, soft, fuel):
        """validate_soft: no NaN, every weight >= 0, +inf on the control rows of a stage with a finite thrust bound or a positive
        fuel weight."""
        sw = sr.expand_soft(soft, p.N, p.nb).reshape(p.N, p.nb)
        if not np.all(sw >= 0.0):
            raise Refused(INVALID, "soft entries must be >= 0 (+inf = a hard row) and not NaN")
        shrink = np.isfinite(ar.expand_unorm(p.unorm, p.N)) | (fr.expand_fuel(fuel, p.N) > 0)
        if np.any(sw[shrink, :p.m] != np.inf):
            raise Refused(INVALID, "soft entries of the control rows must be +inf where unorm is finite or fuel is positive")

    def set_soft(self, soft):
        if self.p.soft is None:
            raise Refused(INVALID, "soft weights cannot be added to a handle")
        soft = np.asarray(soft, np.float64)
        self._check_soft(self.p, soft, self.p.fuel)
        self.p = dataclasses.replace(self.p, soft=soft.copy())

    # ---- half-spaces and approach cones -----------------------------------------------------------------------------------
    @staticmethod
    def _payload(p):
        return (p.hs_a, p.hs_b) if p.z_kind == "halfspace" else (p.cone_c, p.cone_p, p.cone_g)

    def _stages(self, axis, gamma=None):
        """halfspace_stages / cone_stages after the finite check: a'a (c'c) a normal number and, for a cone, gamma a positive normal
        number with 1 + gamma^2 finite, at every (QP, stage) whose axis is not 0 -> (N,) the stages with one for some QP."""
        a3 = np.asarray(axis, np.float64).reshape(-1, self.p.N, np.shape(axis)[-1])
        nz = np.any(a3 != 0.0, axis=2)
        tiny = np.finfo(np.float64).tiny
        with np.errstate(over="ignore", under="ignore"):
            nn = np.sum(a3 * a3, axis=2)
            if np.any(nz & ~((nn >= tiny) & np.isfinite(nn))):
                raise Refused(INVALID, "a'a / c'c of a stage is not a normal number")
            if gamma is not None:
                g2 = np.asarray(gamma, np.float64).reshape(-1, self.p.N)
                if np.any(nz & ~((g2 >= tiny) & np.isfinite(1.0 + g2 * g2))):
                    raise Refused(INVALID, "gamma must be a positive normal number with 1 + gamma^2 finite")
        return np.any(nz, axis=0)

    def _check_box_open(self, p, stages):
        """The open-box rule: state rows 0 .. nh - 1 of problem p unbounded at every stage of `stages`."""
        nh = np.shape(self._payload(self.p)[0])[-1]
        lo = np.broadcast_to(np.atleast_2d(p.lo), (p.N, p.nb))[:, p.m:p.m + nh]
        hi = np.broadcast_to(np.atleast_2d(p.hi), (p.N, p.nb))[:, p.m:p.m + nh]
        if np.any(lo[stages] != -np.inf) or np.any(hi[stages] != np.inf):
            raise Refused(INVALID, "state rows 0 .. nh - 1 must be unbounded at a stage with a plane / cone")

    def _set_payload(self, kind, fields, arrays):
        p = self.p
        if p.z_kind != kind:
            raise Refused(INVALID, f"the handle was not set up with {kind} data: none can be added")
        arrays = [np.array(a, np.float64) for a in arrays]
        if any(a.shape != np.shape(b) for a, b in zip(arrays, self._payload(p))):
            raise Refused(INVALID, "the form and nh of set-up are kept")
        if any(not np.all(np.isfinite(a)) for a in arrays):
            raise Refused(INVALID, "non-finite entry")
        self._check_box_open(p, self._stages(arrays[0], arrays[2] if kind == "cone" else None))
        self.p = dataclasses.replace(p, **dict(zip(fields, arrays)))

    def set_halfspace(self, a, b):
        """admm_set_halfspace*: new planes, same form and nh; the state and the factor stay."""
        self._set_payload("halfspace", ("hs_a", "hs_b"), (a, b))

    def set_cone(self, c, apex, gamma):
        """admm_set_cone*: new cones, same form and nh; the state and the factor stay."""
        self._set_payload("cone", ("cone_c", "cone_p", "cone_g"), (c, apex, gamma))

    def halfspace(self):
        if self.p.z_kind != "halfspace":
            raise Refused(INVALID, "the handle has no half-spaces")
        return tuple(np.array(a, np.float64) for a in self._payload(self.p))

    def cone(self):
        if self.p.z_kind != "cone":
            raise Refused(INVALID, "the handle has no approach cones")
        return tuple(np.array(a, np.float64) for a in self._payload(self.p))

    def _mark_edges(self):
        """The unclear-stage rule at a z-update (the module docstring): its input is z + y of its output."""
        p = self.p
        if p.z_kind not in ("halfspace", "cone"):
            return
        nh = np.shape(self._payload(p)[0])[-1]
        v = (self.z + self.y).reshape(p.batch, p.N, p.nb)[:, :, p.m:p.m + nh]
        scale = np.maximum(1.0, np.sqrt(np.sum(v * v, axis=2)))
        if p.z_kind == "halfspace":
            A, Bv = hr.planes(p)
            nn = np.sum(A * A, axis=2)
            act = nn != 0.0
            dist = np.abs(np.sum(A * v, axis=2) - Bv) / np.sqrt(np.where(act, nn, 1.0))
        else:
            C, Pa, G = cn.cones(p)
            act, s, r, _, _ = cn._coords(C, Pa, v)
            dist = np.abs(r - G * s) / np.sqrt(1.0 + G * G)
        self._edge = act & (dist <= 1e-6 * scale)

    def _report(self, kind, lam):
        p = self.p
        if p.z_kind != kind:
            raise Refused(INVALID, f"the handle was not set up with {kind} data")
        ref = hr if kind == "halfspace" else cn
        mx, cnt, lm = ref.report(p, self.w, self.y, self.rho)
        axis = (hr.planes(p) if kind == "halfspace" else cn.cones(p))[0]
        norm = np.sqrt(np.sum(axis * axis, axis=2))                          # (batch, N): |a_k| / |c_k|, 0 where the stage has none
        act = norm != 0.0
        y_inf = np.abs(self.y).max(axis=1)[:, None]
        small = (lm != 0.0) & (np.abs(lm) <= 1e-6 * np.maximum(1.0, self.rho * y_inf))
        unclear = act & (self._edge | small)
        self.plane_stages.append((int(act.sum()), int(unclear.sum())))
        return dict(max_violation=mx, n_active=cnt, lam=lm, with_lam=bool(lam), norm=norm, unclear=unclear.sum(axis=1))

    def halfspace_report(self, lam=False):
        """admm_get_halfspace_report* -> dict(max_violation, n_active, lam, with_lam: whether the caller asks for lam, norm: |a_k| per
        (QP, stage), unclear: per QP the stages whose exact decision rounding could flip)."""
        return self._report("halfspace", lam)

    def cone_report(self, lam=False):
        """admm_get_cone_report*: as halfspace_report, norm = |c_k|."""
        return self._report("cone", lam)

    def mpc_advance(self, plant=None, du=None, dx=None, x_meas=None, q_tail=None, tail="copy"):
        """admm_mpc_advance: u = z_u,0 + du, x0 <- x+ (the plant's, or x_meas), w, z, y and q one stage on -> dict(u=, x_next=)."""
        p = self.p
        if p.z_kind in ("consensus", "halfspace", "cone"):
            raise Refused(UNSUPPORTED, "not available on a scenario-consensus handle, nor on one with half-spaces or approach cones")
        if self.per_qp:
            raise Refused(UNSUPPORTED, "not available with per-instance dynamics")
        if x_meas is not None and (plant is not None or dx is not None):
            raise Refused(INVALID, "x_meas replaces the plant: Ap, Bp and dx must be absent with it")
        if q_tail is not None and p.q is None:
            raise Refused(INVALID, "q_tail on a handle that was set up without q")
        given = list(plant or ()) + [a for a in (du, dx, x_meas, q_tail) if a is not None]
        if any(not np.all(np.isfinite(np.asarray(a, np.float64))) for a in given):
            raise Refused(INVALID, "non-finite entry in an input")
        u = self.z[:, :p.m].copy() if du is None else self.z[:, :p.m] + du
        if x_meas is not None:
            xn = np.array(x_meas, np.float64)
        else:
            Ap, Bp = mpc.model_plant(p) if plant is None else plant
            xn = mpc.plant_step(p.x0, u, Ap, Bp, dx)
        q = None if p.q is None else mpc.shift_horizon(p.q, p.nb, tail, q_tail)
        self.p = dataclasses.replace(p, x0=xn, q=q)
        self._subs = None
        self.w, self.z, self.y = (mpc.shift_horizon(a, p.nb, tail) for a in (self.w, self.z, self.y))
        self.pair_form = True
        return dict(u=u, x_next=xn.copy())

    def opened(self):
        """The feasibility problem of the handle: the box of every row with a finite soft weight removed."""
        p = self.p
        if p.soft is None:
            return p
        fin = np.isfinite(np.broadcast_to(np.asarray(p.soft, np.float64), np.shape(p.lo)))
        return dataclasses.replace(p, lo=np.where(fin, -np.inf, p.lo), hi=np.where(fin, np.inf, p.hi), soft=None)

    def infeasibility(self, span=10, eps=1e-6, costates=False):
        """admm_probe_infeasibility: keeps y, runs `span` iterations as run(span, 0) does -> the reference's probe of the two y
        (nu left out without `costates`)."""
        span = int(span)
        if span < 1 or not (np.isfinite(eps) and eps >= 0.0):
            raise Refused(INVALID, "span must be >= 1, eps finite and >= 0")
        if self.per_qp or self.p.z_kind in ("consensus", "halfspace", "cone") or self.opt.precision_mode == PRECISION_MIXED:
            raise Refused(UNSUPPORTED, "per-instance dynamics, scenario consensus, half-spaces, approach cones and the mixed-precision mode have no probe")
        y0 = self.y.copy()
        self._advance(span, 0)                  # (the state afterwards is that of get; run(span, 0); get: a get leaves the form alone)
        ref = ir.probe(self.opened(), y0, self.y, span, eps)
        # mu = 0 and lambda = 0 decide between a number and +inf (sep, defect): clear when the value stands out of the rounding of y, or
        # is zero because every y entry that feeds it is -- state rows for mu (nu, and with it mu, is built from lambda^x alone), every
        # row for lambda
        m_, nb = self.p.m, self.p.nb
        clear = np.ones(self.p.batch, bool)
        for b in range(self.p.batch):
            both = np.stack([y0[b], self.y[b]]).reshape(2, self.p.N, nb)
            noise = 1e-9 * max(1.0, np.abs(both).max()) / span          # (ten times the tolerance of y, over span)
            for what, v, rows in (("mu_max>0", ref["mu_max"][b], both[:, :, m_:]), ("drift>0", ref["drift"][b], both)):
                if not (v > noise or (v == 0.0 and not rows.any())):
                    self.unclear.append((self.probes, what, b, float(v), noise))
                    clear[b] = False
            if ref["mu_max"][b] > 0.0:
                self.margins.append(("open<=eps*mu_max", float(ref["open"][b]), float(eps * ref["mu_max"][b])))
            if np.isfinite(ref["sep"][b]):
                self.margins.append(("sep<-eps", float(ref["sep"][b]), -float(eps)))
        self.probes += 1
        return dict(ref, costates=bool(costates), eps=float(eps), defect_clear=clear)

    # ---- solve ------------------------------------------------------------------------------------------------------------
    def solve_begin(self):
        B = self.p.batch
        self._it, self._nconv, self._rho_updates = 0, 0, 0
        self._status = np.zeros(B, np.int32)
        self._iters = np.full(B, self.opt.max_iter, np.int32)
        self._nupd = np.zeros(B, np.int64)

    def solve_step(self):
        """Up to and including the next checked iteration -> (iterations so far, converged QPs, R, S)."""
        o = self.opt
        if self._it >= o.max_iter:
            raise Refused(INVALID, "max_iter already reached")
        nxt = min((self._it // o.check_interval + 1) * o.check_interval, o.max_iter)
        k = nxt - self._it
        self._advance(k, k)
        self._it = nxt
        r, s, nw, nz, ny = self.resid
        L = self.p.L
        e_pri = np.sqrt(L) * o.eps_abs + o.eps_rel * np.maximum(nw, nz)
        e_dua = np.sqrt(L) * o.eps_abs + o.eps_rel * ny
        for b in np.flatnonzero(self._status == 0):
            self.margins.append(("r<=e_pri", float(r[b]), float(e_pri[b])))
            self.margins.append(("s<=e_dua", float(s[b]), float(e_dua[b])))
        newly = ar.converged(r, s, nw, nz, ny, L, o.eps_abs, o.eps_rel) & (self._status == 0)
        self._iters[newly] = nxt
        self._status[newly] = 1
        self._nconv = int(self._status.sum())
        R = S = 0.0
        for b in range(self.p.batch):            # the summation order of the oracle and of the library's host code
            if not self._status[b]:
                R += r[b] * r[b]
                S += s[b] * s[b]
        return nxt, self._nconv, R, S

    def _rule(self, rho, R, S):
        o = self.opt
        mu2 = o.adapt_mu ** 2
        self.margins.append(("R>mu2*S", float(R), float(mu2 * S)))
        self.margins.append(("S>mu2*R", float(S), float(mu2 * R)))
        if R > mu2 * S:
            return rho * o.adapt_tau
        if S > mu2 * R:
            return rho / o.adapt_tau
        return rho

    def solve_adapt(self, R, S):
        o = self.opt
        if not (o.adapt_interval > 0 and self._it % o.adapt_interval == 0 and self._it < o.max_iter):
            return False
        changed = False
        if self.per_qp:                         # the rule runs QP by QP: R = r_b^2, S = s_b^2, adapt_max counted per QP
            r, s = self.resid[0], self.resid[1]
            for b in range(self.p.batch):
                if self._status[b] or self._nupd[b] >= o.adapt_max:
                    continue
                new = self._rule(self.rho[b], r[b] * r[b], s[b] * s[b])
                if new != self.rho[b]:
                    self.y[b] = self.y[b] * (self.rho[b] / new)
                    self.rho[b] = new
                    self._nupd[b] += 1
                    self._rho_updates += 1
                    changed = True
        elif self._rho_updates < o.adapt_max:
            new = self._rule(self.rho, R, S)
            if new != self.rho:
                self.y = self.y * (self.rho / new)
                self.rho = new
                self._rho_updates += 1
                changed = True
        if changed:
            self.pair_form = True
        return changed

    def solve_end(self):
        r, s = (self.resid[0], self.resid[1]) if self._it > 0 else (None, None)
        self.info = dict(iters_run=self._it, n_converged=self._nconv, iters=self._iters.copy(), status=self._status.copy(),
                         r=None if r is None else r.copy(), s=None if s is None else s.copy(),
                         rho=float(np.max(self.rho)), rho_updates=int(self._rho_updates))
        return self.info

    def solve(self, max_steps=None):
        """admm_solve: the loop of include/admm_hip.h with local values (max_steps: leave it early, as a stepwise caller may)."""
        self.solve_begin()
        steps = 0
        while True:
            it, nconv, R, S = self.solve_step()
            steps += 1
            if nconv >= self.p.batch or it >= self.opt.max_iter or (max_steps is not None and steps >= max_steps):
                break
            self.solve_adapt(R, S)
        return self.solve_end()

    # ---- read-outs --------------------------------------------------------------------------------------------------------
    def get(self):
        return self.w, self.z, self.y

    def residuals(self):
        if self.resid is None:
            raise Refused(INVALID, "no residual-evaluating z step has run yet")
        return self.resid

    def rho_per_qp(self):
        return np.array(self.rho, np.float64) if self.per_qp else np.full(self.p.batch, self.rho)

    def certificate(self):
        if self.per_qp:
            raise Refused(UNSUPPORTED, "no certificate with per-instance dynamics")
        return cr.certificate(self.p, self.z, self.y, self.rho)

    def soft_report(self):
        """admm_get_soft_report -> dict(penalty, max_violation, n_violated, weight_sum: the sum of the finite weights)."""
        p = self.p
        if p.soft is None:
            raise Refused(INVALID, "the handle has no soft weights")
        pen, mx, cnt = sr.report(p, self.z)
        sw = sr.expand_soft(p.soft, p.N, p.nb)
        fin = np.isfinite(sw)
        # every finite-weight row: outside its box, inside it, or exactly on a bound with |y| away from s / rho
        lo, hi = self._bounds()
        z, y = self.z[:, fin], self.y[:, fin]
        lo, hi, kap = lo[fin], hi[fin], sw[fin] / self.rho
        clear = 1e-6 * max(1.0, np.abs(self.z).max())
        outside = np.maximum(lo - z, z - hi) > clear
        inside = np.minimum(z - lo, hi - z) > clear
        on = ((z == lo) | (z == hi)) & (np.abs(np.abs(y) - kap) > 1e-6 * np.maximum(np.abs(y), kap))
        self.soft_rows.append((int(fin.sum()) * p.batch, int((~(outside | inside | on)).sum())))
        return dict(penalty=pen, max_violation=mx, n_violated=cnt, weight_sum=float(sw[fin].sum()))

    def consensus(self):
        if self.p.consensus is None:
            raise Refused(INVALID, "the handle has no scenario groups")
        return cs.consensus_of(self.p, self.z)
