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
"""
import dataclasses

import numpy as np

import admm_ref as ar
import oracle_c as oc
import _cert_ref as cr
import _consensus_ref as cs
import _fuel_ref as fr
import _infeas_ref as ir
import _soft_ref as sr
from admm_library_amd import mpc

PRECISION_MIXED = 1

INVALID, UNSUPPORTED, NUMERIC = 1, 2, 5


class Refused(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"refused ({code}): {why}")
        self.code = code


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
        self.fused = fused and problem.soft is None and problem.consensus is None    # (such handles run the unfused path only)
        self.pair_form = True        # the state is held as the (z, y) pair (admm_profile modes 2 / 3 then add one iteration)
        self.iterations = 0          # applied since set-up
        self.margins = []
        self.probes = 0              # probes so far
        self.unclear = []            # (probe, what, QP, value, rounding scale) of a zero / nonzero decision that rounding could flip
        self.soft_rows = []          # per soft report: (rows with a finite weight, rows of none of the three kinds)
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
            o = (sr if self.p.soft is not None else cs).solve(self.p, rho=self.rho, z0=self.z, y0=self.y, **kw)
            self.w, self.z, self.y = o.w, o.z, o.y
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
            raise Refused(UNSUPPORTED, "soft and scenario-consensus handles run the unfused path only")
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
        if p.fuel is not None or p.soft is not None or p.consensus is not None:
            wh = self.alpha * self.w + (1.0 - self.alpha) * self.z if self.alpha != 1.0 else self.w
            v = wh + self.y
            kap = fr.expand_fuel(p.fuel, p.N) / self.rho
            if p.soft is not None:
                zn = sr.prox(v, lo, hi, un, kap, p.m, sr.expand_soft(p.soft, p.N, p.nb) / self.rho)
            elif p.consensus is not None:
                zn = cs.prox(v, lo, hi, un, kap, p.m, int(p.consensus))
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
        # the handle's fuel weights, soft weights and groups stay in force
        self.p = dataclasses.replace(new, fuel=p.fuel, soft=p.soft, consensus=p.consensus)
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

    def mpc_advance(self, plant=None, du=None, dx=None, x_meas=None, q_tail=None, tail="copy"):
        """admm_mpc_advance: u = z_u,0 + du, x0 <- x+ (the plant's, or x_meas), w, z, y and q one stage on -> dict(u=, x_next=)."""
        p = self.p
        if p.consensus is not None:
            raise Refused(UNSUPPORTED, "not available on a scenario-consensus handle")
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
        if self.per_qp or self.p.consensus is not None or self.opt.precision_mode == PRECISION_MIXED:
            raise Refused(UNSUPPORTED, "per-instance dynamics, scenario consensus and the mixed-precision mode have no probe")
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
