"""Seeded call sequences on solver handles (tests/test_gpu_sequences.py, tests/test_handle_model_host.py).

sequence(kind, seed) -> [(op, args), ...], fully determined by (kind, seed) through numpy.random.default_rng; the arguments are
small scalars (lengths, flags, seeds of arrays), so a failing test can print the list.  materialise() turns one op into the
concrete arrays both sides get, apply_model() runs it on the host model (tests/_handle_model.py).

The ops fall into seven classes -- odd iteration call, even iteration call, residual-evaluating call, state change, refused
call, read-out, solve.  The class of every op of a sequence follows a random Eulerian circuit of the complete directed graph
(loops included) over the classes of the kind: EVERY ordered pair of classes occurs as neighbours in every sequence (50 ops with
seven classes, 37 on the kind without a solve), and read-outs come where the circuit puts them, not after every op -- a read-out
brings the hidden state of a handle into its normal form.  Within a class the op and its arguments are drawn at random.

A kind with ext=True also draws the receding-horizon step (admm_mpc_advance*, a state change), the infeasibility probe (a class of its
own, "probe": an iteration call and a read-out at once -- 65 ops with eight classes), and, on a handle with soft weights or scenario
groups, admm_set_soft, the soft report and the consensus read-out, with the calls such handles refuse in the refused class.  There
the ops of a class are dealt from a shuffled deck, so that three seeds hold every one.  The kinds without the flag keep their
sequences to the bit (DIGESTS, asserted by tests/test_handle_model_host.py), and so do the kinds with it that predate PLANE_KINDS
(EXT_DIGESTS).

PLANE_KINDS are handles with one half-space or one approach cone per stage: admm_set_halfspace* / admm_set_cone* among the state
changes (stages gain and lose their plane / cone), admm_get_halfspace / admm_get_cone and the reports among the read-outs, and among
the refused calls the receding-horizon step, the probe, the fused profile, a payload with a NaN, with a plane / cone over a closed box
or with a slope <= 0, and an admm_update_problem that closes the box under a plane / cone in force.
"""
import dataclasses

import numpy as np

import admm_library_amd as pkg
from admm_library_amd import _abi

CLASSES = ("odd", "even", "resid", "change", "refused", "readout", "solve", "probe")
MAX_ITERATIONS = 200           # per sequence: the range over which test_config2_slice_many_iterations holds 1e-10
SOLVE = dict(eps_abs=1e-2, eps_rel=1e-2, max_iter=12, check_interval=4)
PROBE_EPS = 1e-6
ADAPT = dict(adapt_interval=4, adapt_mu=2.0, adapt_tau=2.0, adapt_max=16)
F = _abi


def _ltv(**kw):
    return lambda seed, dN=0: pkg.random_ltv(**dict(kw, N=kw["N"] + dN, seed=seed))


def _inst(**kw):
    return lambda seed, dN=0: pkg.random_instances(**dict(kw, N=kw["N"] + dN, seed=seed))


def _formation(seed, dN=0):
    return pkg.cw_formation(N=64 + dN, batch=17, seed0=20231004 + 1000 * (seed - 1))


def _fuel(seed, dN=0):
    p = pkg.random_ltv(N=37 + dN, n=6, m=3, batch=9, seed=seed, thrust_norm=True)
    w = np.random.default_rng(seed + 99).uniform(0.02, 0.3, p.N)
    return dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), w, 0.0))      # a weight only where the controls have no box


def _soft_box(batch):
    def make(seed, dN=0):
        from test_soft_host import random_soft
        p = pkg.random_ltv(N=33 + dN, n=6, m=3, batch=batch, seed=seed)
        return dataclasses.replace(p, soft=random_soft(p))                          # (the weights of every variant: a handle keeps its own)
    return make


SOFT_FUEL_STAGE = 8            # of _soft_fuel: no thrust bound, no fuel weight, an open control box and finite soft weights on it


def _soft_fuel(seed, dN=0):
    """_fuel with soft weights on the state rows, and one stage on which admm_set_fuel must refuse a weight."""
    from test_soft_host import random_soft
    p = _fuel(seed, dN)
    k, m = SOFT_FUEL_STAGE, p.m
    assert not np.isfinite(p.unorm[k]) and p.fuel[k] == 0.0
    lo, hi = p.lo.copy(), p.hi.copy()
    lo[k, :m], hi[k, :m] = -np.inf, np.inf
    sw = random_soft(p)
    sw[:, :m] = np.inf
    sw[k, :m] = 0.3
    return dataclasses.replace(p, lo=lo, hi=hi, soft=sw)


def _consensus(G, fuel=False, **kw):
    def make(seed, dN=0):
        p = pkg.random_ltv(**dict(kw, N=kw["N"] + dN, seed=seed, thrust_norm=fuel))
        if fuel:
            w = np.random.default_rng(seed + 99).uniform(0.02, 0.3, p.N)
            p = dataclasses.replace(p, fuel=np.where(np.isfinite(p.unorm), w, 0.0))
        return dataclasses.replace(p, consensus=G)
    return make


def _di(name):
    """tests/_infeas_cases.py's problem; the variants of admm_update_problem scale Q, R, QN only (the feasible set stays)."""
    def make(seed, dN=0):
        import _infeas_cases as ic
        p = getattr(ic, name)(N=12 + dN)
        c = 1.0 + 0.25 * (seed - 10)
        return dataclasses.replace(p, Q=p.Q * c, R=p.R * c, QN=p.QN * c)
    return make


def _soft_di(seed, dN=0):
    """di_position_box with the corridor soft (tests/test_gpu_soft.py: no QP is flagged then); admm_set_soft makes it hard again."""
    p = _di("di_position_box")(seed, dN)
    sw = np.full(p.lo.shape, np.inf)
    sw[:, p.m] = 5.0
    return dataclasses.replace(p, soft=sw)


def closed_stages(N):
    """The stages random_planes / random_cones leave without a plane / cone and with their box closed: every fourth from stage 2."""
    off = np.zeros(N, bool)
    off[2::4] = True
    return off


def dormant_stages(N):
    """Of the open stages, every third (from the second): no plane / cone at set-up, so that admm_set_* can give them one."""
    out = np.zeros(N, bool)
    out[np.flatnonzero(~closed_stages(N))[1::3]] = True
    return out


def _planes(base, what, nh, per_qp):
    """base(seed, dN) with one half-space / approach cone per stage on the first nh state rows (random_planes / random_cones: the box
    of every open stage opened, by the stage index alone, so every variant of admm_update_problem keeps the pattern), the dormant
    stages without one.  make.full: the same problem with the payload of every open stage, which admm_set_* perturbs."""
    def full(seed, dN=0):
        p = base(seed, dN)
        if what == "halfspace":
            from test_halfspace_host import random_planes
            return random_planes(p, nh, per_qp, seed=100 + seed)
        from test_cone_host import random_cones
        return random_cones(p, nh, per_qp, seed=100 + seed)

    def make(seed, dN=0):
        p = full(seed, dN)
        d = dormant_stages(p.N)
        if what == "halfspace":
            a, b = np.array(p.hs_a), np.array(p.hs_b)
            a[..., d, :] = 0.0
            b[..., d] = 0.0
            p = dataclasses.replace(p, hs_a=a, hs_b=b)
        else:
            c = np.array(p.cone_c)
            c[..., d, :] = 0.0
            p = dataclasses.replace(p, cone_c=c)
        p.validate()
        return p
    make.full = full
    return make


_FIRST = dict(N=33, n=6, m=3, batch=69, with_q=False)
_THRUST = dict(N=37, n=6, m=3, batch=9, thrust_norm=True)
_LEAN = dict(N=45, n=6, m=3, batch=67, with_q=False, state_bounds=False)

# make(seed, dN): the problem of variant `seed` (1 = set-up, others = admm_update_problem), dN: another horizon (a refused update)
# family: path()["kernel_family"] at set-up; alt: profile modes 2 / 3 are drawn; tol: iterates and residuals
KINDS = {
    "one_lane_alt": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA), family="one_lane_fp64",
                         alt=True, device_io=True),
    "one_lane_alt_relaxed": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, alpha=1.6, segments=4, flags=F.FLAG_NO_MFMA),
                                 family="one_lane_fp64", alt=True),
    "with_q_two_blocks": dict(make=_ltv(N=30, n=4, m=2, batch=300), opt=dict(rho=0.3, segments=4, **ADAPT)),
    "lean_xfree": dict(make=_ltv(N=45, n=6, m=3, batch=67, with_q=False, state_bounds=False),
                       opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA), family="one_lane_fp64", alt=True, lean=True),
    "plain_fused": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_ALTERNATE)),
    "plain_fused_chain": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_ALTERNATE | F.FLAG_SCAN_CHAIN)),
    "unfused": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_UNFUSED), unfused=True),
    "graph_replay": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA | F.FLAG_GRAPH),
                         family="one_lane_fp64", alt=True),
    "thrust_bound": dict(make=_ltv(**_THRUST), opt=dict(rho=0.3, segments=5, **ADAPT)),
    "fuel_thrust_bound": dict(make=_fuel, opt=dict(rho=0.3, segments=5), fuel=True),
    "mfma_fp64_formation": dict(make=_formation, opt=dict(rho=0.05, precision_mode=F.PRECISION_FP64_MFMA), family="mfma_fp64",
                                alt=True),
    "mfma_fp64_ltv": dict(make=_ltv(N=30, n=10, m=4, batch=5, with_q=False), seed0=3,
                          opt=dict(rho=0.3, segments=3, precision_mode=F.PRECISION_FP64_MFMA), family="mfma_fp64", alt=True),
    "mfma_default_formation": dict(make=_formation, opt=dict(rho=0.05), family="mfma_fp64", alt=True, seeds=(1, 2, 7)),
    "mixed": dict(make=_formation, opt=dict(rho=0.05, precision_mode=F.PRECISION_MIXED), family="mfma_mixed", tol=1e-5,
                  solve=False),
    "wide_one_lane": dict(make=_ltv(N=24, n=12, m=6, batch=3), seed0=6, opt=dict(rho=0.3, segments=4)),
    "pinst_lane_per_qp": dict(make=_inst(N=30, n=6, m=3, batch=70), opt=dict(rho=0.3, segments=5, **ADAPT), pinst=True,
                              device_io=True),
    "pinst_rows_over_lanes": dict(make=_inst(N=24, n=6, m=3, batch=9), opt=dict(rho=0.3), pinst=True,
                                  env={"ADMM_PI_ROWS": "1"}),
    "pinst_wide_one_segment": dict(make=_inst(N=20, n=12, m=6, batch=5), opt=dict(rho=0.3, segments=1), pinst=True),
    "pinst_wide_four_segments": dict(make=_inst(N=20, n=12, m=6, batch=5), opt=dict(rho=0.3, segments=4), pinst=True),
}
OLD_KINDS = tuple(KINDS)

# The kinds with the receding-horizon step and the probe (ext=True).  soft / consensus: such a handle runs the unfused path only.
# stationary_rows: the largest share of the probed QPs on which mu or lambda may be a rounding error of a stationary y (rows violated
# for good hold y = s / rho); elsewhere the committed seeds have none (tests/test_handle_model_host.py).
KINDS.update({
    # odd batch with a pad column; chunks of 8 rows, the last short and no multiple of 4; kappa under the adaptive rule
    "soft_box_relaxed": dict(make=_soft_box(69), opt=dict(rho=0.3, alpha=1.6, segments=4, zrows=8, **ADAPT), ext=True, soft=True,
                             unfused=True, family="one_lane_fp64", seeds=(2, 4, 8), stationary_rows=0.05),
    # block-structured chunks (two blocks each); admm_set_fuel and admm_set_soft interleaved
    "soft_fuel_thrust": dict(make=_soft_fuel, opt=dict(rho=0.3, segments=5, zrows=18), ext=True, soft=True, fuel=True, unfused=True,
                             family="one_lane_fp64", seeds=(2, 3, 4)),
    # kappa changing under a captured graph
    "soft_graph": dict(make=_soft_box(129), opt=dict(rho=0.3, alpha=1.6, segments=4, zrows=8, flags=F.FLAG_GRAPH), ext=True,
                       soft=True, unfused=True, family="one_lane_fp64", seeds=(3, 4, 7), stationary_rows=0.05),
    # groups inside one lane pair / wave
    "consensus_G3": dict(make=_consensus(3, N=33, n=6, m=3, batch=15), opt=dict(rho=0.3, alpha=1.6, segments=4, **ADAPT), ext=True,
                         consensus=True, unfused=True, family="one_lane_fp64"),
    # a group across a wave, pad columns; two blocks per chunk
    "consensus_G65_fuel": dict(make=_consensus(65, fuel=True, N=37, n=6, m=3, batch=195), opt=dict(rho=0.3, segments=5, zrows=18),
                               ext=True, consensus=True, fuel=True, unfused=True, family="one_lane_fp64"),
    # a group wider than a workgroup's tile (256 columns at m = 6): the two-pass route
    "consensus_wide": dict(make=_consensus(300, N=10, n=12, m=6, batch=600), opt=dict(rho=0.3), ext=True, consensus=True,
                           unfused=True, family="one_lane_fp64"),
    "one_lane_alt_ext": dict(make=_ltv(N=30, n=4, m=2, batch=300), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA),
                             family="one_lane_fp64", alt=True, device_io=True, ext=True, seeds=(1, 4, 6)),
    "lean_xfree_ext": dict(make=_ltv(**_LEAN), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA), family="one_lane_fp64", alt=True,
                           ext=True, seeds=(2, 4, 5)),
    "plain_fused_ext": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_ALTERNATE), ext=True),
    "unfused_ext": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_UNFUSED), unfused=True, ext=True,
                        seeds=(2, 3, 4)),
    "graph_replay_ext": dict(make=_ltv(**_FIRST), opt=dict(rho=0.3, segments=4, flags=F.FLAG_NO_MFMA | F.FLAG_GRAPH),
                             family="one_lane_fp64", alt=True, ext=True, seeds=(1, 2, 4)),
    "mfma_fp64_ext": dict(make=_formation, opt=dict(rho=0.05, precision_mode=F.PRECISION_FP64_MFMA), family="mfma_fp64", alt=True,
                          ext=True),
    "fuel_thrust_ext": dict(make=_fuel, opt=dict(rho=0.3, segments=5), fuel=True, ext=True),
    # flags of both values: infeasible QPs beside a feasible one (tests/_infeas_cases.py, rho = its RHO)
    "probe_di_position_box": dict(make=_di("di_position_box"), opt=dict(rho=1.0), ext=True),
    "probe_di_pinned": dict(make=_di("di_pinned"), opt=dict(rho=1.0), ext=True),
    # the probe's bound table after admm_set_soft: the corridor rows go from open to hard and back, the flags with them
    "soft_probe_corridor": dict(make=_soft_di, opt=dict(rho=1.0), ext=True, soft=True, unfused=True, hard_or_soft=True,
                                seeds=(5, 7, 8), stationary_rows=0.25),
})
NEW_KINDS = tuple(k for k in KINDS if k not in OLD_KINDS)

# Handles with one half-space / one approach cone per stage (plane="halfspace" / "cone"): the unfused path only, no receding-horizon
# step and no probe (seven classes, 50 ops).  Shapes follow the z kernel's geometry (the header of tests/test_gpu_cone.py: one lane =
# two adjacent QPs, 512 columns per workgroup, chunks of whole blocks).  unclear_stages (none needs it): the largest share of a
# report's plane / cone stages whose exact decision rounding could flip; without it the committed seeds have none.
_PLANE = dict(ext=True, unfused=True, family="one_lane_fp64")
_SHARED = dict(N=33, n=6, m=3, batch=69)
_WIDE = dict(N=12, n=4, m=2, batch=514)
for _what in ("halfspace", "cone"):
    KINDS.update({
        # odd batch with a pad column; chunks of 4 blocks, the last of one; rho changes inside a solve
        f"{_what}_shared_relaxed": dict(make=_planes(_ltv(**_SHARED), _what, 3, False),
                                        opt=dict(rho=0.3, alpha=1.6, segments=4, zrows=36, **ADAPT), plane=_what, **_PLANE),
        # plane / cone, thrust ball and fuel shrink in one block, two blocks per chunk; admm_set_fuel and admm_set_* interleaved
        f"{_what}_perqp_fuel": dict(make=_planes(_fuel, _what, 6 if _what == "halfspace" else 2, True),
                                    opt=dict(rho=0.3, segments=5, zrows=18), plane=_what, fuel=True, **_PLANE),
        # two workgroups along the batch; the payload replaced under a captured graph; the device forms and their scan kernel
        f"{_what}_perqp_graph": dict(make=_planes(_ltv(**_WIDE), _what, 2, True), opt=dict(rho=0.3, segments=3, flags=F.FLAG_GRAPH),
                                     plane=_what, device_io=True, **_PLANE),
    })
PLANE_KINDS = tuple(k for k in KINDS if KINDS[k].get("plane"))
for _kind, _seeds in {"halfspace_shared_relaxed": (3, 4, 5), "halfspace_perqp_graph": (1, 2, 4), "cone_perqp_fuel": (1, 2, 4),
                      "cone_perqp_graph": (1, 2, 15)}.items():
    KINDS[_kind]["seeds"] = _seeds          # (picked like the margins' seeds: every op dealt, no unclear stage in any report)
SEEDS = (1, 2, 3)

# sha256 of repr(sequence(kind, seed)) of the kinds with ext=True that predate the half-space and cone kinds, taken before those existed
EXT_DIGESTS = {
    ("soft_box_relaxed", 2): "a79dfea7cd8c848908d5f4aba7624a0782f5ddff81b3e2c57f8b901f07a10f62",
    ("soft_box_relaxed", 4): "9b979128716145f5aa47249af42625da98d7f4c3862f4950379303f9b5e42c33",
    ("soft_box_relaxed", 8): "e719f4e72c72f4aa6b6b9f98f2bab311b2a74ab205fd692832b25957e1b44e31",
    ("soft_fuel_thrust", 2): "40888f078fc73715fd582d7aaeab67645e92f8342a01668518cfbff1dde86a51",
    ("soft_fuel_thrust", 3): "b61c8c0fc85fc83f32a9343cb97cee9947bc9d92f627e5b56a7e80ae119ade25",
    ("soft_fuel_thrust", 4): "97482fe3cc53460b83f3d4f8318cce5b2b82592215d7ffb0876af0313d679e0b",
    ("soft_graph", 3): "3cd28bcd60e65e2d400080b00105b4e06bac07ae9b4af61b04c636284256be57",
    ("soft_graph", 4): "bd78ebededb92e184b834e4f8223ba5502772ba0549ac78261de9dbece3db02f",
    ("soft_graph", 7): "e0d43bb45afaaf75bace4ad798cec812150149ea522ca7574ba74297103763c8",
    ("consensus_G3", 1): "5c65371bcd9562f9bbc2aabe436dd41ec61eb70d5d9e858a03424ad906d380ad",
    ("consensus_G3", 2): "14c15a3adf9e3bdda0842f7d47b68b6b6259ddd7173cf6a4cc60aeb9e9d8a891",
    ("consensus_G3", 3): "fad0f72c403f63d26024c6d10bd0efe5d0924f3aa382055c50bdd43d0d7a45bb",
    ("consensus_G65_fuel", 1): "de1f862854cf3832c22fee4bc623fae1a1c977dba98233900e79f9485ccc3c9f",
    ("consensus_G65_fuel", 2): "2d7ccad980703906696ba7376c2822996d26236c03ea08fac9ebe21b356afae6",
    ("consensus_G65_fuel", 3): "c13e76680619b3e5d02b421d26fca9ca47619c9f25ec8b3d0a6b8f6f186d361e",
    ("consensus_wide", 1): "dab107bb75844dcc034d1a146241c5ca1415331d5e9ed8cc0263d4affa77a784",
    ("consensus_wide", 2): "c80db634f58dcec8e6c6e236bf48892c8fbd14ffd955755a57c42652051ffa14",
    ("consensus_wide", 3): "5e6884c1031c049e7562f4833a3c57efcd322f83cc9fcdef39ab5f02d0c7bf06",
    ("one_lane_alt_ext", 1): "64dbe59d27d88b226f16ec2b72cfb7734f1e7187deaf63a02df47e4aa861932e",
    ("one_lane_alt_ext", 4): "e8b21fa16c922c5a2c9ed564a419bc3f22d7c8a50ac5ef3656b0abe6689ffe4c",
    ("one_lane_alt_ext", 6): "23e8aaaefba67083732968ceaa1dc377f30b5e0d9a29002368e2916a627f96ea",
    ("lean_xfree_ext", 2): "c0c441bcd8d39eb718891ff8cbb39de7b55ec00b96bc1dec0c563870c2baa3aa",
    ("lean_xfree_ext", 4): "68f50a06a31944ec14deb8bed7c6c29708e0a8d5504881dd45bb83f7ec536271",
    ("lean_xfree_ext", 5): "03018861121ca932d021b9d49bfc84ed118bd067f159b6b313e6e09362f87331",
    ("plain_fused_ext", 1): "3e69c3c0ba2b7963d41979bee6e4d41a0d8b00d3b159eb30c385e48aeb7dc283",
    ("plain_fused_ext", 2): "3d8a3ec55f10893c14a35b55a193958e27b2b244130b7f2dddb7b11a473c3cb2",
    ("plain_fused_ext", 3): "ec2ff820e13a1e1d2a11aacdfed3fadfb8a4f6009c72efea6c46295e4b69536f",
    ("unfused_ext", 2): "618080c35e1384fa16084a090c05d1ab9aca4225da59e6201cad3739cbec32ca",
    ("unfused_ext", 3): "07522fe7eb12860b301bbc166decdc2e41661e9e0cab87e24b383197fb0b5ebc",
    ("unfused_ext", 4): "a6923277bd8f17c142323e43ac12d4d987100cf8770784316bb7a7027556ab63",
    ("graph_replay_ext", 1): "229196d1923cf53b011150b62f9e404f40eaee128f4e7519a576ba6cd08d146e",
    ("graph_replay_ext", 2): "3dd18cda917f3d997ce88dcb9c99c25c9019432c4df6c386b16f01280775fa06",
    ("graph_replay_ext", 4): "a575facfd52c17145c686b0cc051e777382edf699f63580ddc37c2145acfd39c",
    ("mfma_fp64_ext", 1): "b36663cf22a9c130c3fa1fbee004585ab7b55b6b18e1d4fa09694517a1a42888",
    ("mfma_fp64_ext", 2): "24548eadcebb8a88934dccdb552da821c280143e1e7b29bb03e348a4d71ed73c",
    ("mfma_fp64_ext", 3): "67a57f888b3fb8cbd07497864cac89c2e4140cb9da72832398bded5892d2b418",
    ("fuel_thrust_ext", 1): "2a265cf097f0c67ce690afb3df9b3047aab0fbf64241f1544bfd04aa01900dd6",
    ("fuel_thrust_ext", 2): "9775153e6dc7189af66c836ffb60b8ea69c638f7e5a344c4288f8840a1662ea0",
    ("fuel_thrust_ext", 3): "de893e5870821877fe2ddd7bc4a7cd34637c27525c67c4803f0f9ecc743a2f4a",
    ("probe_di_position_box", 1): "1f0cb5ca5da7db45736d9e21d271c0d883565c925b19c63d6399d42588492f4b",
    ("probe_di_position_box", 2): "b04a54ceddc3bc3342985fc558ced499d8610b3debc2693a863faa0a9ff1fda0",
    ("probe_di_position_box", 3): "4a524cbffa1328ee720849f7e825a2a28463b7ef40ab7f20b08bac9cc7724d8c",
    ("probe_di_pinned", 1): "99178c69abe85bc70a0476ffbe5ba77e6d14f9aaa7e19a4eb090c83358feb34a",
    ("probe_di_pinned", 2): "f26efd454c877f236c949821e24c6a77c7d76f4a81ebfd03a140b0cf0e2cd854",
    ("probe_di_pinned", 3): "fb75ee51a3b869509693b9790a7948a726257d0de19f1054ba7d754c378d04da",
    ("soft_probe_corridor", 5): "ad053d1f883b9de7cbb46ea5a0daf539d252f329c31f2186ca9248241df7c830",
    ("soft_probe_corridor", 7): "239834c9dfebfef9c7093cbc8bbbc32f3b3dd3d9ac1062f335d16bc4eb95e01a",
    ("soft_probe_corridor", 8): "3a179b2a3ff4e25f7c62d682afbc1565cf5eb978f112349b6535d97ba688f0d6",
}

# sha256 of repr(sequence(kind, seed)) of the kinds that predate ext=True, taken before the flag existed: their sequences stay as they were
DIGESTS = {
    ("one_lane_alt", 1): "b7d292afd9bee50bb1a5e80a466960925ff812515f321ab4a308ab4d612fb04f",
    ("one_lane_alt", 2): "9dfceecdb88200105ac1a9d491da4381e27212f9d78e5fad031ffb0917522ce1",
    ("one_lane_alt", 3): "1981d8718250503de2263e14000c355a0774790a9daeb173ce5443fcc2cf4569",
    ("one_lane_alt_relaxed", 1): "ce3158f646e7acfdeb30c15716f1a7f0923d403dd4a9de7d26777412515b8647",
    ("one_lane_alt_relaxed", 2): "cc90c47a2360ba776e6b4c20e77738436afc4cffc3fe4cadaccc8d71a192138f",
    ("one_lane_alt_relaxed", 3): "3ed4f704a35f287bfc3fe8385dfd52f4386c585fb7a9a2e1b1eb8791deb0969b",
    ("with_q_two_blocks", 1): "6b777f0c2387304012e8d62eef9bd3164f644a19c0f8400855303700193712b1",
    ("with_q_two_blocks", 2): "94f187659063040c5ed3d8fb9d3bc39024cf35b420c4db94a247fda04dde6280",
    ("with_q_two_blocks", 3): "1c991e9925ec3480ea9edffd5b5472d37c51feb577fd5dbc136168eb3d7cde7b",
    ("lean_xfree", 1): "d844bbf7c47f7f3a68314704af92face44f64a114cb872760b119598ca7a43d4",
    ("lean_xfree", 2): "9e954c91e4105fa065a025567b7a2c8f02ff69195da808b96b3256ca51d61a22",
    ("lean_xfree", 3): "99445ec516f104fe534c13550ab74bfcd2846e66597d430cc98d2d9e798ec577",
    ("plain_fused", 1): "182ca7eef3a0ff4c13a00da512fb234fd1442ecb24195f82d22159122a4a4d00",
    ("plain_fused", 2): "875ad1286e36e25f2f9b12d3bf3d05f57a9c6689ec05de4c8b16f3df1315d0e5",
    ("plain_fused", 3): "18402256e2df58ad210da1b2c7067821b4fcb85e598a9dc5ed365e78b0d4eb4d",
    ("plain_fused_chain", 1): "c1547ade80256d3b97ec3e7257926490213a3854354df85c50e5ab7451baa2bd",
    ("plain_fused_chain", 2): "00380f76e1c8d850f2708482aa48b995def2ea3a759f6b440806810aeaf73d9e",
    ("plain_fused_chain", 3): "da07d86a83cd819dde627343416f26d259d61045ef47e0ab5287ea15ba0c4e8a",
    ("unfused", 1): "cba584be7ccf8a443ada5921312a26ed0c0aeffc3cffe681a9b45b92ec7c839a",
    ("unfused", 2): "ec5830c30cba5b6235c7d92f73a3272a8f85c5479777d53d5958cedc58a4c953",
    ("unfused", 3): "821ea96050213ba80f9ffbb6d774be24036ebea26e3b68b6df1abee9def99508",
    ("graph_replay", 1): "16e0df7119369fffa703c0ec5e5f88a2a6eea484d2c485db4d9ad178f2359801",
    ("graph_replay", 2): "b6ffd9197d94d41aa08e1e00fa69aa1a11f6cbb6dda02bc488ba3ace0a1a65fb",
    ("graph_replay", 3): "d01ced0d1d6f42bb70f1789b5f35a92387d1fd11b864f25e35184c49a0698415",
    ("thrust_bound", 1): "482e3a2055ab032d6db0275ccfe31179c63b669e056b6f00c48178c7175db581",
    ("thrust_bound", 2): "461a69dc04e0b9829d98d23861e68dfc132801783d884ff7971a039b4e39ab0a",
    ("thrust_bound", 3): "0f5e2692b8e9715ff693961e12e55ad7e7e0d207dea615495aeb3d57d0f7b3e9",
    ("fuel_thrust_bound", 1): "210c33cb54395c1fdf544a7555f300a64278ba4fc179b54ad2b34b171e229a5f",
    ("fuel_thrust_bound", 2): "22592783fb857afa8d58d82508be7ab16e18b887c33169599855b2e2dc1ab637",
    ("fuel_thrust_bound", 3): "e5bcd190a5307f8576726c0ec6cbb162508925278d7eb79594ad44dfe0e19718",
    ("mfma_fp64_formation", 1): "d99a8a888467e27ff67672f6dbcd28a8090c944777235b32eaa0c7b65a189e98",
    ("mfma_fp64_formation", 2): "dae367351034dfc21e0bd0e3b2d62e61af812d2e1c08146a693e0057ac9c0401",
    ("mfma_fp64_formation", 3): "da5e84bd5c08e0e89b34c8a4124581819318935eb2a9b5aafa2dd92adf6d21ef",
    ("mfma_fp64_ltv", 1): "2af6f95d45f90306a216925e564c5534e39635afe6b37385988601105529a235",
    ("mfma_fp64_ltv", 2): "6152f861d787fbd9c401723be46243bb9bf3f748e50f4bf60d4b0c8e6e3af6b3",
    ("mfma_fp64_ltv", 3): "2d7b7342665890ae61a7e2cf703d296744aca6371e25c22369058fd319d3b299",
    ("mfma_default_formation", 1): "feb61ed4a8784e8447e1df26ad54ef90381ebafd87fb5216dd8b6bbc4bec0e4d",
    ("mfma_default_formation", 2): "1f56c1bbb20a0617671552a9e8fbae7fc110e3746368ff2b36bbf5f843284a81",
    ("mfma_default_formation", 7): "417d6823c9ecdad299516f8e86c477ca0d20f3e854e0d6db76f48a63a4d69da4",
    ("mixed", 1): "2cb39949c4a2ed8c05e37fa057c48c2f9d7f7345b5d64f5f340a235a103f183e",
    ("mixed", 2): "cc1ba6becc6f9e7bd29b13e967fb079ca94da19c685a6c29bf74d451c31997b5",
    ("mixed", 3): "73cd11b292fe0ba3e45e429ec606be7584f22ff9356a7d659a19c1d527d38a0b",
    ("wide_one_lane", 1): "7164f98ed3128560f7d847337685bf63691656f95c8eabeb9d28a42a6e2cbacb",
    ("wide_one_lane", 2): "b72e656eb9bf613503664da3d3b4f7d2c204a101fc5f9ba7a3a03fdab523fbed",
    ("wide_one_lane", 3): "cd8292921c3f8240f7e64fe90aa6cb2207e3d9a535bc1e32b392192af4c2a2b4",
    ("pinst_lane_per_qp", 1): "a6764bc413bd15aafa4bf7c998e5225dcf3383c9557a62e6bf7f1da05a48e727",
    ("pinst_lane_per_qp", 2): "b49d4876cd20e48b42cda34f8bf3a3d330f35b2f8c6f33947dd6e5ecabc370ab",
    ("pinst_lane_per_qp", 3): "936db52fdf2a5f0caa79053825f81e258fca660835b2c1521f49cb2287531dc7",
    ("pinst_rows_over_lanes", 1): "5239b62bec35a64032272e62e74858eeb5bb8d70d503a3f92b83022e3507d21e",
    ("pinst_rows_over_lanes", 2): "9eb8c1de7febcab5b14042ef15ecbe5677908c9d48e337072cc19f1b7d249161",
    ("pinst_rows_over_lanes", 3): "868165e93c8b269b068bbf2fe6450284c31ed5a72dee033a677de83ad776ae75",
    ("pinst_wide_one_segment", 1): "29e87dc7e2b7133cef601834cb00bd571d3c7580e4b4c66ee805b2d9ba5053ba",
    ("pinst_wide_one_segment", 2): "7cdd3a51f374849019e3a907ac5c114032e4d9ad1550867a90876257642a1c97",
    ("pinst_wide_one_segment", 3): "40a4c4a10d0cbd708cde5c132ce27f48a3ea444d57d99dff575742a3e6646c04",
    ("pinst_wide_four_segments", 1): "88db4cf859c9503ae4474d5edb4c0de441f275fda2208e7d9685a1fbdbbb675b",
    ("pinst_wide_four_segments", 2): "ff428057dff6896bcb610f43312a550f71faced116baa9c8a69d18ea55d5dd3d",
    ("pinst_wide_four_segments", 3): "c3f591889a53915b0000b1f5027e1f0bc16f3020d503665881880335ad13244a",
}


def seeds(kind):
    """The committed seeds of a kind: together they hold every op legal on it (tests/test_handle_model_host.py)."""
    return KINDS[kind].get("seeds", SEEDS)


CASES = [(kind, seed) for kind in KINDS for seed in seeds(kind)]


def problem(kind, variant=1, dN=0):
    cfg = KINDS[kind]
    return cfg["make"](cfg.get("seed0", 10) + variant - 1, dN)


def options(kind):
    return pkg.Options(**dict(SOLVE, **KINDS[kind]["opt"]))


def classes_of(kind):
    cfg = KINDS[kind]
    probe = cfg.get("ext", False) and not cfg.get("consensus") and not cfg.get("plane")     # (such handles refuse the probe)
    return tuple(c for c in CLASSES if (c != "solve" or cfg.get("solve", True)) and (c != "probe" or probe))


def legal_ops(kind):
    """{class: [op names]} of the kind -- what include/admm_hip.h allows on such a handle."""
    cfg = KINDS[kind]
    pinst, dev = cfg.get("pinst", False), cfg.get("device_io", False)
    ops = {
        "odd": ["iterate", "run"] + ([] if pinst else ["step_z"]) + ["profile"],
        "even": ["iterate", "run", "profile"],
        "resid": ["run", "profile"] + ([] if pinst else ["step_z"]),
        "change": ["step_x", "set_rho", "set_state", "update_instances", "update_problem"] + (["set_fuel"] if cfg.get("fuel") else [])
                  + (["set_state_device"] if dev else []),
        "refused": ["refuse_set_state_nan", "refuse_update_N", "refuse_update_lohi"] + (["refuse_set_fuel_neg"] if cfg.get("fuel") else []),
        "readout": ["get", "residuals", "rho_per_qp"] + ([] if pinst else ["certificate"]) + (["get_device"] if dev else []),
        "solve": ["solve", "solve_pieces"],
        "probe": [],
    }
    if cfg.get("ext"):
        soft, cons, x = cfg.get("soft", False), cfg.get("consensus", False), cfg.get("plane")
        if cons or x:
            ops["refused"] += ["refuse_mpc", "refuse_probe"]
        else:
            ops["change"] += ["mpc_advance"] + (["mpc_advance_device"] if dev else [])
            ops["probe"] = ["infeasibility"] + (["infeasibility_device"] if dev else [])
            ops["refused"] += ["refuse_mpc_xmeas_and_dx", "refuse_mpc_nan_du"] + ([] if problem_has_q(kind) else ["refuse_mpc_qtail_without_q"])
        if soft:
            ops["change"] += ["set_soft"]
            ops["readout"] += ["soft_report", "soft_report_device"]
            ops["refused"] += ["refuse_set_soft_neg"] + (["refuse_set_fuel_on_soft_rows"] if cfg.get("fuel") else [])
        if cons:
            ops["readout"] += ["consensus", "consensus_device"]
        if x:                                                                   # x = "halfspace" / "cone"
            ops["change"] += [f"set_{x}"] + ([f"set_{x}_device"] if dev else [])
            ops["readout"] += [f"get_{x}", f"{x}_report", f"{x}_report_device"]
            refusals = [f"refuse_set_{x}_closed_box", f"refuse_set_{x}_nan"] + (["refuse_set_cone_gamma"] if x == "cone" else [])
            ops["refused"] += refusals + ["refuse_update_closed_box"] + ([r + "_device" for r in refusals] if dev else [])
        if soft or cons or x:
            ops["refused"] += ["refuse_profile_fused"]
    return {c: ops[c] for c in classes_of(kind)}


def _circuit(rng, classes):
    """Random Eulerian circuit (Hierholzer) of the complete digraph with loops on `classes`: len(classes)^2 + 1 nodes."""
    out = {c: [classes[i] for i in rng.permutation(len(classes))] for c in classes}
    stack, walk = [classes[int(rng.integers(len(classes)))]], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def sequence(kind, seed):
    cfg = KINDS[kind]
    rng = np.random.default_rng([seed, sum(map(ord, kind))])
    walk = _circuit(rng, classes_of(kind))
    ops_of = legal_ops(kind)
    profile_modes = [0] if cfg.get("unfused") else [1, 2, 3] if cfg.get("alt") else [1]
    cost = {"odd": 1, "even": 2, "resid": 1, "solve": SOLVE["max_iter"], "probe": 1}        # the least an op of the class applies
    used, seq = 0, []
    deck = {c: [] for c in ops_of}
    for i, cls in enumerate(walk):
        reserve = sum(cost.get(c, 0) for c in walk[i + 1:])
        room = MAX_ITERATIONS - used - reserve
        if cfg.get("ext"):                                                      # dealt from a shuffled deck of the class's ops
            if not deck[cls]:
                deck[cls] = [ops_of[cls][j] for j in rng.permutation(len(ops_of[cls]))]
            name = deck[cls].pop()
        else:
            name = ops_of[cls][int(rng.integers(len(ops_of[cls])))]
        k = int(rng.integers(1, 10))                                            # lengths 1 .. 9: both parities
        if cls == "odd":
            k = k if k % 2 else k - 1 if k > 1 else 1
        elif cls == "even":
            k = k + 1 if k % 2 else k
            k = min(k, 8)
        if cls in ("odd", "even", "resid") and k > room:
            k = 2 if cls == "even" else 1
        args = ()
        if name == "iterate":
            args = (k,)
        elif name == "run":
            if cls == "resid":
                every = (1, 2, k)[int(rng.integers(3))]
                every = min(every, k)
            else:
                every = 0 if k > 1 or rng.integers(2) else 2                    # run(1, 2): a residual interval that never comes
            args = (k, every)
        elif name == "step_z":
            k, args = 1, (cls == "resid",)
        elif name == "profile":
            if cls == "resid":
                mode = profile_modes[int(rng.integers(len(profile_modes)))]
                iters = 1 + int(rng.integers(2))
                k = {0: iters, 1: iters, 2: 2 * iters + 2, 3: 2}[mode]
                if k > room:
                    mode, iters, k = profile_modes[0], 1, 1
                args = (iters, True, mode)
            else:
                k = min(k, 4) if cls == "even" else min(k, 3)
                args = (k, False, profile_modes[0])
        elif name in ("solve", "solve_pieces"):
            k = SOLVE["max_iter"]
            args = () if name == "solve" else (int(rng.integers(3)),)           # steps before solve_end; 0: until done
        elif name == "set_rho":
            args = (float(np.round(4.0 ** rng.uniform(-1.0, 1.0), 3)),)         # within a factor of 4 of the start value
        elif name in ("set_state", "set_state_device"):
            mask = int(rng.integers(1, 8))
            args = (mask,) + tuple(float(x) for x in np.round(rng.uniform(0.5, 1.5, 3), 3))
        elif name == "update_instances":
            which = int(rng.integers(1, 4)) if problem_has_q(kind) else 1       # 1: x0, 2: q, 3: both
            args = (which, int(rng.integers(1 << 30)))
        elif name == "update_problem":
            args = (2 + int(rng.integers(4)),)
        elif name == "set_fuel":
            args = (float(np.round(rng.uniform(0.3, 2.0), 3)),)
        elif name == "certificate":
            args = (bool(rng.integers(2)),)
        elif name in ("get", "get_device"):
            args = (int(rng.integers(1, 8)),)
        elif name == "refuse_set_state_nan":
            args = (int(rng.integers(3)),)
        elif name in ("mpc_advance", "mpc_advance_device"):
            # (tail: 0 copy / 1 zero; x_meas in place of the plant; seeds of du, dx, the plant and q_tail, 0: absent)
            sd = [int(rng.integers(1, 1 << 30)) if rng.integers(2) else 0 for _ in range(4)]
            if name == "mpc_advance_device" and not sd[0]:
                sd[0] = 1 + int(rng.integers(1 << 30))                          # (the device form of the wrapper needs one tensor)
            if not problem_has_q(kind):
                sd[3] = 0
            args = (int(rng.integers(2)), int(rng.integers(3) == 0)) + tuple(sd)
        elif name in ("infeasibility", "infeasibility_device"):
            k = int(rng.integers(1, 7))
            k = k if k <= room else 1
            args = (k, bool(rng.integers(2)))
        elif name == "set_soft":
            args = (float(np.round(4.0 ** rng.uniform(-1.0, 1.0), 3)), int(rng.integers(1, 1 << 30)))
        elif name in SET_PLANE:
            args = (float(np.round(2.0 ** rng.uniform(-1.0, 1.0), 3)), int(rng.integers(1, 1 << 30)))     # a scale, the seed of the arrays
        elif name in PLANE_REPORTS:
            args = (bool(rng.integers(2)),)                                     # lam asked for
        elif name.startswith(("refuse_set_halfspace_nan", "refuse_set_cone_nan", "refuse_set_cone_gamma")):
            args = (int(rng.integers(2)),)                                      # which array holds the NaN; gamma = 0 or negative
        if cls in cost:
            used += k
        seq.append((name, args))
    return seq


def problem_has_q(kind):
    return problem(kind).q is not None


SET_PLANE = ("set_halfspace", "set_halfspace_device", "set_cone", "set_cone_device")
PLANE_REPORTS = ("halfspace_report", "halfspace_report_device", "cone_report", "cone_report_device")


def op_class(name, args):
    if name in ("solve", "solve_pieces"):
        return "solve"
    if name.startswith("refuse_"):
        return "refused"
    if name in ("infeasibility", "infeasibility_device"):
        return "probe"
    if name in ("get", "get_device", "residuals", "rho_per_qp", "certificate", "soft_report", "soft_report_device", "consensus",
                "consensus_device", "get_halfspace", "get_cone") + PLANE_REPORTS:
        return "readout"
    if name == "step_z":
        return "resid" if args[0] else "odd"
    if name == "profile":
        return "resid" if args[1] else ("odd" if args[0] % 2 else "even")
    if name == "run":
        k, every = args
        return "resid" if every and k // every >= 1 else ("odd" if k % 2 else "even")
    if name == "iterate":
        return "odd" if args[0] % 2 else "even"
    return "change"


# ---- from an op to what both sides are given ------------------------------------------------------------------------------

def initial_snapshot(kind, seed):
    """What set_state scales before the first read-out: small random arrays."""
    p = problem(kind)
    rng = np.random.default_rng([seed, 7])
    return tuple(0.1 * rng.standard_normal((p.batch, p.L)) for _ in range(3))


def materialise(kind, name, args, model, snap):
    """Concrete arguments of one op: arrays are built from the MODEL's problem and from `snap`, the model's (w, z, y) at the
    last state read-out, so the handle and the model are given the same numbers."""
    p = model.p
    if name in ("set_state", "set_state_device"):
        mask, scales = args[0], args[1:]
        out = {k: (snap[i] * scales[i] if mask >> i & 1 else None) for i, k in enumerate(("w", "z", "y"))}
        if p.consensus is not None and out["z"] is not None:                    # control rows that differ within a group
            out["z"] = out["z"] + 0.01 * np.random.default_rng(int(1000 * scales[1])).standard_normal(out["z"].shape)
        return out
    if name == "refuse_set_state_nan":
        arrs = {k: None for k in ("w", "z", "y")}
        a = snap[args[0]].copy()
        a[p.batch - 1, p.L // 2] = np.nan
        arrs[("w", "z", "y")[args[0]]] = a
        return arrs
    if name == "update_instances":
        which, s = args
        rng = np.random.default_rng(s)
        x0 = p.x0 * (1.0 + 0.2 * rng.standard_normal(p.x0.shape)) if which & 1 else None
        q = p.q * (1.0 + 0.2 * rng.standard_normal(p.q.shape)) + 0.02 * rng.standard_normal(p.q.shape) if which & 2 else None
        return dict(x0=x0, q=q)
    if name == "update_problem":
        return dict(problem=dataclasses.replace(problem(kind, args[0]), **_DROP))          # (the handle's weights, planes and cones stay in force)
    if name == "refuse_update_N":
        return dict(problem=dataclasses.replace(problem(kind, 2, dN=1), **_DROP))
    if name == "refuse_update_closed_box":          # a finite bound on a state row under a plane / cone in force
        new = dataclasses.replace(problem(kind, 2), **_DROP)
        live = np.flatnonzero(np.any(np.asarray(plane_payload(p)[0]).reshape(-1, p.N, plane_nh(p)) != 0.0, axis=(0, 2)))
        lo = np.array(new.lo, np.float64)
        lo[live[len(live) // 2], p.m + plane_nh(p) - 1] = -5.0
        return dict(problem=dataclasses.replace(new, lo=lo))
    if name == "refuse_update_lohi":
        new = dataclasses.replace(problem(kind, 2), **_DROP)
        lo = np.array(new.lo, np.float64, order="C")                            # (reshape(-1) below must be a view)
        finite = np.flatnonzero(np.isfinite(np.asarray(new.hi).reshape(-1)))
        k = int(finite[len(finite) // 2])                                       # one bounded row in the middle of the box
        lo.reshape(-1)[k] = np.asarray(new.hi).reshape(-1)[k] + 1.0
        return dict(problem=dataclasses.replace(new, lo=lo))
    if name == "set_fuel":
        return dict(fuel=np.asarray(problem(kind).fuel) * args[0])
    if name == "refuse_set_fuel_neg":
        f = np.array(p.fuel, np.float64)
        f[p.N // 3] = -0.1
        return dict(fuel=f)
    if name == "set_rho":
        return dict(rho=KINDS[kind]["opt"]["rho"] * args[0])
    if name in ("mpc_advance", "mpc_advance_device"):
        tail, meas, s_du, s_dx, s_plant, s_q = args
        B, n, m = p.batch, p.n, p.m
        gen = lambda s, shape, scale: scale * np.random.default_rng(s).standard_normal(shape) if s else None
        out = dict(tail=("copy", "zero")[tail], du=gen(s_du, (B, m), 0.05), q_tail=gen(s_q, (B, p.nb), 0.1), plant=None, dx=None,
                   x_meas=None)
        if meas:
            out["x_meas"] = p.x0 * (1.0 + gen(s_dx or 7, (B, n), 0.1)) + gen(s_plant or 11, (B, n), 0.02)
        else:
            out["dx"] = gen(s_dx, (B, n), 0.02)
            if s_plant:
                from admm_library_amd import mpc
                A0, B0 = mpc.model_plant(p)
                out["plant"] = (A0 * (1.0 + gen(s_plant, A0.shape, 0.05)), B0 * (1.0 + gen(s_plant + 1, B0.shape, 0.05)))
        return out
    if name in ("refuse_mpc_xmeas_and_dx", "refuse_mpc_nan_du", "refuse_mpc_qtail_without_q", "refuse_mpc"):
        out = dict(tail="copy", du=None, q_tail=None, plant=None, dx=None, x_meas=None)
        if name == "refuse_mpc_xmeas_and_dx":
            out.update(x_meas=np.array(p.x0, np.float64), dx=np.zeros((p.batch, p.n)))
        elif name == "refuse_mpc_nan_du":
            du = np.zeros((p.batch, p.m))
            du[p.batch - 1, p.m - 1] = np.nan
            out.update(du=du)
        elif name == "refuse_mpc_qtail_without_q":
            out.update(q_tail=np.zeros((p.batch, p.nb)))
        return out
    if name in ("set_soft", "refuse_set_soft_neg"):
        base = np.array(problem(kind).soft, np.float64)
        if name == "refuse_set_soft_neg":
            sw = np.array(p.soft, np.float64, order="C")
            fin = np.flatnonzero(np.isfinite(sw).reshape(-1))
            sw.reshape(-1)[fin[len(fin) // 2] if len(fin) else sw.size // 2] = -0.1
            return dict(soft=sw)
        if KINDS[kind].get("hard_or_soft"):                                     # every row hard, or the weights of set-up scaled
            return dict(soft=base * args[0] if args[1] % 2 else np.full_like(base, np.inf))
        rng = np.random.default_rng(args[1])
        pick = rng.uniform(size=base.shape)
        sw = base * args[0]                                                     # (+inf stays +inf)
        sw[pick < 0.1] = np.inf                                                 # some rows turned hard,
        sw[(pick > 0.9) & np.isfinite(base)] = 0.0                              # some ignored
        return dict(soft=sw)
    if name == "refuse_set_fuel_on_soft_rows":
        f = np.array(p.fuel, np.float64)
        f[SOFT_FUEL_STAGE] = 0.1
        return dict(fuel=f)
    if name in SET_PLANE:
        return dict(payload=new_payload(kind, *args))
    if name.startswith(("refuse_set_halfspace", "refuse_set_cone")):
        # the payload in force with one entry changed, in the last QP of the per-QP form
        arrs = [np.array(a, np.float64, order="C") for a in plane_payload(p)]
        N, nh = p.N, plane_nh(p)
        axis = arrs[0].reshape(-1, N, nh)                                        # (views of the copies)
        if "closed_box" in name:                    # a plane / cone on a stage whose box is closed
            k = int(np.flatnonzero(closed_stages(N))[1])
            axis[-1, k, 0] = 1.0
        elif "nan" in name:
            arrs[args[0]].reshape(-1)[arrs[args[0]].size - 1 - (N // 2) * (nh if args[0] == 0 else 1)] = np.nan
        else:                                       # the slope of a stage with a cone
            k = int(np.flatnonzero(np.any(axis[-1] != 0.0, axis=1))[-1])
            arrs[2].reshape(-1, N)[-1, k] = (0.0, -0.5)[args[0]]
        return dict(payload=tuple(arrs))
    return {}


_DROP = dict(fuel=None, soft=None, hs_a=None, hs_b=None, cone_c=None, cone_p=None, cone_g=None)


def plane_payload(p):
    """(a, b) / (c, apex, gamma) of a problem with half-spaces / approach cones."""
    return (p.hs_a, p.hs_b) if p.hs_a is not None else (p.cone_c, p.cone_p, p.cone_g)


def plane_nh(p):
    return int(np.shape(plane_payload(p)[0])[-1])


def new_payload(kind, scale, seed):
    """What admm_set_halfspace* / admm_set_cone* is given: the payload of every open stage (make.full) scaled and perturbed -- the
    signs and the zero entries of an axis stay -- then taken away from about a third of the open stages (dormant ones among them: the
    others of those gain one) and, in the per-QP form, from a tenth of the remaining (QP, stage) pairs."""
    cfg = KINDS[kind]
    full = cfg["make"].full(cfg.get("seed0", 10))
    rng = np.random.default_rng(seed)
    arrs = [np.array(a, np.float64) for a in plane_payload(full)]
    N = full.N
    gone = closed_stages(N) | (rng.uniform(size=N) < 0.3)
    axis = arrs[0] * scale * np.clip(1.0 + 0.1 * rng.standard_normal(arrs[0].shape), 0.5, 1.5)
    if cfg["plane"] == "halfspace":
        b = arrs[1] * scale + 0.05 * np.sqrt(np.sum(axis * axis, axis=-1)) * rng.standard_normal(arrs[1].shape)
        rest = [b]
    else:
        rest = [arrs[1] + 0.05 * rng.standard_normal(arrs[1].shape), arrs[2] * np.clip(1.0 + 0.1 * rng.standard_normal(arrs[2].shape), 0.5, 1.5)]
    off = np.broadcast_to(gone, axis.shape[:-1]).copy()
    if axis.ndim == 3:
        off |= rng.uniform(size=off.shape) < 0.1
    axis[off] = 0.0
    if cfg["plane"] == "halfspace":
        rest[0][off] = 0.0
    return (axis,) + tuple(rest)


def apply_model(model, name, args, concrete):
    """Run one op on the host model; returns what a read-out op reads (a dict), else None.  Raises _handle_model.Refused."""
    if name == "iterate":
        return model.iterate(args[0])
    if name == "run":
        return model.run(*args)
    if name == "step_x":
        return model.step_x()
    if name == "step_z":
        return model.step_z(args[0])
    if name == "profile":
        return model.profile(*args)
    if name == "solve":
        return dict(info=model.solve())
    if name == "solve_pieces":
        return dict(info=model.solve(max_steps=args[0] or None))
    if name == "set_rho":
        return model.set_rho(concrete["rho"])
    if name in ("set_state", "set_state_device", "refuse_set_state_nan"):
        return model.set_state(**concrete)
    if name == "update_instances":
        return model.update_instances(**concrete)
    if name in ("update_problem", "refuse_update_N", "refuse_update_lohi", "refuse_update_closed_box"):
        return model.update_problem(concrete["problem"])
    if name in ("set_fuel", "refuse_set_fuel_neg", "refuse_set_fuel_on_soft_rows"):
        return model.set_fuel(concrete["fuel"])
    if name in ("set_soft", "refuse_set_soft_neg"):
        return model.set_soft(concrete["soft"])
    if name in SET_PLANE or name.startswith(("refuse_set_halfspace", "refuse_set_cone")):
        return (model.set_halfspace if "halfspace" in name else model.set_cone)(*concrete["payload"])
    if name in ("get_halfspace", "get_cone"):
        return dict(payload=model.halfspace() if name == "get_halfspace" else model.cone())
    if name in PLANE_REPORTS:
        return dict(plane_report=(model.halfspace_report if "halfspace" in name else model.cone_report)(args[0]))
    if name in ("mpc_advance", "mpc_advance_device") or name.startswith("refuse_mpc"):
        return dict(mpc=model.mpc_advance(**concrete))
    if name in ("infeasibility", "infeasibility_device"):
        return dict(probe=model.infeasibility(args[0], PROBE_EPS, args[1]))
    if name == "refuse_probe":
        return dict(probe=model.infeasibility(3, PROBE_EPS, False))
    if name == "refuse_profile_fused":
        return model.profile(1, False, 1)
    if name in ("soft_report", "soft_report_device"):
        return dict(soft_report=model.soft_report())
    if name in ("consensus", "consensus_device"):
        return dict(consensus=model.consensus())
    if name == "certificate":
        return dict(cert=model.certificate())
    if name in ("get", "get_device"):
        w, z, y = model.get()
        return {k: a.copy() for i, (k, a) in enumerate(zip(("w", "z", "y"), (w, z, y))) if args[0] >> i & 1}
    if name == "residuals":
        return dict(resid=tuple(a.copy() for a in model.residuals()))
    if name == "rho_per_qp":
        return dict(rho_per_qp=model.rho_per_qp())
    raise KeyError(name)


def new_model(kind, alternating=None):
    from _handle_model import HandleModel
    cfg = KINDS[kind]
    return HandleModel(problem(kind), options(kind), alternating=cfg.get("alt", False) if alternating is None else alternating,
                       fused=not cfg.get("unfused", False))


def run_model(kind, seed):
    """The whole sequence on the host model -> (model, [(index, op, args, read-out or None, refused code or None)])."""
    from _handle_model import Refused
    model = new_model(kind)
    snap = initial_snapshot(kind, seed)
    log = []
    for i, (name, args) in enumerate(sequence(kind, seed)):
        concrete = materialise(kind, name, args, model, snap)
        try:
            out = apply_model(model, name, args, concrete)
            log.append((i, name, args, out, None))
        except Refused as e:
            log.append((i, name, args, None, e.code))
        if name in ("get", "get_device"):
            snap = tuple(a.copy() for a in model.get())
    return model, log
