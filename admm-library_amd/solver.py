"""ctypes binding of libadmm_hip.so and the host-side solver front end.

Mirrors the entry-point surface of include/admm_hip.h one to one
(`admm_setup` / `admm_solve` / ... keep their C names as methods or module
functions).  The reference defines no such surface (README.md:1-2 only), so
the names are this repository's own; a MATLAB caller gets the same surface
through matlab/admm_mex.cpp.

No CPU fallback: if the shared library is missing this module raises at load
time, and without a GPU `admm_setup` fails with ADMM_ERR_NO_DEVICE.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Optional

import numpy as np

from . import _abi
from ._abi import CInfo, COptions, CProblem, c_double_p, c_int32_p, dptr, iptr
from .problems import DeviceProblem, Problem, check_device_tensor

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libadmm_hip.so"
_lib = None


class AdmmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_abi.STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code


def library_path() -> str:
    """In-tree libadmm_hip.so; ADMM_HIP_LIB overrides it (A/B runs of kernel variants)."""
    return os.environ.get("ADMM_HIP_LIB") or os.path.join(_PKG_DIR, _LIB_NAME)


# name -> (restype, argtypes); every symbol include/admm_hip.h declares.
_SIGNATURES = {
    "admm_default_options": (None, [C.POINTER(COptions)]),
    "admm_setup": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions)]),
    "admm_update_instances": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "admm_set_state": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "admm_set_rho": (C.c_int, [C.c_void_p, C.c_double]),
    "admm_solve": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.POINTER(CInfo)]),
    "admm_solve_begin": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "admm_solve_step": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_double_p, c_double_p]),
    "admm_solve_adapt": (C.c_int, [C.c_void_p, C.c_double, C.c_double, c_int32_p]),
    "admm_solve_end": (C.c_int, [C.c_void_p, C.POINTER(CInfo)]),
    "admm_iterate": (C.c_int, [C.c_void_p, C.c_int32]),
    "admm_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "admm_get_lean_iterations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "admm_sync": (C.c_int, [C.c_void_p]),
    "admm_step_x": (C.c_int, [C.c_void_p]),
    "admm_step_z": (C.c_int, [C.c_void_p, C.c_int32]),
    "admm_get_residuals": (C.c_int, [C.c_void_p] + [c_double_p] * 5),
    "admm_get": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "admm_get_info": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_double_p, c_double_p]),
    "admm_profile": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p]),
    "admm_get_geometry": (C.c_int, [C.c_void_p] + [c_int32_p] * 4),
    "admm_get_rho": (C.c_int, [C.c_void_p, c_double_p]),
    "admm_get_history": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    "admm_get_path": (C.c_int, [C.c_void_p, C.POINTER(_abi.CPathInfo)]),
    "admm_get_scan_geometry": (C.c_int, [C.c_void_p] + [c_int32_p] * 4),
    "admm_setup_timeshard": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), C.c_int32, C.c_int32,
                                      _abi.EXCHANGE_FN, C.c_void_p]),
    "admm_get_window": (C.c_int, [C.c_void_p] + [c_int32_p] * 5),
    "admm_free": (None, [C.c_void_p]),
    "admm_last_error": (C.c_char_p, []),
    "admm_last_warning": (C.c_char_p, []),
    "admm_abi_version": (C.c_int, []),
    "admm_device_count": (C.c_int, []),
    "admm_record_sizes": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p]),
    "admm_host_scan_matrix": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, c_double_p, c_int32_p,
                                        c_int32_p, c_int32_p]),
    "admm_host_scan_packed": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, C.c_int32, c_double_p, c_int32_p, c_int32_p]),
    "admm_host_factor": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, c_double_p, c_double_p,
                                   c_double_p, c_double_p, c_double_p, c_int32_p]),
    "admm_host_scan_matrices_timeshard": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, C.c_int32, c_double_p, c_double_p,
                                                   c_int32_p]),
    "admm_update_problem": (C.c_int, [C.c_void_p, C.POINTER(CProblem)]),
    # minimum-fuel cost (ADMM_HIP_HAS_FUEL)
    "admm_setup_fuel": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), c_double_p]),
    "admm_set_fuel": (C.c_int, [C.c_void_p, c_double_p]),
    "admm_get_fuel": (C.c_int, [C.c_void_p, c_double_p]),
    # scenario consensus (ADMM_HIP_HAS_CONSENSUS): groups of QPs sharing one control profile
    "admm_setup_consensus": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), c_double_p, C.c_int32]),
    "admm_get_consensus": (C.c_int, [C.c_void_p, c_double_p]),
    "admm_get_consensus_device": (C.c_int, [C.c_void_p, c_double_p, C.c_void_p]),
    # soft box constraints (ADMM_HIP_HAS_SOFT): an exact L1 penalty on box violation per row
    "admm_setup_soft": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), c_double_p, c_double_p]),
    "admm_set_soft": (C.c_int, [C.c_void_p, c_double_p]),
    "admm_get_soft": (C.c_int, [C.c_void_p, c_double_p]),
    "admm_get_soft_report": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_int32_p]),
    "admm_get_soft_report_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_int32_p, C.c_void_p]),
    # one half-space per stage (ADMM_HIP_HAS_HALFSPACE): a linear inequality on the first nh state rows of every block
    "admm_setup_halfspace": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), c_double_p, c_double_p, c_double_p,
                                      C.c_int32, C.c_int32]),
    "admm_set_halfspace": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "admm_set_halfspace_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_get_halfspace": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "admm_get_halfspace_report": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_double_p]),
    "admm_get_halfspace_report_device": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_double_p, C.c_void_p]),
    # one approach cone per stage (ADMM_HIP_HAS_CONE): a second-order cone on the first nh state rows of every block
    "admm_setup_cone": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), c_double_p, c_double_p, c_double_p,
                                  c_double_p, C.c_int32, C.c_int32]),
    "admm_set_cone": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "admm_set_cone_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_get_cone": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "admm_get_cone_report": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_double_p]),
    "admm_get_cone_report_device": (C.c_int, [C.c_void_p, c_double_p, c_int32_p, c_double_p, C.c_void_p]),
    # device-memory forms (ABI v9): array pointers in the handle's GPU memory, the caller's hipStream_t last
    "admm_setup_device": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CProblem), C.POINTER(COptions), C.c_void_p]),
    "admm_update_problem_device": (C.c_int, [C.c_void_p, C.POINTER(CProblem), C.c_void_p]),
    "admm_update_instances_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_set_state_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_get_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_void_p]),
    # certificate: costates, objective, optimality measures (ADMM_HIP_HAS_CERTIFICATE)
    "admm_get_certificate": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "admm_get_certificate_device": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_void_p]),
    # infeasibility probe: a Farkas certificate per QP (ADMM_HIP_HAS_INFEASIBILITY)
    "admm_probe_infeasibility": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, c_double_p, c_double_p, c_double_p, c_int32_p,
                                          c_double_p]),
    "admm_probe_infeasibility_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, c_double_p, c_double_p, c_double_p, c_int32_p,
                                                 c_double_p, C.c_void_p]),
    # outer step of the batched SCvx loop on the device (ADMM_HIP_HAS_SCVX): device ordinal first, the caller's hipStream_t last
    "admm_scvx_rollout_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxModel), c_double_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_scvx_init_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxModel), C.POINTER(_abi.CScvxParams), c_double_p,
                                        C.POINTER(_abi.CScvxState), C.c_double, C.c_double, C.c_void_p]),
    "admm_scvx_prepare_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxModel), C.POINTER(_abi.CScvxParams), c_double_p,
                                           C.POINTER(_abi.CScvxState)] + [c_double_p] * 5 + [C.c_void_p]),
    "admm_scvx_advance_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxModel), C.POINTER(_abi.CScvxParams), c_double_p, c_double_p,
                                           C.POINTER(_abi.CScvxState), c_int32_p, C.c_void_p]),
    # ... with the model as an argument (ADMM_HIP_HAS_SCVX_MODELS): admm_scvx_dynamics in place of admm_scvx_model
    "admm_scvx_model_name": (C.c_char_p, [C.c_int32]),
    "admm_scvx_rollout_model_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxDynamics), c_double_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_scvx_init_model_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxDynamics), C.POINTER(_abi.CScvxParams), c_double_p,
                                              C.POINTER(_abi.CScvxState), C.c_double, C.c_double, C.c_void_p]),
    "admm_scvx_prepare_model_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxDynamics), C.POINTER(_abi.CScvxParams), c_double_p,
                                                 C.POINTER(_abi.CScvxState)] + [c_double_p] * 5 + [C.c_void_p]),
    "admm_scvx_advance_model_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxDynamics), C.POINTER(_abi.CScvxParams), c_double_p, c_double_p,
                                                 C.POINTER(_abi.CScvxState), c_int32_p, C.c_void_p]),
    # ... for a time-dependent model (ADMM_HIP_HAS_SCVX_STAGE_MODELS): admm_scvx_stage_dynamics, which carries the node table
    "admm_scvx_stage_model_name": (C.c_char_p, [C.c_int32]),
    "admm_scvx_rollout_stage_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxStageDynamics), c_double_p, c_double_p, c_double_p, C.c_void_p]),
    "admm_scvx_init_stage_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxStageDynamics), C.POINTER(_abi.CScvxParams), c_double_p,
                                              C.POINTER(_abi.CScvxState), C.c_double, C.c_double, C.c_void_p]),
    "admm_scvx_prepare_stage_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxStageDynamics), C.POINTER(_abi.CScvxParams), c_double_p,
                                                 C.POINTER(_abi.CScvxState)] + [c_double_p] * 5 + [C.c_void_p]),
    "admm_scvx_advance_stage_device": (C.c_int, [C.c_int32, C.POINTER(_abi.CScvxStageDynamics), C.POINTER(_abi.CScvxParams), c_double_p, c_double_p,
                                                 C.POINTER(_abi.CScvxState), c_int32_p, C.c_void_p]),
    # costates and the optimality certificate of the nonlinear problem (ADMM_HIP_HAS_SCVX_ADJOINT): no handle, no model
    "admm_scvx_adjoint_device": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_abi.CScvxParams)] + [c_double_p] * 4 +
                                 [C.POINTER(_abi.CScvxAdjointOut), C.c_void_p]),
    # receding-horizon step on the device (ADMM_HIP_HAS_MPC)
    "admm_mpc_advance": (C.c_int, [C.c_void_p, C.POINTER(_abi.CMpcStep), c_double_p, c_double_p]),
    "admm_mpc_advance_device": (C.c_int, [C.c_void_p, C.POINTER(_abi.CMpcStep), c_double_p, c_double_p, C.c_void_p]),
    "admm_record_sizes_alt": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "admm_host_factor_alt": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, c_double_p, c_double_p,
                                       c_double_p, c_int32_p]),
    "admm_record_alloc_check": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "admm_mfma_record_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "admm_host_factor_mfma": (C.c_int, [C.POINTER(CProblem), C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        c_int32_p]),
}


def load_library(path: Optional[str] = None):
    """Load libadmm_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or library_path()
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.admm_abi_version() != _abi.ABI_VERSION:
        raise RuntimeError("libadmm_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int):
    if rc != 0:
        msg = lib.admm_last_error().decode()
        if "non-finite entry in A, B" in msg or "non-finite entry in x0" in msg:    # what Problem.validate raises for small arrays (it leaves the large ones to the library)
            raise ValueError("non-finite problem data: " + msg)
        raise AdmmError(rc, msg)


def _on_gpu(a) -> bool:
    return getattr(a, "is_cuda", False) is True


def _tptr(t):
    """double* of a (checked) CUDA tensor; None -> NULL."""
    return c_double_p() if t is None else C.cast(C.c_void_p(t.data_ptr()), c_double_p)


def _stream(device):
    """The caller's stream of the device-memory entry points: torch's current stream on `device`.  torch's default stream is the
    null stream, which the library's non-blocking stream is not ordered against: it is synchronised here and passed as NULL (the
    caller vouches for its data) -- what torch has queued on it (copies, transposes of marshal_device_problem) is then complete."""
    import torch
    s = torch.cuda.current_stream(device)
    if not s.cuda_stream:
        s.synchronize()
    return C.c_void_p(s.cuda_stream)


def last_warning() -> str:
    """admm_last_warning(): what the last setup / set_rho / update_problem / solve call on this thread changed about the
    kernels a handle runs ('' = nothing) -- e.g. the forward-elimination gate of the default path failing."""
    return load_library().admm_last_warning().decode()


def device_count() -> int:
    return int(load_library().admm_device_count())


@dataclasses.dataclass
class Options:
    rho: float = 0.1
    alpha: float = 1.0
    eps_abs: float = 1e-6
    eps_rel: float = 1e-6
    max_iter: int = 4000
    check_interval: int = 10
    segments: int = 0
    device: int = -1
    zrows: int = 0
    flags: int = 0
    adapt_interval: int = 0
    adapt_max: int = 16
    adapt_mu: float = 10.0
    adapt_tau: float = 2.0
    precision_mode: int = 0       # _abi.PRECISION_FP64 / _MIXED / _FP64_MFMA

    def to_c(self) -> COptions:
        return _abi.make_options(**dataclasses.asdict(self))


@dataclasses.dataclass
class SolveInfo:
    iters_run: int
    n_converged: int
    max_r: float
    max_s: float
    solve_ms: float
    rho: float
    rho_updates: int
    mixed_iters: int
    iters: np.ndarray
    status: np.ndarray
    r: np.ndarray
    s: np.ndarray


@dataclasses.dataclass
class Certificate:
    """Solver.certificate(): per-QP objective, dynamics defect and stationarity defect of the handle's current (z, y) pair
    (DESIGN.md §2.9), and the costates nu_1 .. nu_N as (batch, N, n) if asked for.  NumPy arrays, or CUDA tensors on a solver
    built from a DeviceProblem."""
    obj: object
    feas_dyn: object
    stat: object
    nu: object = None


@dataclasses.dataclass
class Infeasibility:
    """Solver.infeasibility(): per-QP Farkas certificate from the drift of the scaled dual -- sep (negative
    beyond eps: proven infeasible; +inf: no ray), drift, defect, the flags (int32), and the ray costates nu_1 .. nu_N as
    (batch, N, n) if asked for.  NumPy arrays, or CUDA tensors on a solver built from a DeviceProblem."""
    sep: object
    drift: object
    defect: object
    infeasible: object
    nu: object = None


@dataclasses.dataclass
class SoftReport:
    """Solver.soft_report(): per QP, at the handle's z and over the rows with a finite soft weight: penalty =
    sum s_i dist_i, max_violation = max dist_i, n_violated = rows with dist_i > 0 (int32).  NumPy arrays, or CUDA tensors with
    device=True.  The total objective is Certificate.obj + penalty."""
    penalty: object
    max_violation: object
    n_violated: object


@dataclasses.dataclass
class HalfspaceReport:
    """Solver.halfspace_report(): per QP, max_violation = max_k (a_k . w_xi - b_k)+ / |a_k| on w of the last
    x-update, n_active = stages with a positive multiplier (int32), and with multipliers=True lam (batch, N) = rho (a_k . y_xi) /
    a_k . a_k, the multiplier of the stage's inequality (0 where the stage has no half-space).  NumPy arrays, or CUDA tensors with
    device=True."""
    max_violation: object
    n_active: object
    lam: object = None


@dataclasses.dataclass
class ConeReport:
    """Solver.cone_report(): per QP, max_violation = max_k (r_k - g_k s_k)+ / sqrt(1 + g_k^2) on w of the last
    x-update (the distance of w_xi from its cone), n_active = stages with a cone whose y_xi is not zero (int32), and with
    multipliers=True lam (batch, N) = rho |y_xi|_2, the size of the stage's multiplier (0 where the stage has no cone).  NumPy
    arrays, or CUDA tensors with device=True."""
    max_violation: object
    n_active: object
    lam: object = None


class Solver:
    """One handle = one batch of QPs on one GPU.

    Given a DeviceProblem (torch tensors on one GPU) it is set up through admm_setup_device, and update_problem(DeviceProblem),
    update_instances / set_state with CUDA tensors and get_device() use the device-memory entry points: the data stay on the GPU,
    ordered on torch's current stream.  NumPy arrays take the host entry points as before."""

    def __init__(self, problem, options: Optional[Options] = None, timeshard=None):
        """timeshard = (rank, nranks, exchange): a TIME-SHARDED handle (admm_setup_timeshard; sharding.TimeShardedSolver builds
        the exchange function over torch.distributed) -- `exchange` is an _abi.EXCHANGE_FN the caller keeps alive."""
        self._lib = load_library()
        self._h = C.c_void_p()
        self.problem = problem
        self.options = options or Options()
        co = self.options.to_c()
        on_device = isinstance(problem, DeviceProblem)
        if on_device:
            problem.validate()               # (ValueError for a DeviceProblem with a fuel term, groups or soft weights: no device-memory form)
            if timeshard is not None:
                raise ValueError("time-sharded handles take host arrays (admm_setup_timeshard has no device-memory form)")
            if co.device < 0:
                co.device = problem.device.index
            elif co.device != problem.device.index:
                raise ValueError(f"options.device = {co.device}, but the DeviceProblem lives on {problem.device}")
        # the handle's GPU, for the wrapper's checks of CUDA tensors (None: the current device at setup, asked for when needed)
        self.device_index = co.device if co.device >= 0 else None
        # per-instance dynamics: NumPy's row-major blocks go to the library as they are (ADMM_FLAG_ROW_MAJOR, transposed on the
        # device); ADMM_PY_COLMAJOR=1 keeps the host transposition (the column-major path of the ABI)
        self._row_major = bool(problem.per_instance and not os.environ.get("ADMM_PY_COLMAJOR"))
        if self._row_major:
            co.flags |= _abi.FLAG_ROW_MAJOR
        if on_device:
            cp, keep = _abi.marshal_device_problem(problem, self._row_major)
            _check(self._lib, self._lib.admm_setup_device(C.byref(self._h), C.byref(cp), C.byref(co), _stream(problem.device)))
        elif timeshard is None:
            cp, keep = _abi.marshal_problem(problem, self._row_major)
            keep["fuel"] = None if problem.fuel is None else _abi.marshal_fuel(problem)
            head = (C.byref(self._h), C.byref(cp), C.byref(co))
            kind = problem.z_kind                # (validate() has admitted at most one extension of the z-update)
            if kind == "cone":
                keep["cone_c"], keep["cone_p"], keep["cone_g"], nh, per_qp = _abi.marshal_cone(problem)
                rc = self._lib.admm_setup_cone(*head, dptr(keep["fuel"]), dptr(keep["cone_c"]), dptr(keep["cone_p"]), dptr(keep["cone_g"]),
                                               nh, int(per_qp))
            elif kind == "halfspace":
                keep["hs_a"], keep["hs_b"], nh, per_qp = _abi.marshal_halfspace(problem)
                rc = self._lib.admm_setup_halfspace(*head, dptr(keep["fuel"]), dptr(keep["hs_a"]), dptr(keep["hs_b"]), nh, int(per_qp))
            elif kind == "soft":
                keep["soft"] = _abi.marshal_soft(problem)
                rc = self._lib.admm_setup_soft(*head, dptr(keep["fuel"]), dptr(keep["soft"]))
            elif kind == "consensus":
                rc = self._lib.admm_setup_consensus(*head, dptr(keep["fuel"]), int(problem.consensus))
            elif keep["fuel"] is not None:
                rc = self._lib.admm_setup_fuel(*head, dptr(keep["fuel"]))
            else:
                rc = self._lib.admm_setup(*head)
            _check(self._lib, rc)
        else:
            cp, keep = _abi.marshal_problem(problem, self._row_major)
            if problem.fuel is not None:
                raise AdmmError(2, "a fuel term is not supported on time-sharded handles")
            if problem.consensus is not None:
                raise AdmmError(2, "scenario consensus is not supported on time-sharded handles")
            if problem.soft is not None:
                raise ValueError("soft constraints are not supported on time-sharded handles")
            if problem.hs_a is not None:
                raise ValueError("half-spaces are not supported on time-sharded handles")
            if problem.cone_c is not None:
                raise ValueError("approach cones are not supported on time-sharded handles")
            rank, nranks, fn = timeshard
            self._exchange = fn                     # the C side calls it for as long as the handle lives
            _check(self._lib, self._lib.admm_setup_timeshard(C.byref(self._h), C.byref(cp), C.byref(co), int(rank), int(nranks),
                                                            fn if fn is not None else _abi.EXCHANGE_FN(0), None))
        del keep
        self.batch, self.L = problem.batch, problem.L
        self._warn()

    def _warn(self):
        """Surface admm_last_warning() (the library never changes the kernel path silently)."""
        msg = self._lib.admm_last_warning().decode()
        self.last_warning = msg
        if msg:
            import warnings
            warnings.warn(msg, RuntimeWarning, stacklevel=3)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.admm_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- helpers ----------------------------------------------------------
    def _vec(self, a, rows=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != (self.batch, rows or self.L):
            raise ValueError(f"expected shape {(self.batch, rows or self.L)}, got {a.shape}")
        return a

    def _device(self):
        if self.device_index is None:
            import torch
            self.device_index = torch.cuda.current_device()
        return self.device_index

    def _tensors(self, **arrays):
        """The CUDA-tensor arguments of a device-memory call, checked (ValueError before the library is called); None stays None."""
        dev = f"cuda:{self._device()}"
        for name, (a, cols) in arrays.items():
            if a is not None:
                check_device_tensor(name, a, dev, (self.batch, cols))
        return dev

    # -- C ABI, one method per entry point -------------------------------
    def update_instances(self, x0=None, q=None):
        """x0 (batch, n), q (batch, L): NumPy arrays, or CUDA tensors on the handle's GPU (admm_update_instances_device)."""
        if _on_gpu(x0) or _on_gpu(q):
            dev = self._tensors(x0=(x0, self.problem.n), q=(q, self.L))
            _check(self._lib, self._lib.admm_update_instances_device(self._h, _tptr(x0), _tptr(q), _stream(dev)))
            return
        x0 = self._vec(x0, self.problem.n)
        q = self._vec(q)
        _check(self._lib, self._lib.admm_update_instances(self._h, dptr(x0), dptr(q)))

    def update_problem(self, problem):
        """New shared data (dynamics, weights, box, x0, q) on this handle; same N, n, m, batch.  A DeviceProblem on the handle's GPU
        goes through admm_update_problem_device."""
        import time
        if isinstance(problem, DeviceProblem):
            problem.validate()
            dev = f"cuda:{self._device()}"
            check_device_tensor("x0", problem.x0, dev)
            cp, keep = _abi.marshal_device_problem(problem, self._row_major)
            t0 = time.perf_counter()
            _check(self._lib, self._lib.admm_update_problem_device(self._h, C.byref(cp), _stream(dev)))
        else:
            if problem.fuel is not None or getattr(self.problem, "fuel", None) is not None:
                problem = self._keep_fuel(problem)
            if problem.soft is not None or getattr(self.problem, "soft", None) is not None:
                problem = self._keep_soft(problem)
            if problem.hs_a is not None or getattr(self.problem, "hs_a", None) is not None:
                problem = self._keep_halfspace(problem)
            if problem.cone_c is not None or getattr(self.problem, "cone_c", None) is not None:
                problem = self._keep_cone(problem)
            cp, keep = _abi.marshal_problem(problem, self._row_major)        # (validates)
            t0 = time.perf_counter()
            _check(self._lib, self._lib.admm_update_problem(self._h, C.byref(cp)))
        self.last_update_ms = (time.perf_counter() - t0) * 1e3      # the C call alone (validation, upload, refactor)
        del keep
        self.problem = problem
        self._warn()

    def _keep_fuel(self, problem):
        """update_problem on a handle with a fuel term: the handle's weights stay in force (admm_update_problem); the problem that
        becomes self.problem carries them, and the new box is validated against them."""
        import dataclasses
        if getattr(self.problem, "fuel", None) is None:
            raise ValueError("a fuel term cannot be added to a handle: set up a new Solver")
        cur = self.fuel()
        if problem.fuel is not None and not np.array_equal(np.broadcast_to(np.asarray(problem.fuel, np.float64), cur.shape), cur):
            raise ValueError("update_problem keeps the handle's fuel weights: change them with set_fuel")
        if problem.lo.ndim < 2 and np.any(cur != cur[0]):
            raise ValueError("per-stage fuel weights need per-stage bounds")
        return dataclasses.replace(problem, fuel=cur if problem.lo.ndim >= 2 else np.float64(cur[0]))

    def set_fuel(self, fuel):
        """New weights of the minimum-fuel term (scalar, or (N,) with per-stage bounds) on a handle set up with Problem.fuel:
        continuation in the weight, the state kept as a warm start (admm_set_fuel)."""
        import dataclasses
        cand = dataclasses.replace(self.problem, fuel=np.asarray(fuel, np.float64))
        cand.validate()
        _check(self._lib, self._lib.admm_set_fuel(self._h, dptr(_abi.marshal_fuel(cand))))
        self.problem = cand
        self._warn()

    def fuel(self) -> np.ndarray:
        """(N,) weights of the minimum-fuel term in force, per stage (zeros on a handle without the term)."""
        out = np.zeros(self.problem.N)
        _check(self._lib, self._lib.admm_get_fuel(self._h, dptr(out)))
        return out

    def _keep_soft(self, problem):
        """update_problem on a handle with soft weights: the handle's weights stay in force, per stacked row (admm_update_problem);
        the problem that becomes self.problem carries them, and the new problem is validated against them."""
        import dataclasses
        if getattr(self.problem, "soft", None) is None:
            raise ValueError("soft weights cannot be added to a handle: set up a new Solver")
        cur = self.soft()                                                     # (N, n + m)
        if problem.soft is not None and not np.array_equal(np.broadcast_to(np.asarray(problem.soft, np.float64), cur.shape), cur):
            raise ValueError("update_problem keeps the handle's soft weights: change them with set_soft")
        if problem.lo.ndim < 2 and np.any(cur != cur[0]):
            raise ValueError("per-stage soft weights need per-stage bounds")
        return dataclasses.replace(problem, soft=cur if problem.lo.ndim >= 2 else cur[0].copy())

    def set_soft(self, soft):
        """New weights of the soft box (the shape of lo / hi) on a handle set up with Problem.soft: continuation in the penalty, the
        state kept as a warm start (admm_set_soft)."""
        import dataclasses
        if getattr(self.problem, "soft", None) is None:
            raise AdmmError(1, "admm_set_soft: soft weights cannot be added to a handle (set Problem.soft)")
        cand = dataclasses.replace(self.problem, soft=np.asarray(soft, np.float64))
        cand.validate()
        _check(self._lib, self._lib.admm_set_soft(self._h, dptr(_abi.marshal_soft(cand))))
        self.problem = cand
        self._warn()

    def soft(self) -> np.ndarray:
        """(N, n + m) weights of the soft box in force, per stacked row (inf everywhere on a handle without weights)."""
        out = np.empty((self.problem.N, self.problem.nb))
        _check(self._lib, self._lib.admm_get_soft(self._h, dptr(out)))
        return out

    def soft_report(self, device: bool = False) -> SoftReport:
        """admm_get_soft_report: penalty, largest violation and number of violated rows of every QP at the handle's z, over the rows
        with a finite weight, computed on the device.  device=True returns CUDA tensors through admm_get_soft_report_device, ordered
        on torch's current stream."""
        if device:
            import torch
            dev = f"cuda:{self._device()}"
            pen, mx = (torch.empty(self.batch, dtype=torch.float64, device=dev) for _ in range(2))
            cnt = torch.empty(self.batch, dtype=torch.int32, device=dev)
            _check(self._lib, self._lib.admm_get_soft_report_device(self._h, _tptr(pen), _tptr(mx),
                                                                   C.cast(C.c_void_p(cnt.data_ptr()), c_int32_p), _stream(dev)))
            return SoftReport(pen, mx, cnt)
        pen, mx, cnt = np.empty(self.batch), np.empty(self.batch), np.empty(self.batch, np.int32)
        _check(self._lib, self._lib.admm_get_soft_report(self._h, dptr(pen), dptr(mx), iptr(cnt)))
        return SoftReport(pen, mx, cnt)

    def _keep_halfspace(self, problem):
        """update_problem on a handle with half-spaces: the handle's planes stay in force (admm_update_problem); the problem that
        becomes self.problem carries them, and the new box is validated against them."""
        if getattr(self.problem, "hs_a", None) is None:
            raise ValueError("half-spaces cannot be added to a handle: set up a new Solver")
        a, b = self.halfspace()
        if problem.hs_a is not None and not (np.array_equal(np.asarray(problem.hs_a, np.float64), a) and
                                             np.array_equal(np.asarray(problem.hs_b, np.float64), b)):
            raise ValueError("update_problem keeps the handle's half-spaces: change them with set_halfspace")
        return dataclasses.replace(problem, hs_a=a, hs_b=b)

    def _hs_form(self):
        """(nh, per_qp) of the handle's half-spaces; AdmmError on a handle without."""
        if getattr(self.problem, "hs_a", None) is None:
            raise AdmmError(1, "the handle has no half-spaces (set Problem.hs_a / hs_b)")
        return tuple(self.problem.hs_a.shape)[-1], len(self.problem.hs_a.shape) == 3

    def set_halfspace(self, a, b):
        """New planes a . xi <= b (the form and nh of Problem.hs_a / hs_b) on a handle set up with them -- the re-linearisation
        step of a keep-out loop; the state is kept as a warm start (admm_set_halfspace).  NumPy arrays, or CUDA tensors on the
        handle's GPU (admm_set_halfspace_device, ordered on torch's current stream; self.problem then keeps the tensors).  A
        refused call changes nothing."""
        nh, per_qp = self._hs_form()
        N = self.problem.N
        sa, sb = ((self.batch, N, nh), (self.batch, N)) if per_qp else ((N, nh), (N,))
        if _on_gpu(a) or _on_gpu(b):
            dev = f"cuda:{self._device()}"
            check_device_tensor("a", a, dev, sa)
            check_device_tensor("b", b, dev, sb)
            _check(self._lib, self._lib.admm_set_halfspace_device(self._h, _tptr(a), _tptr(b), _stream(dev)))
            self.problem = dataclasses.replace(self.problem, hs_a=a, hs_b=b)
            return
        a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
        if a.shape != sa or b.shape != sb:
            raise ValueError(f"set_halfspace keeps the handle's form: expected shapes {sa} and {sb}, got {a.shape} and {b.shape}")
        cand = dataclasses.replace(self.problem, hs_a=a, hs_b=b)
        cand.validate()
        _check(self._lib, self._lib.admm_set_halfspace(self._h, dptr(a), dptr(b)))
        self.problem = cand
        self._warn()

    def halfspace(self):
        """(a, b): the planes in force, in the shapes of Problem.hs_a / hs_b (admm_get_halfspace)."""
        nh, per_qp = self._hs_form()
        N = self.problem.N
        a = np.empty((self.batch, N, nh) if per_qp else (N, nh))
        b = np.empty((self.batch, N) if per_qp else (N,))
        _check(self._lib, self._lib.admm_get_halfspace(self._h, dptr(a), dptr(b)))
        return a, b

    def halfspace_report(self, multipliers: bool = False, device: bool = False) -> HalfspaceReport:
        """admm_get_halfspace_report: per QP the largest violation of a plane by w, the number of stages with a positive
        multiplier and, with multipliers=True, the multipliers (batch, N), computed on the device.  device=True returns CUDA
        tensors through admm_get_halfspace_report_device, ordered on torch's current stream."""
        N = self.problem.N
        if device:
            import torch
            dev = f"cuda:{self._device()}"
            mx = torch.empty(self.batch, dtype=torch.float64, device=dev)
            cnt = torch.empty(self.batch, dtype=torch.int32, device=dev)
            lam = torch.empty((self.batch, N), dtype=torch.float64, device=dev) if multipliers else None
            _check(self._lib, self._lib.admm_get_halfspace_report_device(self._h, _tptr(mx), C.cast(C.c_void_p(cnt.data_ptr()), c_int32_p),
                                                                        _tptr(lam), _stream(dev)))
            return HalfspaceReport(mx, cnt, lam)
        mx, cnt = np.empty(self.batch), np.empty(self.batch, np.int32)
        lam = np.empty((self.batch, N)) if multipliers else None
        _check(self._lib, self._lib.admm_get_halfspace_report(self._h, dptr(mx), iptr(cnt), dptr(lam)))
        return HalfspaceReport(mx, cnt, lam)

    def _keep_cone(self, problem):
        """update_problem on a handle with approach cones: the handle's cones stay in force (admm_update_problem); the problem that
        becomes self.problem carries them, and the new box is validated against them."""
        if getattr(self.problem, "cone_c", None) is None:
            raise ValueError("approach cones cannot be added to a handle: set up a new Solver")
        cur = self.cone()
        if problem.cone_c is not None and not all(np.array_equal(np.asarray(getattr(problem, k), np.float64), v)
                                                  for k, v in zip(("cone_c", "cone_p", "cone_g"), cur)):
            raise ValueError("update_problem keeps the handle's approach cones: change them with set_cone")
        return dataclasses.replace(problem, cone_c=cur[0], cone_p=cur[1], cone_g=cur[2])

    def _cone_form(self):
        """(nh, per_qp) of the handle's cones; AdmmError on a handle without."""
        if getattr(self.problem, "cone_c", None) is None:
            raise AdmmError(1, "the handle has no approach cones (set Problem.cone_c / cone_p / cone_g)")
        return tuple(self.problem.cone_c.shape)[-1], len(self.problem.cone_c.shape) == 3

    def set_cone(self, c, apex, gamma):
        """New cones (axis c, apex, slope gamma: the form and nh of Problem.cone_c / cone_p / cone_g) on a handle set up with them;
        the state is kept as a warm start (admm_set_cone).  NumPy arrays, or CUDA tensors on the handle's GPU (admm_set_cone_device,
        ordered on torch's current stream; self.problem then keeps the tensors).  A refused call changes nothing."""
        nh, per_qp = self._cone_form()
        N = self.problem.N
        sc, sg = ((self.batch, N, nh), (self.batch, N)) if per_qp else ((N, nh), (N,))
        if _on_gpu(c) or _on_gpu(apex) or _on_gpu(gamma):
            dev = f"cuda:{self._device()}"
            check_device_tensor("c", c, dev, sc)
            check_device_tensor("apex", apex, dev, sc)
            check_device_tensor("gamma", gamma, dev, sg)
            _check(self._lib, self._lib.admm_set_cone_device(self._h, _tptr(c), _tptr(apex), _tptr(gamma), _stream(dev)))
            self.problem = dataclasses.replace(self.problem, cone_c=c, cone_p=apex, cone_g=gamma)
            return
        c, apex, gamma = (np.ascontiguousarray(x, np.float64) for x in (c, apex, gamma))
        if c.shape != sc or apex.shape != sc or gamma.shape != sg:
            raise ValueError(f"set_cone keeps the handle's form: expected shapes {sc}, {sc} and {sg}, got {c.shape}, {apex.shape} and {gamma.shape}")
        cand = dataclasses.replace(self.problem, cone_c=c, cone_p=apex, cone_g=gamma)
        cand.validate()
        _check(self._lib, self._lib.admm_set_cone(self._h, dptr(c), dptr(apex), dptr(gamma)))
        self.problem = cand
        self._warn()

    def cone(self):
        """(c, apex, gamma): the cones in force, in the shapes of Problem.cone_c / cone_p / cone_g (admm_get_cone)."""
        nh, per_qp = self._cone_form()
        N = self.problem.N
        c, apex = (np.empty((self.batch, N, nh) if per_qp else (N, nh)) for _ in range(2))
        g = np.empty((self.batch, N) if per_qp else (N,))
        _check(self._lib, self._lib.admm_get_cone(self._h, dptr(c), dptr(apex), dptr(g)))
        return c, apex, g

    def cone_report(self, multipliers: bool = False, device: bool = False) -> ConeReport:
        """admm_get_cone_report: per QP the largest violation of a cone by w, the number of stages whose cone moved their rows and,
        with multipliers=True, rho |y_xi| per stage (batch, N), computed on the device.  device=True returns CUDA tensors through
        admm_get_cone_report_device, ordered on torch's current stream."""
        N = self.problem.N
        if device:
            import torch
            dev = f"cuda:{self._device()}"
            mx = torch.empty(self.batch, dtype=torch.float64, device=dev)
            cnt = torch.empty(self.batch, dtype=torch.int32, device=dev)
            lam = torch.empty((self.batch, N), dtype=torch.float64, device=dev) if multipliers else None
            _check(self._lib, self._lib.admm_get_cone_report_device(self._h, _tptr(mx), C.cast(C.c_void_p(cnt.data_ptr()), c_int32_p),
                                                                   _tptr(lam), _stream(dev)))
            return ConeReport(mx, cnt, lam)
        mx, cnt = np.empty(self.batch), np.empty(self.batch, np.int32)
        lam = np.empty((self.batch, N)) if multipliers else None
        _check(self._lib, self._lib.admm_get_cone_report(self._h, dptr(mx), iptr(cnt), dptr(lam)))
        return ConeReport(mx, cnt, lam)

    def set_rho(self, rho: float):
        _check(self._lib, self._lib.admm_set_rho(self._h, float(rho)))
        self._warn()

    def set_state(self, w=None, z=None, y=None):
        """(batch, L) each: NumPy arrays, or CUDA tensors on the handle's GPU (admm_set_state_device)."""
        if _on_gpu(w) or _on_gpu(z) or _on_gpu(y):
            dev = self._tensors(w=(w, self.L), z=(z, self.L), y=(y, self.L))
            _check(self._lib, self._lib.admm_set_state_device(self._h, _tptr(w), _tptr(z), _tptr(y), _stream(dev)))
            return
        w, z, y = self._vec(w), self._vec(z), self._vec(y)
        _check(self._lib, self._lib.admm_set_state(self._h, dptr(w), dptr(z), dptr(y)))

    def _info(self, ci: CInfo) -> SolveInfo:
        iters = np.empty(self.batch, np.int32)
        status = np.empty(self.batch, np.int32)
        r = np.empty(self.batch)
        s = np.empty(self.batch)
        _check(self._lib, self._lib.admm_get_info(self._h, iptr(iters), iptr(status), dptr(r), dptr(s)))
        return SolveInfo(ci.iters_run, ci.n_converged, ci.max_r, ci.max_s, ci.solve_ms, ci.rho, ci.rho_updates,
                         ci.mixed_iters, iters, status, r, s)

    def solve(self, z0=None, y0=None) -> SolveInfo:
        z0, y0 = self._vec(z0), self._vec(y0)
        ci = CInfo()
        _check(self._lib, self._lib.admm_solve(self._h, dptr(z0), dptr(y0), C.byref(ci)))
        self._warn()
        return self._info(ci)

    # admm_solve in pieces (global stop / adaptive-rho decisions of a sharded solve)
    def solve_begin(self, z0=None, y0=None):
        z0, y0 = self._vec(z0), self._vec(y0)
        _check(self._lib, self._lib.admm_solve_begin(self._h, dptr(z0), dptr(y0)))

    def solve_step(self, sums: bool = False):
        """Run up to and including the next checked iteration.
        Returns (iterations so far, converged QPs of this handle, R, S)."""
        it, nc = C.c_int32(), C.c_int32()
        R, S = C.c_double(), C.c_double()
        _check(self._lib, self._lib.admm_solve_step(self._h, C.byref(it), C.byref(nc),
                                                    C.byref(R) if sums else None, C.byref(S) if sums else None))
        return it.value, nc.value, R.value, S.value

    def solve_adapt(self, R: float, S: float) -> bool:
        ch = C.c_int32()
        _check(self._lib, self._lib.admm_solve_adapt(self._h, float(R), float(S), C.byref(ch)))
        return bool(ch.value)

    def solve_end(self) -> SolveInfo:
        ci = CInfo()
        _check(self._lib, self._lib.admm_solve_end(self._h, C.byref(ci)))
        self._warn()
        return self._info(ci)

    def iterate(self, iters: int, sync: bool = True):
        _check(self._lib, self._lib.admm_iterate(self._h, int(iters)))
        if sync:
            self.sync()

    def run(self, iters: int, residual_every: int = 0, sync: bool = True):
        _check(self._lib, self._lib.admm_run(self._h, int(iters), int(residual_every)))
        if sync:
            self.sync()

    def lean_iterations(self) -> int:
        """admm_get_lean_iterations: iterations launched so far in the lean residual form."""
        n = C.c_int64(0)
        _check(self._lib, self._lib.admm_get_lean_iterations(self._h, C.byref(n)))
        return int(n.value)

    def sync(self):
        _check(self._lib, self._lib.admm_sync(self._h))

    def step_x(self):
        _check(self._lib, self._lib.admm_step_x(self._h))

    def step_z(self, residuals: bool = False):
        _check(self._lib, self._lib.admm_step_z(self._h, int(bool(residuals))))

    def residuals(self):
        out = [np.empty(self.batch) for _ in range(5)]
        _check(self._lib, self._lib.admm_get_residuals(self._h, *[dptr(o) for o in out]))
        return tuple(out)

    def get(self, w=True, z=True, y=True):
        outs = [np.empty((self.batch, self.L)) if f else None for f in (w, z, y)]
        _check(self._lib, self._lib.admm_get(self._h, *[dptr(o) for o in outs]))
        return tuple(outs)

    def certificate(self, costates: bool = False) -> Certificate:
        """admm_get_certificate: objective (fuel term included), max dynamics defect and max stationarity defect of every QP at
        the current (z, y) pair with mu = rho y, computed on the device; costates=True adds the multipliers nu_{k+1} of the
        dynamics rows, (batch, N, n) -- B_k' nu_{k+1} is the primer vector.  A solver built from a DeviceProblem returns CUDA
        tensors through admm_get_certificate_device, ordered on torch's current stream."""
        N, n = self.problem.N, self.problem.n
        if isinstance(self.problem, DeviceProblem):
            import torch
            dev = f"cuda:{self._device()}"
            outs = [torch.empty(self.batch, dtype=torch.float64, device=dev) for _ in range(3)]
            nu = torch.empty((self.batch, N, n), dtype=torch.float64, device=dev) if costates else None
            _check(self._lib, self._lib.admm_get_certificate_device(self._h, *[_tptr(o) for o in outs], _tptr(nu), _stream(dev)))
            return Certificate(outs[0], outs[1], outs[2], nu)
        outs = [np.empty(self.batch) for _ in range(3)]
        nu = np.empty((self.batch, N, n)) if costates else None
        _check(self._lib, self._lib.admm_get_certificate(self._h, *[dptr(o) for o in outs], dptr(nu)))
        return Certificate(outs[0], outs[1], outs[2], nu)

    def consensus(self) -> np.ndarray:
        """admm_get_consensus: the control profile of each scenario group, (batch / group_size, N, m) -- the control rows of the
        group's z (equal, bit for bit, across the QPs of a group).  Only on a solver whose Problem has `consensus` set."""
        p = self.problem
        if getattr(p, "consensus", None) is None:
            raise AdmmError(1, "admm_get_consensus: the handle has no scenario groups (set Problem.consensus)")
        out = np.empty((self.batch // int(p.consensus), p.N, p.m))
        _check(self._lib, self._lib.admm_get_consensus(self._h, dptr(out)))
        return out

    def infeasibility(self, span: int = 10, eps: float = 1e-6, costates: bool = False) -> Infeasibility:
        """admm_probe_infeasibility: runs `span` iterations (as run(span) does) and turns the drift of the scaled dual over them
        into a Farkas certificate per QP, on the device: infeasible[b] = 1 proves -- up to rounding and `eps` -- that QP b has no
        point meeting its dynamics, box and thrust bounds; a feasible QP is never flagged, converged or not.  costates=True adds
        the ray costates, (batch, N, n).  A solver built from a DeviceProblem returns CUDA tensors through
        admm_probe_infeasibility_device, ordered on torch's current stream."""
        N, n = self.problem.N, self.problem.n
        if isinstance(self.problem, DeviceProblem):
            import torch
            dev = f"cuda:{self._device()}"
            outs = [torch.empty(self.batch, dtype=torch.float64, device=dev) for _ in range(3)]
            flag = torch.empty(self.batch, dtype=torch.int32, device=dev)
            nu = torch.empty((self.batch, N, n), dtype=torch.float64, device=dev) if costates else None
            _check(self._lib, self._lib.admm_probe_infeasibility_device(
                self._h, int(span), float(eps), *[_tptr(o) for o in outs], C.cast(C.c_void_p(flag.data_ptr()), c_int32_p),
                _tptr(nu), _stream(dev)))
            return Infeasibility(outs[0], outs[1], outs[2], flag, nu)
        outs = [np.empty(self.batch) for _ in range(3)]
        flag = np.empty(self.batch, np.int32)
        nu = np.empty((self.batch, N, n)) if costates else None
        _check(self._lib, self._lib.admm_probe_infeasibility(self._h, int(span), float(eps), *[dptr(o) for o in outs], iptr(flag),
                                                            dptr(nu)))
        return Infeasibility(outs[0], outs[1], outs[2], flag, nu)

    def get_device(self, w=True, z=True, y=True):
        """The state as (batch, L) fp64 tensors on the handle's GPU (None where not asked for), written by admm_get_device and
        ordered on torch's current stream: work queued on it afterwards sees them, without a host synchronisation."""
        import torch
        dev = f"cuda:{self._device()}"
        outs = [torch.empty((self.batch, self.L), dtype=torch.float64, device=dev) if f else None for f in (w, z, y)]
        _check(self._lib, self._lib.admm_get_device(self._h, *[_tptr(o) for o in outs], _stream(dev)))
        return tuple(outs)

    def mpc_advance(self, plant=None, du=None, dx=None, x_meas=None, q_tail=None, tail="copy"):
        """admm_mpc_advance: one receding-horizon step on the device.  Applies u = z_u,0 + du, sets
        x0 <- x+ = dx + Ap x0 + Bp u (or x_meas), and moves w, z, y (and q) one stage, the last block following `tail`
        ("copy" / "zero") or, for q, q_tail.  plant = (Ap, Bp) as (n, n), (n, m) NumPy arrays; None: the handle's A_0, B_0.
        du (batch, m), dx / x_meas (batch, n), q_tail (batch, n + m): NumPy arrays (host form) or CUDA tensors on the handle's
        GPU (admm_mpc_advance_device on torch's current stream).  Returns (u_applied, x_next) of the same kind."""
        n, m = self.problem.n, self.problem.m
        if tail not in _abi.MPC_TAILS:
            raise ValueError(f"tail must be one of {sorted(_abi.MPC_TAILS)}, got {tail!r}")
        keep = []
        if plant is not None:
            Ap, Bp = (np.asarray(a, np.float64) for a in plant)
            if Ap.shape != (n, n) or Bp.shape != (n, m):
                raise ValueError(f"plant: expected shapes {(n, n)} and {(n, m)}, got {Ap.shape} and {Bp.shape}")
            keep = [_abi._colmajor(Ap), _abi._colmajor(Bp)]
        step = _abi.CMpcStep(Ap=dptr(keep[0]) if keep else None, Bp=dptr(keep[1]) if keep else None,
                             tail=_abi.MPC_TAILS[tail], reserved=0)
        arrays = {"du": (du, m), "dx": (dx, n), "x_meas": (x_meas, n), "q_tail": (q_tail, n + m)}
        if any(_on_gpu(a) for a, _ in arrays.values()):
            import torch
            dev = self._tensors(**arrays)
            for k, (a, _) in arrays.items():
                setattr(step, k, _tptr(a))
            u = torch.empty((self.batch, m), dtype=torch.float64, device=dev)
            x = torch.empty((self.batch, n), dtype=torch.float64, device=dev)
            _check(self._lib, self._lib.admm_mpc_advance_device(self._h, C.byref(step), _tptr(u), _tptr(x), _stream(dev)))
            return u, x
        for k, (a, cols) in arrays.items():
            a = self._vec(a, cols)
            keep.append(a)
            setattr(step, k, dptr(a))
        u, x = np.empty((self.batch, m)), np.empty((self.batch, n))
        _check(self._lib, self._lib.admm_mpc_advance(self._h, C.byref(step), dptr(u), dptr(x)))
        return u, x

    def profile(self, iters: int, residuals: bool = True, fused: bool = True, alternating: bool = False,
                back_to_back: bool = False, lean: bool = False):
        """Per-kernel HIP-event timings (ms).  alternating: `iters` PAIRS of the alternating-direction
        iteration (forward form, backward form) instead of the plain kernels; with
        back_to_back each of the pair's kernels is launched `iters` times in a row between two events
        (admm_profile mode 3: no event-record bubble inside the averages); with lean the pairs run in the lean
        residual forms (mode 4; raises where they do not apply)."""
        ms = np.zeros(6)
        mode = (4 if lean else 3 if back_to_back else 2) if alternating else int(bool(fused))
        _check(self._lib, self._lib.admm_profile(self._h, int(iters), int(bool(residuals)), mode, dptr(ms)))
        if alternating:
            return {"xscan_ms": ms[0], "xfze_ms": ms[1], "finalize_xscan_ms": ms[2], "xbze_ms": ms[3],
                    "finalize_ms": ms[4], "pair_ms": ms[5]}
        if fused:
            return {"xb_ms": ms[0], "xscan_ms": ms[1], "xfz_ms": ms[2], "finalize_ms": ms[4], "iter_ms": ms[5]}
        return {"xb_ms": ms[0], "xscan_ms": ms[1], "xf_ms": ms[2], "zdual_ms": ms[3], "finalize_ms": ms[4],
                "iter_ms": ms[5]}

    def history(self) -> dict:
        """Residual history of the last solve (Options(flags=FLAG_HISTORY)): one entry per stopping test --
        iteration, n_converged, max_r, max_s (maxima over the batch), rho."""
        n = C.c_int32()
        _check(self._lib, self._lib.admm_get_history(self._h, 0, C.byref(n), None, None, None, None, None))
        it, nc = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        r, s, rho = np.empty(n.value), np.empty(n.value), np.empty(n.value)
        _check(self._lib, self._lib.admm_get_history(self._h, n.value, C.byref(n), iptr(it), iptr(nc), dptr(r), dptr(s), dptr(rho)))
        return {"iteration": it, "n_converged": nc, "max_r": r, "max_s": s, "rho": rho}

    def rho_per_qp(self) -> np.ndarray:
        """rho of every QP: the handle's rho for batch-shared dynamics; with per-instance dynamics each QP's own
        (the adaptive rule runs per QP there)."""
        out = np.empty(self.problem.batch)
        _check(self._lib, self._lib.admm_get_rho(self._h, dptr(out)))
        return out

    def geometry(self):
        v = [C.c_int32() for _ in range(4)]
        _check(self._lib, self._lib.admm_get_geometry(self._h, *[C.byref(x) for x in v]))
        return {"pitch": v[0].value, "segments": v[1].value, "zrows": v[2].value, "zchunks": v[3].value}

    def window(self) -> dict:
        """admm_get_window: the stages / segments this handle iterates (the whole horizon unless it is a time shard)."""
        v = [C.c_int32() for _ in range(5)]
        _check(self._lib, self._lib.admm_get_window(self._h, *[C.byref(x) for x in v]))
        return {"stage_lo": v[0].value, "stage_hi": v[1].value, "seg_lo": v[2].value, "segs_local": v[3].value, "segs_total": v[4].value}

    def scan_geometry(self) -> dict:
        """admm_get_scan_geometry: split-K factor, padded shape and row groups of the segment scan as a dense product (split 1 and
        zeros with per-instance dynamics)."""
        v = [C.c_int32() for _ in range(4)]
        _check(self._lib, self._lib.admm_get_scan_geometry(self._h, *[C.byref(x) for x in v]))
        return {"split": v[0].value, "M": v[1].value, "K": v[2].value, "groups": v[3].value}

    def path(self) -> dict:
        """admm_get_path: which kernels this handle runs and the measured margin of the default path."""
        pi = _abi.CPathInfo()
        _check(self._lib, self._lib.admm_get_path(self._h, C.byref(pi)))
        return {"alternating": bool(pi.alternating), "alt_requested": bool(pi.alt_requested),
                "kernel_family": _abi.KERNEL_FAMILIES[pi.mfma], "xfree": bool(pi.xfree), "segments": pi.segments,
                "auto_segments": bool(pi.auto_segments), "scan_form": _abi.SCAN_FORMS[pi.scan_form],
                "per_instance": bool(pi.per_instance), "alt_check": pi.alt_check, "alt_gate": pi.alt_gate,
                "scan_growth": pi.scan_growth}


def admm_setup(problem: Problem, options: Optional[Options] = None) -> Solver:
    """admm_setup of the C ABI: validate, factor the KKT system, upload."""
    return Solver(problem, options)


def admm_solve(problem_or_solver, options: Optional[Options] = None, z0=None, y0=None):
    """One-call front end: setup (if given a Problem) + solve + read-out.
    Returns (w, z, y, info)."""
    own = not isinstance(problem_or_solver, Solver)
    s = Solver(problem_or_solver, options) if own else problem_or_solver
    try:
        info = s.solve(z0, y0)
        w, z, y = s.get()
    finally:
        if own:
            s.close()
    return w, z, y, info


def host_factor(problem: Problem, rho: float, segments: int):
    """Host-only: the packed factor records exactly as admm_setup uploads them
    (no GPU needed).  Used by the CPU tests of the segment algebra."""
    lib = load_library()
    cp, keep = _abi.marshal_problem(problem)
    N, n, m = problem.N, problem.n, problem.m
    S = max(1, min(segments, N))
    rb, rf, rs = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.admm_record_sizes(n, m, C.byref(rb), C.byref(rf), C.byref(rs)))
    K = np.empty((N, m, n)); Sinv = np.empty((N, m, m))
    recB = np.empty((N, rb.value)); recF = np.empty((N, rf.value)); recS = np.empty((S, rs.value))
    seg = np.empty(S + 1, np.int32)
    _check(lib, lib.admm_host_factor(C.byref(cp), float(rho), S, dptr(K), dptr(Sinv), dptr(recB),
                                     dptr(recF), dptr(recS), iptr(seg)))
    M, Mt, Kd = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.admm_host_scan_matrix(C.byref(cp), float(rho), S, None, C.byref(M), C.byref(Mt), C.byref(Kd)))
    W = np.empty((M.value, Kd.value))
    _check(lib, lib.admm_host_scan_matrix(C.byref(cp), float(rho), S, dptr(W), None, None, None))
    out = {"K": K, "Sinv": Sinv, "recB": recB, "recF": recF, "recS": recS, "seg_start": seg,
           "scanW": W, "scanMt": Mt.value, "alt_ok": False}
    # records of the alternating-direction iteration
    rfe, rbe, ok = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.admm_record_sizes_alt(n, m, C.byref(rfe), C.byref(rbe)))
    recFE = np.empty((N, rfe.value)); recBE = np.empty((N, rbe.value)); WB = np.empty_like(W)
    _check(lib, lib.admm_host_factor_alt(C.byref(cp), float(rho), S, dptr(recFE), dptr(recBE), dptr(WB),
                                         C.byref(ok)))
    if ok.value:
        out.update(alt_ok=True, recFE=recFE, recBE=recBE, scanWB=WB)
    del keep
    return out


def host_scan_packed(problem: Problem, rho: float, segments: int, backward: bool = False):
    """Host-only: the segment-scan matrix in the fragment order xscan_mfma_kernel reads (flat, M * K doubles) and the k-step range
    [begin, end) of every row group, as (Wp, range (groups, 2), M, K); backward: the pair of the forward-elimination form (None,
    None, M, K when that form cannot be built)."""
    lib = load_library()
    cp, keep = _abi.marshal_problem(problem)
    sizes = np.zeros(4, np.int32)
    _check(lib, lib.admm_host_scan_packed(C.byref(cp), float(rho), int(segments), int(backward), None, None, iptr(sizes)))
    M, K, groups, ok = (int(v) for v in sizes)
    if not ok:
        return None, None, M, K
    Wp = np.empty(M * K)
    rng = np.empty((groups, 2), np.int32)
    _check(lib, lib.admm_host_scan_packed(C.byref(cp), float(rho), int(segments), int(backward), dptr(Wp), iptr(rng), None))
    del keep
    return Wp, rng, M, K


def host_factor_mfma(problem: Problem, rho: float, segments: int, mode: int):
    """Host-only: the MFMA fragment records exactly as admm_setup uploads them, as
    (N, bytes) uint8 arrays (forward, backward), plus whether the forward-elimination products are present."""
    lib = load_library()
    cp, keep = _abi.marshal_problem(problem)
    fb, bb, ok = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.admm_mfma_record_bytes(problem.n, problem.m, int(mode), C.byref(fb), C.byref(bb)))
    recMF = np.zeros((problem.N, fb.value), np.uint8)
    recMB = np.zeros((problem.N, bb.value), np.uint8)
    _check(lib, lib.admm_host_factor_mfma(C.byref(cp), float(rho), int(segments), int(mode),
                                          recMF.ctypes.data_as(C.c_void_p), recMB.ctypes.data_as(C.c_void_p), C.byref(ok)))
    del keep
    return recMF, recMB, bool(ok.value)
