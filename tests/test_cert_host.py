"""On-device certificate, the part that needs no GPU: the ABI surface (header, exported symbols, NULL handle)
and the reference the GPU tests compare against (tests/_cert_ref.py), checked against the independent routines of
tests/_indep.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import admm_library_amd as pkg
import oracle_c
import _cert_ref as cr
import _indep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def test_header_announces_the_certificate_and_keeps_abi_9(built):
    h = open(os.path.join(ROOT, "include", "admm_hip.h")).read()
    assert re.search(r"^#define ADMM_HIP_HAS_CERTIFICATE 1\s*$", h, re.M)
    assert re.search(r"^#define ADMM_HIP_ABI_VERSION 9\s*$", h, re.M)
    assert re.search(r"int admm_get_certificate\(admm_handle\* h, double\* obj, double\* feas_dyn, double\* stat, double\* nu\);", h)
    assert re.search(r"int admm_get_certificate_device\(admm_handle\* h, double\* obj, double\* feas_dyn, double\* stat, double\* nu, "
                     r"void\* hip_stream\);", h)
    assert pkg.load_library().admm_abi_version() == 9


def test_library_exports_both_symbols(built):
    out = subprocess.run(["nm", "-D", pkg.library_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"admm_get_certificate", "admm_get_certificate_device"} <= names


def test_null_handle_is_invalid(built):
    lib = pkg.load_library()
    out = np.zeros(4)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.admm_get_certificate(None, ptr, None, None, None) == INVALID
    assert "NULL handle" in lib.admm_last_error().decode()
    assert lib.admm_get_certificate_device(None, ptr, None, None, None, None) == INVALID
    assert "NULL handle" in lib.admm_last_error().decode()


def _solution():
    p = pkg.cw_rendezvous(N=40, batch=3)
    rho = 0.05
    ref = oracle_c.solve(p, rho=rho, max_iter=4000, check_interval=10, eps_abs=1e-9, eps_rel=1e-9)
    return p, rho, ref["z"], ref["y"]


def test_reference_costates_cancel_the_state_rows():
    """g + G'nu_ref, with G from _indep.dynamics_matrix: its state rows vanish to rounding (the recursion is their solution) and
    its largest entry is stat_ref."""
    p, rho, z, y = _solution()
    c = cr.certificate(p, z, y, rho)
    g = cr.gradient(p, z, y, rho).reshape(p.batch, p.L)
    G = _indep.dynamics_matrix(p)
    res = (g + (G.T @ c["nu"].reshape(p.batch, -1).T).T).reshape(p.batch, p.N, p.nb)
    scale = np.maximum(1.0, np.abs(c["nu"]).reshape(p.batch, -1).max(axis=1))
    assert np.all(np.abs(res[:, :, p.m:]).reshape(p.batch, -1).max(axis=1) <= 1e-13 * scale)
    assert np.allclose(np.abs(res).reshape(p.batch, -1).max(axis=1), c["stat"], rtol=0, atol=1e-13 * scale.max())
    fd = _indep.kkt_certificate_batch(p, z, y, rho)[0]
    assert np.allclose(c["feas_dyn"], fd, rtol=0, atol=1e-14)


def test_reference_stat_bounds_the_least_squares_stat():
    """kkt_certificate_batch takes the multiplier that minimises the 2-norm of r = g + G'nu.  So
    |r_ls|_inf <= |r_ls|_2 <= |r_ref|_2 <= sqrt(L) |r_ref|_inf, i.e. stat_ref >= stat_ls / sqrt(L)."""
    p, rho, z, y = _solution()
    c = cr.certificate(p, z, y, rho)
    stat_ls = _indep.kkt_certificate_batch(p, z, y, rho)[2]
    assert np.all(c["stat"] >= stat_ls / np.sqrt(p.L))
    # not converged: the same bound
    rng = np.random.default_rng(5)
    z2, y2 = z + 0.1 * rng.standard_normal(z.shape), y + 0.1 * rng.standard_normal(y.shape)
    c2 = cr.certificate(p, z2, y2, rho)
    assert np.all(c2["stat"] >= _indep.kkt_certificate_batch(p, z2, y2, rho)[2] / np.sqrt(p.L))


def test_reference_objective_is_the_quadratic_form():
    p = pkg.random_ltv(N=7, n=4, m=2, batch=2, seed=11)
    rng = np.random.default_rng(2)
    z, y = rng.standard_normal((2, p.L)), rng.standard_normal((2, p.L))
    fuel = rng.uniform(0.0, 1.0, p.N)
    c = cr.certificate(p, z, y, 0.3, fuel=fuel)
    Pd = _indep.hessian_diag_blocks(p)
    for b in range(2):
        Z = z[b].reshape(p.N, p.nb)
        want = sum(0.5 * Z[k] @ Pd[k] @ Z[k] + fuel[k] * np.linalg.norm(Z[k, :p.m]) for k in range(p.N)) + p.q[b] @ z[b]
        assert abs(c["obj"][b] - want) <= 1e-12 * c["obj_abs"][b]
