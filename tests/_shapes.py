"""The (n, m) pairs the build compiles, read from the X-macro lists of the instantiation units (their release branch: the
ADMM_DEV_DIMS lists of development builds are skipped).  One source of truth for the shape sweeps of the suite:

  SHARED        batch-shared dynamics, ADMM_GROUP_DIMS of csrc/admm_dims_g*.hip (what admm_setup accepts)
  PER_INSTANCE  per-instance dynamics, ADMM_PINST_DIMS_G0 / _G1 / _G2 of csrc/admm_pinst*.hip
  WIDE          the per-instance pairs that run rows-over-lanes only (ADMM_PINST_DIMS_G2, admm_pinst_wide.hpp)
  MFMA          the MFMA family, ADMM_MFMA_DIMS of csrc/admm_mfma.hip"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "admm-library_amd", "csrc")


def x_macro(fname: str, macro: str):
    """The X(n, m) pairs of `#define macro(X) ...` in csrc/fname, outside `#ifdef ADMM_DEV_DIMS` ... `#else`."""
    pairs, dev = [], False
    for line in open(os.path.join(CSRC, fname)):
        s = line.strip()
        if s.startswith("#ifdef ADMM_DEV_DIMS"):
            dev = True
        elif s.startswith("#else") or s.startswith("#endif"):
            dev = False
        elif not dev and re.match(r"#define\s+" + re.escape(macro) + r"\(X\)", s):
            pairs += [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", s.split("(X)", 1)[1])]
    if not pairs:
        raise RuntimeError(f"no {macro} list in {fname}")
    return pairs


SHARED = sorted(p for g in range(4) for p in x_macro(f"admm_dims_g{g}.hip", "ADMM_GROUP_DIMS"))
WIDE = sorted(x_macro("admm_pinst_g2.hip", "ADMM_PINST_DIMS_G2"))
PER_INSTANCE = sorted(x_macro("admm_pinst.hip", "ADMM_PINST_DIMS_G0") + x_macro("admm_pinst_g1.hip", "ADMM_PINST_DIMS_G1") + WIDE)
MFMA = sorted(x_macro("admm_mfma.hip", "ADMM_MFMA_DIMS"))


def sid(shape) -> str:
    return f"n{shape[0]}m{shape[1]}"


# The shared-dynamics sweep's problem per pair (tests/test_gpu_shapes.py): pkg.random_ltv(N=SWEEP_N, n, m, batch, seed) at rho, with
# SWEEP_SEGMENTS segments.  Each passes the forward-elimination form's host probe (admm_factor.cpp, alt_check <= 5e-12), so the
# library's default path -- the alternating-direction kernels -- runs; tests/test_shapes.py checks that on the CPU.  The probe
# depends on the dynamics, weights, rho and segments only: not on q, the bounds, the thrust bound or the batch.
SWEEP_N, SWEEP_SEGMENTS = 20, 4
ALT_TABLE = {      # (n, m): (seed, rho)
    (1, 1): (1017, 0.3), (2, 1): (1033, 0.3), (2, 2): (1034, 0.3), (3, 1): (1049, 0.3), (3, 2): (1050, 0.3), (3, 3): (1051, 0.3),
    (4, 1): (1065, 0.3), (4, 2): (1066, 0.3), (4, 3): (1067, 0.3), (4, 4): (1068, 0.3), (5, 1): (1081, 0.3), (5, 2): (1082, 0.3),
    (5, 3): (1083, 0.3), (6, 1): (1097, 0.3), (6, 2): (1098, 0.3), (6, 3): (1099, 0.3), (6, 4): (1100, 0.3), (6, 6): (1102, 0.3),
    (7, 2): (1114, 0.3), (7, 3): (1115, 0.3), (8, 2): (1130, 0.3), (8, 3): (1131, 0.3), (8, 4): (1132, 0.3), (9, 3): (1147, 0.3),
    (10, 2): (1163, 0.3),          # (seed 1162, the rule 1000 + 16 n + m, fails the probe: 1163 is the next one that passes)
    (10, 4): (1164, 0.3), (12, 3): (1195, 0.3), (12, 4): (1196, 0.3), (12, 6): (1198, 0.3),
}
# pairs without a reasonable problem that passes the probe: they run the plain kernels, and the sweep asserts the warning
PLAIN_ONLY = {}
