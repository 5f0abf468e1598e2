"""What the oracle sweeps of the GPU suite share (tests/test_gpu_shapes.py, tests/test_gpu_scan_geometry.py): the call schedule
every case runs and the project's comparison, 1e-10 relative to max(1, |reference|_inf) per array."""
import numpy as np

TOL = 1e-10
SCHEDULE_ITERATIONS = 39


def close(got, ref, tol=TOL):
    return all(np.abs(a - ref[k]).max() <= tol * max(1.0, np.abs(ref[k]).max()) for a, k in zip(got, ("w", "z", "y")))


def schedule(s, z0, y0, first_residuals):
    """39 iterations: the (z, y)-form first sweep from a caller's state, residual / non-residual kernels, calls of both
    parities (a forward or a backward kernel before a residual one) -- RESID 0 / 1 and XFREE 0 / 1 / 2 on one handle."""
    s.set_state(z=z0, y=y0)
    s.run(1, residual_every=1 if first_residuals else 0)
    s.run(8, residual_every=4)
    s.iterate(5)
    s.iterate(2)
    s.run(6, residual_every=1)
    s.run(10, residual_every=3)
    s.run(7, residual_every=2)
    return s.get()
