"""bench.py's launcher contract (ADVICE r01 / VERDICT r01 next #6): `--gpus N` must never silently time
fewer than N GPUs.  CPU-only checks: no GPU exists here, so both forms must exit non-zero with a message
that says why, before anything touches a device.  Then the plain run's contract: exactly --steps timed steps, and
--dump-outputs writes what they computed (on the GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, drop=()):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_gpus_without_launcher_refuses_when_devices_are_missing():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this check is for machines with fewer than 2 GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], drop=("WORLD_SIZE", "RANK", "LOCAL_RANK"))
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and "visible" in r.stderr
    assert '"n_gpus"' not in r.stdout            # no figure was reported


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4", "--steps", "1", "--warmup", "0"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_plain_run_options_are_offered():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_dump_outputs_are_exactly_warmup_plus_steps_iterations(gpu, tmp_path):
    """A plain run times exactly --steps steps after --warmup ones on a freshly set-up handle, and --dump-outputs writes what
    the last of them computed: the w, z, y and residual norms of W + K iterations of a handle of the same seeded problem."""
    import numpy as np
    import admm_library_amd as pkg
    W, K = 2, 3
    r = _run(["--gpus", "1", "--steps", str(K), "--warmup", str(W), "--batch", "64", "--horizon", "50", "--warm-seconds", "0",
              "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["ms_per_step"] > 0
    assert "roofline" not in line and "cpu_baseline" not in line           # side measurements are --full only
    with pkg.Solver(pkg.cw_rendezvous(N=50, batch=64), pkg.Options(rho=0.05, check_interval=1, device=0)) as s:
        s.run(W, residual_every=1)
        s.run(K, residual_every=1, sync=True)
        want = s.get() + s.residuals()
    for name, v in zip(("w", "z", "y", "r", "s", "norm_w", "norm_z", "norm_y"), want):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == v.shape, name
        np.testing.assert_allclose(got, v, rtol=1e-12, atol=1e-12, err_msg=name)
