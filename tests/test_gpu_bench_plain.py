"""The plain ``bench.py`` run (no ``--full``): the headline fields only, exactly ``--steps`` timed passes, and
``--dump-outputs`` writing what the LAST timed step computed -- checked against the same pass computed here, in
this process, at the pose of that step, and against a ``--full`` run of the same arguments."""

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

NAMES = ("H", "g", "e2", "correspondences")
CONFIG = "plane_b01_100k"


def _run(steps, extra, dump):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PCR_BENCH_SELF_LAUNCHED")}
    env["PCR_BENCH_NO_RCCL_PROBE"] = "1"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--config", CONFIG, "--steps", str(steps), "--warmup", "2",
           "--dump-outputs", str(dump)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(dump, f"{n}.npy")) for n in NAMES}


def _passes_along_the_trajectory():
    """The workload of bench.py's CONFIG built here, independently of the bench process: its Gauss-Newton trajectory
    and the sums of one pass at every pose of it (H, g, e2, count)."""
    from point_cloud_registration_amd import _capi
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    kind_name, n_target, n_scan, _, _ = bench.CONFIGS[CONFIG]
    assert kind_name == "plane"
    target = bench.make_cloud(n_target, seed=0, config=CONFIG)
    scan, _ = bench.make_scan(CONFIG, target, n_scan, seed=2)
    ctx = _capi.get_context(0)
    tgt = _capi.Target.points(ctx, target)
    tgt.estimate_normals(15, compat=True, want=False)
    sc = _capi.Scan(ctx, scan)
    try:
        _, iters, trace = _capi.align(tgt, sc, _capi.PLANE, np.eye(4), 30, 1e-3, 2.0, want_trace=True)
        traj = [trace[i, :16].reshape(4, 4).copy() for i in range(iters)]
        return [_capi.unpack29(_capi.linearize(tgt, sc, _capi.PLANE, T, 2.0)) for T in traj]
    finally:
        sc.close()
        tgt.close()


def _close(got, exp):
    H, g, e2, count = exp
    return (int(got["correspondences"]) == count and np.allclose(got["H"], H, rtol=1e-12, atol=0)
            and np.allclose(got["g"], g, rtol=1e-12, atol=1e-12 * float(np.max(np.abs(g))))
            and np.allclose(got["e2"], e2, rtol=1e-12, atol=0))


def test_plain_run_and_dumped_outputs(tmp_path):
    expected = _passes_along_the_trajectory()
    assert len(expected) >= 2, "the trajectory needs two poses to tell the last step from the first"
    steps = len(expected) + 2                         # the last step sits at pose 1 of the walk, the first at pose 0
    last = (steps - 1) % len(expected)

    line, got = _run(steps, [], tmp_path / "plain")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["unit"] == "Mcorr/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == steps and line["repeats"] == 1 and line["full"] is False and line["settle_passes"] > 0
    assert not {"roofline", "kernels", "cpu_baseline", "seam", "rccl_1rank"} & set(line)
    assert abs(line["value"] - 100_000 / (line["ms_per_step"] * 1e-3) / 1e6) < 0.02 * line["value"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["H"].shape == (6, 6) and got["g"].shape == (6,)
    assert int(got["correspondences"]) == line["config"]["correspondences_last_step"] > 0
    # the dump is the pass at the pose of the LAST timed step, and not the one at the first step's pose
    assert _close(got, expected[last]), "the dumped sums are not those of the last timed step"
    assert not _close(got, expected[0])

    full, ref = _run(steps, ["--full", "--no-pmc", "--no-cpu-baseline"], tmp_path / "full")
    assert full["full"] is True and "roofline" in full and full["repeats"] == 5 and full["settle_passes"] == 0
    assert _close(ref, expected[last])
