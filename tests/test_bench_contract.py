"""bench.py pieces that do not need a GPU: configuration table, argument defaults, and the
cpu_baseline leg (the oracle timed on a bounded sample)."""

import importlib.util
import json
import os
import sys

import numpy as np

from conftest import REPO


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_configs_match_baseline_json():
    bench = _load_bench()
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert "correspondences/sec" in base["metric"]
    # one bench config per BASELINE.json config line
    assert {"icp_b01_harness", "plane_b01", "vplane_10m", "ndt_10m", "plane_100m"} <= set(bench.CONFIGS)
    assert bench.CONFIGS["icp_b01_harness"][0] == "icp" and bench.CONFIGS["icp_b01_harness"][2] == 100_000
    assert bench.CONFIGS["plane_b01"][0] == "plane" and bench.CONFIGS["plane_b01"][1] == 1_060_000
    assert bench.CONFIGS["vplane_10m"][3] == 0.5 and bench.CONFIGS["ndt_10m"][3] == 1.0
    assert bench.B_ALG == {"icp": 24, "plane": 36, "vplane": 36, "ndt": 48}
    assert bench.HBM_PEAK_GBS == 8000.0
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse()
    finally:
        sys.argv = old
    assert a.gpus == 1 and a.config == "plane_b01" and a.steps > 0 and a.warmup >= 0


def test_plain_run_is_lean_and_full_is_opt_in():
    """A plain run times ONE block of exactly --steps passes; --full brings back the repeated blocks (and everything
    else that is not the headline); --repeats still wins when given."""
    bench = _load_bench()
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--steps", "17"]
        a = bench.parse()
        assert a.full is False and a.dump_outputs is None and a.repeats == 1 and a.steps == 17
        sys.argv = ["bench.py", "--full"]
        a = bench.parse()
        assert a.full is True and a.repeats == 5
        sys.argv = ["bench.py", "--full", "--repeats", "3", "--dump-outputs", "out"]
        a = bench.parse()
        assert a.repeats == 3 and a.dump_outputs == "out"
    finally:
        sys.argv = old


def test_dump_outputs_writes_what_a_caller_receives(tmp_path):
    """--dump-outputs: the 29 sums of the last step as H (6x6, symmetric), g (6), e2 and the correspondence count,
    float64 .npy files."""
    bench = _load_bench()
    out = np.arange(29, dtype=np.float64)
    out[28] = 1234.0
    bench.dump_outputs(str(tmp_path / "d"), out)
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("H", "g", "e2", "correspondences")}
    assert all(v.dtype == np.float64 for v in got.values())
    H = got["H"]
    assert H.shape == (6, 6) and np.array_equal(H, H.T) and H[0, 0] == 0 and H[0, 5] == 5 and H[5, 5] == 20
    assert np.array_equal(got["g"], np.arange(21, 27)) and got["e2"] == 27 and got["correspondences"] == 1234


def test_cpu_baseline_leg_runs_on_the_oracle():
    bench = _load_bench()
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(20000, seed=1)
    scan, _ = perturbed_scan(target, 5000, seed=2)
    out = bench.cpu_baseline("icp", target, scan, None, [np.eye(4)], 2.0, None, 1)
    assert out["kind"] == "port" and out["unit"] == "Mcorr/s" and out["value"] > 0 and out["cores"] >= 1
    assert out["cores"] == out["effective_cpus"] == bench.effective_cpus()      # the OpenMP team = the CPU quota
    out = bench.cpu_baseline("ndt", target, scan, None, [np.eye(4)], 2.0, 1.0, 1)
    assert out["value"] > 0 and "sample" in out


def test_self_launch_builds_the_torchrun_command(monkeypatch):
    """`python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run on 127.0.0.1."""
    bench = _load_bench()
    seen = {}

    def fake_exec(file, argv, env):
        seen.update(file=file, argv=list(argv), env=dict(env))
        raise SystemExit(0)

    monkeypatch.setattr(os, "execvpe", fake_exec)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5"])
    for k in ("WORLD_SIZE", "RANK"):
        monkeypatch.delenv(k, raising=False)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    a = seen["argv"]
    assert a[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in a and "--nnodes=1" in a
    assert a[a.index("--master-addr") + 1] == "127.0.0.1" and int(a[a.index("--master-port") + 1]) > 0
    i = a.index(os.path.join(REPO, "bench.py"))
    assert a[i + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_rank_environment_is_not_relaunched(monkeypatch):
    """Under a launcher (RANK / WORLD_SIZE set) bench.py must NOT exec again; a world-size mismatch is an error."""
    bench = _load_bench()
    monkeypatch.setattr(os, "execvpe", lambda *a: (_ for _ in ()).throw(AssertionError("relaunched")))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setenv("WORLD_SIZE", "4"); monkeypatch.setenv("RANK", "0")
    fd1 = os.dup(1)
    try:
        try:
            bench.main()
        except SystemExit as e:
            assert "WORLD_SIZE=4" in str(e.code)
        else:
            raise AssertionError("expected SystemExit")
    finally:
        os.dup2(fd1, 1); os.close(fd1)


def test_effective_cpus_respects_the_quota():
    bench = _load_bench()
    n = bench.effective_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            assert n <= max(int(float(q) / float(per)), 1)
    except OSError:
        pass
