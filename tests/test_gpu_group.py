"""Single-process multi-device (``devices=[...]`` -> pcr_group_*, csrc/group.hip) on the one GPU of the test box: N contexts of
device 0 (the C ABI lets a device id repeat for exactly this).  The checks live in tests/group_check.py and run in a fresh
process per N, because N streams that wait for each other inside kernels need N hardware queues (GPU_MAX_HW_QUEUES, read when
the HIP runtime starts).  Reference seam: the single-process call order of registration.py:28,71 / demo_matching.py:147-152."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_group_n_contexts_one_gpu(n):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(4 if n <= 2 else 4 * n), PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "group_check.py"), str(n)], env=env, capture_output=True,
                       text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "GROUP_CHECK_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- at scale: the pipelines large shards run (tests/group_scale_check.py) ------------------------------------------------
SCALE_CASES = [("b01", 2, {}), ("b01", 3, {}), ("b01", 8, {}),
               ("b01", 3, {"PCR_VARIANT": "1"}), ("b01", 8, {"PCR_VARIANT": "1"}),
               ("b01", 3, {"PCR_VARIANT": "1", "PCR_REUSE": "2"}), ("b01", 3, {"PCR_VARIANT": "1", "PCR_TILE_LOCAL": "0"}),
               ("straddle", 2, {}), ("tiny", 8, {}), ("lidar", 2, {"PCR_VARIANT": "1"}), ("lidar", 3, {"PCR_VARIANT": "1"})]


def _case_id(case):
    scenario, n, env = case
    return f"{scenario}-{n}" + "".join(f"-{k[4:].lower()}{v}" for k, v in env.items())


@pytest.fixture(scope="module")
def scale_runs(tmp_path_factory):
    """The saved sums / poses / traces of every case that ran, for the comparisons across runs."""
    return {"dir": tmp_path_factory.mktemp("group_scale"), "done": {}}


@pytest.mark.parametrize("case", SCALE_CASES, ids=[_case_id(c) for c in SCALE_CASES])
def test_group_at_scale(case, scale_runs):
    """N contexts of GPU 0 at B-01 size, on the straddling crossover, with empty shards and on the heavy LiDAR index: the group's
    sums against the SPMD sums bit for bit, the oracle and the reference; which pipeline every member ran; device loop against
    host loop; the exchange after wrapped slots and a singular align.  Then, across runs: the three N = 3 PCR_VARIANT=1 runs
    (which differ only in which exact search finds the same matches) are bit-identical, and at N = 8 the fused members'
    sums agree with the split members' to the bar of test_tile_handout_covers_every_point_once."""
    import numpy as np
    scenario, n, extra = case
    out = os.path.join(str(scale_runs["dir"]), _case_id(case) + ".npz")
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(4 if n <= 2 else min(4 * n, 32)), PYTHONPATH=REPO)
    for k in ("PCR_VARIANT", "PCR_REUSE", "PCR_TILE_LOCAL"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "group_scale_check.py"), scenario, str(n), out], env=env,
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "GROUP_SCALE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    res = dict(np.load(out))
    runs = scale_runs["done"]
    runs[_case_id(case)] = res
    if scenario == "b01" and (n == 2 or extra):
        # the pipeline proof: every member ran search + reduce on the full scan (not a vacuous pass through the fused kernel)
        assert all(res["pertfull_icp_split"]) and all(res["pertfull_ndt_split"]), {k: v for k, v in res.items() if k.endswith("_split")}
    if scenario == "b01" and n == 3 and extra:
        v1 = [runs.get(_case_id(c)) for c in SCALE_CASES if c[0] == "b01" and c[1] == 3 and c[2]]
        if all(x is not None for x in v1):
            a = v1[0]
            for b in v1[1:]:
                assert sorted(a) == sorted(b)
                for k in a:
                    assert a[k].tobytes() == b[k].tobytes(), (k, "N = 3 PCR_VARIANT=1 runs differ")
    if scenario == "b01" and n == 8:
        both = [runs.get(_case_id(c)) for c in SCALE_CASES if c[0] == "b01" and c[1] == 8]
        if all(x is not None for x in both):
            fused, split = both
            assert not any(fused["pertfull_icp_split"]) and all(split["pertfull_icp_split"])
            for k in fused:
                if k.endswith("_lin") or k.endswith("_xchg"):
                    f, s = fused[k], split[k]
                    assert np.array_equal(f[..., 28], s[..., 28]), (k, "correspondence counts")
                    assert np.allclose(f, s, rtol=1e-11, atol=1e-9 * np.max(np.abs(s))), (k, "fused and split members disagree")
