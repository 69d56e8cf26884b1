"""The PCR_*_TIMES lines of the neighbourhood units (radius.hip, fpfh.hip, keypoints.hip, ransac.hip): which call leaves
which line on stderr, with which fields in which order.  tools/{radius,fpfh,iss,ransac}_time.py and docs/EXPERIMENTS.md read
these lines; nothing else pins their format.  The switches are read once per process, so the calls run in one fresh child."""
import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("pcr_tools_timing", os.path.join(REPO, "tools", "timing.py"))
timing = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(timing)

N, CHUNK = 2000, 4096

CHILD = r"""
import json, sys
import numpy as np
from point_cloud_registration_amd import _capi
from point_cloud_registration_amd.synthetic import street, street_normals

def mark(name):
    sys.stderr.flush()
    print("== " + name, file=sys.stderr, flush=True)

n, budget = %d, %d
mark("setup")
ctx = _capi.get_context(0)
pts = street(n, seed=0)
t = _capi.Target.points(ctx, pts, street_normals(pts))
lo, hi = 0.0, 5.0
for _ in range(30):                       # the radius with a mean count of about 15
    mid = 0.5 * (lo + hi)
    if t.radius_count(pts, mid).mean() < 15:
        lo = mid
    else:
        hi = mid
r = float(np.float32(hi))
mark("radius_count")
counts = t.radius_count(pts, r)
offsets = np.zeros(n + 1, np.int64)
np.cumsum(counts, out=offsets[1:])
chunks, a = [], 0                          # radius.hip: consecutive queries whose segments fit the budget, a larger one alone
while a < n:
    b = a + 1
    while b < n and offsets[b + 1] - offsets[a] <= budget:
        b += 1
    chunks.append([b - a, int(offsets[b] - offsets[a])])
    a = b
mark("radius_query")
t.radius_query(pts, r, offsets=offsets)
mark("fpfh")
F = t.fpfh(r)
mark("fpfh_rows")
t.fpfh(r, rows=np.arange(0, n, n // 50, dtype=np.int64)[:50])
rng = np.random.default_rng(5)
A, B = rng.uniform(0, 100, (300, 33)).astype(np.float32), rng.uniform(0, 100, (300, 33)).astype(np.float32)
mark("feature_match")
_capi.feature_match(ctx, A, B)
mark("iss_saliency")
t.iss_saliency(r)
mark("iss_keypoints")
t.iss_keypoints(r, float(np.float32(r * 2.0 / 3.0)))
src = rng.uniform(-5, 5, (64, 3)).astype(np.float32)
dst = (src + np.float32([0.5, -0.25, 0.125])).astype(np.float32)
poses = np.tile(np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, -0.25, 0.125]), (16, 1))
mark("pose_score")
_capi.pose_score(ctx, src, dst, poses, 0.1)
mark("ransac_poses")
_capi.ransac_poses(ctx, src, dst, 1024, 0, 0.1, 0.9, 0.0)
mark("end")
print(json.dumps({"mean_count": float(counts.mean()), "chunks": chunks}))
""" % (N, CHUNK)

MS = r"[0-9]+\.[0-9]{4}"


def _line(prefix, middle, phases):
    return re.compile("^" + prefix + " " + middle + "".join(f" {p} {MS}" for p in phases) + "$")


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, PCR_RADIUS_TIMES="1", PCR_FPFH_TIMES="1", PCR_ISS_TIMES="1", PCR_RANSAC_TIMES="1", PCR_RADIUS_CHUNK=str(CHUNK),
               PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
            sections[name] = []
        elif line.startswith("pcr_") and name is not None:
            sections[name].append(line)
    return sections, json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_stage_time_lines(child):
    sections, info = child
    assert 10 <= info["mean_count"] <= 20
    chunks = info["chunks"]
    assert len(chunks) > 1
    expected = {
        "radius_count": [_line("pcr_radius_times", f"pcr_radius_count queries {N}", ["count_ms"])],
        "radius_query": [_line("pcr_radius_times", f"pcr_radius_query queries {m} entries {e}", ["fill_ms", "sort_ms", "unpack_ms"])
                         for m, e in chunks],
        "fpfh": [_line("pcr_fpfh_times", f"points {N}", ["spfh_ms", "fpfh_ms"])],
        "fpfh_rows": [_line("pcr_fpfh_times", f"points {N} rows 50", ["spfh_ms", "fpfh_rows_ms"])],
        "feature_match": [_line("pcr_fpfh_times", "match na 300 nb 300 dim 33 splits [0-9]+", ["nn_ms", "merge_ms"])],
        "iss_saliency": [_line("pcr_iss_times", f"points {N}", ["saliency_ms"])],
        "iss_keypoints": [_line("pcr_iss_times", f"points {N}", ["saliency_ms", "nms_ms"])],
        "pose_score": [_line("pcr_ransac_times", "score m 64 b 16 splits [0-9]+", ["score_ms"])],
        "ransac_poses": [_line("pcr_ransac_times", "ransac m 64 n_hyp 1024 chunk 1024", ["fit_ms", "score_ms", "best_ms"])],
    }
    assert sections["end"] == []
    for call, patterns in expected.items():
        lines = sections[call]
        assert len(lines) == len(patterns), (call, lines)
        for line, pat in zip(lines, patterns):
            assert pat.match(line), (call, line, pat.pattern)
            assert line.split(" ", 1)[0] in timing.PREFIXES
            # what the tools read: the same names, in the line's order, through tools/timing.py's own regex
            got = timing.phase_ms(line)
            assert [name for name, _ in got] == re.findall(r"([a-z_]+_ms) ", pat.pattern), (call, line)
            assert all(math.isfinite(v) and v >= 0 for _, v in got), (call, line)
