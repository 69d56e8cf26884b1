#!/usr/bin/env python3
"""Developer probe: what fast global registration costs (csrc/fgr.hip).

    python tools/fgr_time.py [out.json]
    PCR_LIB=point_cloud_registration_amd/libpcr_hip_dev.so python tools/fgr_time.py [out.json]      (+ the solo A/B)

Every figure is the median of five timed calls after two warm-ups, by HIP events around the call; loop_ms is the library's own
bracket around the kernels of the loop (PCR_FGR_TIMES=1, a line on stderr).

1. With a library that has k_fgr_solo (a developer build): pcr_fgr_pose, 64 iterations, as the loop of launches
   (PCR_FGR_SOLO=0) and as the single-block kernel (PCR_FGR_SOLO=1), three alternating runs, at 2 622 matches and at the
   largest list that fits (pcr_fgr_solo_max); the two forms must return the same bits.
2. The whole calls at 2 622, 5 000 and 50 000 matches: fgr_pose at its defaults (tuple test, loop, refinement), and
   ransac_pose at its defaults on the same matches beside it -- a figure to report, not a bar."""
import json
import os
import sys

import numpy as np

os.environ["PCR_FGR_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, timed  # noqa: E402
import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
MAX_DIST = 0.05
ctx = _capi.get_context(0)


def pairs(m, seed, inlier_share=0.3):
    """Uniform points in a 40 m box, a share of them a rigid copy with 0.01 m noise, the rest unrelated points."""
    from point_cloud_registration_amd.math_tools import expSO3
    rng = np.random.default_rng(seed)
    R, t = expSO3(np.array([0.9, -0.7, 1.1])), np.array([4.0, -7.0, 1.5])
    src = rng.uniform(-20, 20, (m, 3))
    dst = src @ R.T + t + rng.normal(0, 0.01, (m, 3))
    out = rng.random(m) >= inlier_share
    dst[out] = rng.uniform(-20, 20, (int(out.sum()), 3)) + t
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)


def mu0_of(src, dst):
    D = max(float(np.linalg.norm(a.max(axis=0).astype(np.float64) - a.min(axis=0).astype(np.float64))) for a in (src, dst))
    return D * D


res = {"warmups": WARM, "timed_calls": REPS, "solo_max": _capi.fgr_solo_max(ctx), "ab": [], "calls": []}
if res["solo_max"]:
    for m in (2622, res["solo_max"]):
        if m > res["solo_max"]:
            print(f"m {m} does not fit (solo_max {res['solo_max']})", flush=True)
            continue
        src, dst = pairs(m, seed=m)
        mu0 = mu0_of(src, dst)
        row = {"m": m, "loop_call_ms": [], "solo_call_ms": [], "loop_kernels_ms": [], "solo_kernels_ms": []}
        box = {}
        for run in range(3):
            for form, flag in (("loop", "0"), ("solo", "1")):
                os.environ["PCR_FGR_SOLO"] = flag
                t, line = timed(lambda: box.__setitem__(form, _capi.fgr_pose(ctx, src, dst, np.eye(4), mu0, MAX_DIST ** 2, 1.4, 4, 64)), ("loop_ms",),
                                report=True)
                assert ("form solo" in line) == (form == "solo"), line
                row[form + "_call_ms"].append(t["call_ms"])
                row[form + "_kernels_ms"].append(t["loop_ms"])
        os.environ.pop("PCR_FGR_SOLO")
        row["same_bits"] = bool(np.array_equal(box["loop"]["T"].view(np.uint64), box["solo"]["T"].view(np.uint64)) and
                                np.array_equal(box["loop"]["weights"].view(np.uint64), box["solo"]["weights"].view(np.uint64)))
        row["solo_below_loop_in_every_run"] = bool(all(s < l for s, l in zip(row["solo_call_ms"], row["loop_call_ms"])))
        res["ab"].append(row)
        print(row, flush=True)

for m in (2622, 5_000, 50_000):
    src, dst = pairs(m, seed=m)
    rows = np.arange(m)
    box = {}
    tf, line = timed(lambda: box.__setitem__("fgr", pcr.fgr_pose(src, dst, rows, rows, MAX_DIST, return_info=True)), ("loop_ms",), report=True)
    tl = timed(lambda: _capi.fgr_pose(ctx, src, dst, np.eye(4), mu0_of(src, dst), MAX_DIST ** 2, 1.4, 4, 64), ("loop_ms",))
    tr = timed(lambda: box.__setitem__("ransac", pcr.ransac_pose(src, dst, rows, rows, MAX_DIST, return_info=True)))
    Tf, Tr = box["fgr"][0], box["ransac"][0]
    row = {"m": m, "fgr_pose_call_ms": tf["call_ms"], "fgr_pose_loop_kernels_ms": tf["loop_ms"], "pcr_fgr_pose_call_ms": tl["call_ms"],
           "pcr_fgr_pose_loop_kernels_ms": tl["loop_ms"], "ransac_pose_call_ms": tr["call_ms"], "fgr_count": box["fgr"][1]["count"],
           "ransac_count": box["ransac"][1]["count"], "fgr_n_valid": box["fgr"][1]["n_valid"],
           "max_abs_T_difference": float(np.abs(Tf - Tr).max()), "report": line}
    res["calls"].append(row)
    print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
