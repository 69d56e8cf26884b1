#!/usr/bin/env python3
"""Developer probe: what the ISS keypoints and the FPFH descriptors at chosen rows cost (csrc/keypoints.hip, k_fpfh_rows of
csrc/fpfh.hip), kernel by kernel.

    python tools/iss_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points) with its analytic normals.  The two radii of tools/fpfh_time.py, found by bisection
on the counts of a 20 k-point sample: a mean count of about 15 and about 60; the non-maximum radius is 2/3 of the salient one
(the 4 : 6 of the defaults).  With PCR_ISS_TIMES=1 the library brackets k_iss_saliency and k_iss_nms of a
pcr_target_iss_keypoints call, with PCR_FPFH_TIMES=1 k_spfh and (k_fpfh_row_index +) k_fpfh_rows of a pcr_target_fpfh_rows
call, with HIP events on the context's stream and reports their milliseconds on stderr; this tool collects those lines and
prints the median of the timed calls after the warm-ups, beside the time of the whole call by events around it.  The full
pcr_target_fpfh call is timed beside the rows call, and register_global on a pair of clouds of at most 100 k points with and
without keypoints="iss" by the wall clock."""
import json
import os
import sys
import time

import numpy as np

os.environ["PCR_ISS_TIMES"] = "1"                 # (both read once, by the first call)
os.environ["PCR_FPFH_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, quiet, radius_for, timed  # noqa: E402
import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import street, street_normals  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None

ctx = _capi.get_context(0)
pts = street(n, seed=0)
nrm = street_normals(pts)
t = _capi.Target.points(ctx, pts, nrm)
sample = pts[np.random.default_rng(3).choice(n, min(n, 20_000), replace=False)]

res = {"n": n, "warmups": WARM, "timed_calls": REPS, "rows": []}
for want in (15, 60):
    rs = radius_for(t, sample, want)
    rn = float(np.float32(rs * 2.0 / 3.0))
    mask = quiet(lambda: t.iss_keypoints(rs, rn))
    keys = np.flatnonzero(mask).astype(np.int64)
    m = timed(lambda: t.iss_keypoints(rs, rn), ("saliency_ms", "nms_ms"))
    row = {"what": f"iss, salient radius for a mean count of {want}", "r_salient": rs, "r_nonmax": rn, "keypoints": int(len(keys)),
           "saliency_kernel_ms": m["saliency_ms"], "nms_kernel_ms": m["nms_ms"], "call_ms": m["call_ms"]}
    res["rows"].append(row)
    print(row, flush=True)
    full = timed(lambda: t.fpfh(rs), ("spfh_ms", "fpfh_ms"))
    part = timed(lambda: t.fpfh(rs, rows=keys), ("spfh_ms", "fpfh_rows_ms"))
    row = {"what": f"fpfh at the {len(keys)} keypoints against all {n} rows", "r": rs, "spfh_kernel_ms": part["spfh_ms"],
           "fpfh_rows_kernel_ms": part["fpfh_rows_ms"], "rows_call_ms": part["call_ms"], "full_spfh_kernel_ms": full["spfh_ms"],
           "full_fpfh_kernel_ms": full["fpfh_ms"], "full_call_ms": full["call_ms"]}
    res["rows"].append(row)
    print(row, flush=True)

# register_global with and without keypoints on a pair of clouds of at most 100 k points, by the wall clock
m = min(n, 100_000)
a = street(m, seed=0)
na = street_normals(a)
yaw = 0.3
R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
b = (a.astype(np.float64) @ R.T + np.array([2.0, -1.0, 0.3])).astype(np.float32)
nb = (na.astype(np.float64) @ R.T).astype(np.float32)
ta = _capi.Target.points(ctx, a)
probe = a[np.random.default_rng(3).choice(m, min(m, 20_000), replace=False)]
r60 = radius_for(ta, probe, 60)
for kp in (None, "iss"):
    walls = []
    for _ in range(1 + 3):
        t0 = time.perf_counter()
        T, info = quiet(lambda: pcr.register_global(a, b, r60, 0.5 * r60, normals=(na, nb), keypoints=kp, n_hypotheses=20_000, return_info=True))
        walls.append(time.perf_counter() - t0)
    moved = np.linalg.norm(a.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - b, axis=1)
    row = {"what": f"register_global, {m} points, keypoints={kp!r}", "feature_radius": r60, "wall_s": float(np.median(walls[1:])),
           "matches": int(len(info["inliers"])), "inliers": int(info["count"]), "within_max_dist": float(np.mean(moved <= 0.5 * r60))}
    res["rows"].append(row)
    print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
