#!/usr/bin/env python3
"""Developer probe: what the normals from a ball cost (k_ball_moments of csrc/ball_moments.hip), beside k_iss_saliency
(csrc/keypoints.hip), which does the same walk and the same sums.

    python tools/ball_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points).  Radii: the 0.266 m and 0.540 m every neighbouring unit is quoted at (a mean count of
about 15 and about 60 on that cloud).  With PCR_BALL_TIMES=1 the library brackets k_ball_moments of a
pcr_target_estimate_normals_radius call, with PCR_ISS_TIMES=1 k_iss_saliency of a pcr_target_iss_saliency call, with HIP
events on the context's stream and reports their milliseconds on stderr; this tool collects those lines and prints the median
of the timed calls after the warm-ups, beside the time of the whole call by events around it.  Forms: the radius set
(max_nn = 0), the register list (max_nn = 16) and the LDS list (max_nn = 30)."""
import json
import os
import sys

import numpy as np

os.environ["PCR_BALL_TIMES"] = "1"                # (both read once, by the first call)
os.environ["PCR_ISS_TIMES"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, quiet, timed  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import street  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None

ctx = _capi.get_context(0)
pts = street(n, seed=0)
t = _capi.Target.points(ctx, pts)

res = {"n": n, "warmups": WARM, "timed_calls": REPS, "rows": []}
for r in (0.266, 0.540):
    cnt = quiet(lambda: t.estimate_normals_radius(r, want=False, want_counts=True))[1]
    iss = timed(lambda: t.iss_saliency(r), ("saliency_ms",))
    row = {"what": "k_iss_saliency", "r": r, "mean_count": float(cnt.mean()), "max_count": int(cnt.max()), "kernel_ms": iss["saliency_ms"],
           "call_ms": iss["call_ms"]}
    res["rows"].append(row)
    print(row, flush=True)
    for max_nn in (0, 16, 30):
        m = timed(lambda: t.estimate_normals_radius(r, max_nn, want=False), ("moments_ms",))
        row = {"what": f"k_ball_moments, max_nn = {max_nn}", "r": r, "kernel_ms": m["moments_ms"], "call_ms": m["call_ms"],
               "ratio_to_iss": m["moments_ms"] / iss["saliency_ms"]}
        res["rows"].append(row)
        print(row, flush=True)
knn = timed(lambda: t.estimate_normals(15, compat=False, want=False))
row = {"what": "pcr_target_estimate_normals, k = 15 (the whole call)", "call_ms": knn["call_ms"]}
res["rows"].append(row)
print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
