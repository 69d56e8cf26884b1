#!/usr/bin/env python3
"""Developer probe: what the FPFH descriptors and the feature matching cost (csrc/fpfh.hip), kernel by kernel.

    python tools/fpfh_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points) with its analytic normals.  Two radii, found by bisection on the counts of a
20 k-point sample (tools/radius_time.py's): a mean count of about 15 and about 60.  With PCR_FPFH_TIMES=1 the library
brackets k_spfh and k_fpfh of a pcr_target_fpfh call, and k_feature_nn and its merge of a pcr_feature_match call, with HIP
events on the context's stream and reports their milliseconds on stderr; this tool collects those lines (stderr goes through
a temporary file) and prints the median of the timed calls after the warm-ups, beside the time of the whole call by events
around it -- upload, kernels and copy-back, what a caller of the C ABI pays.

Matching: 33-column rows, 20 k x 20 k and 100 k x 100 k (descriptors of the cloud where it has that many, random rows
otherwise).  Its arithmetic is 3 D lane-operations per pair (subtract, multiply, add; no fma by contract); the share printed
is that count over the kernel time, against one unpacked float32 VALU operation per lane and cycle on every CU:
256 CUs x 64 lanes x 2.4 GHz = 39.3 T lane-operations/s."""
import json
import os
import sys

import numpy as np

os.environ["PCR_FPFH_TIMES"] = "1"                # (read once, by the first call)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, quiet, radius_for, timed  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import street, street_normals  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
VALU_LANE_OPS = 256 * 64 * 2.4e9

ctx = _capi.get_context(0)
pts = street(n, seed=0)
t = _capi.Target.points(ctx, pts, street_normals(pts))
sample = pts[np.random.default_rng(3).choice(n, min(n, 20_000), replace=False)]

res = {"n": n, "warmups": WARM, "timed_calls": REPS, "rows": []}
F = None
for want in (15, 60):
    r = radius_for(t, sample, want)
    F, k = quiet(lambda: t.fpfh(r, want_k=True))
    m = timed(lambda: t.fpfh(r), ("spfh_ms", "fpfh_ms"))
    row = {"what": f"fpfh, mean neighbours {k.mean():.1f}", "r": r, "pairs": int(k.sum()), "most_neighbours": int(k.max()),
           "spfh_kernel_ms": m["spfh_ms"], "fpfh_kernel_ms": m["fpfh_ms"], "call_ms": m["call_ms"]}
    res["rows"].append(row)
    print(row, flush=True)
rng = np.random.default_rng(4)
for rows in (20_000, 100_000):
    if 2 * rows <= n:
        A, B, src = F[:rows], F[rows:2 * rows], "descriptors of the cloud"
    else:
        A, B, src = rng.uniform(0, 100, (rows, 33)).astype(np.float32), rng.uniform(0, 100, (rows, 33)).astype(np.float32), "random rows"
    m = timed(lambda: _capi.feature_match(ctx, A, B), ("nn_ms", "merge_ms"))
    ops = 3.0 * 33 * rows * rows
    row = {"what": f"match {rows} x {rows} x 33 ({src})", "nn_kernel_ms": m["nn_ms"], "merge_kernel_ms": m["merge_ms"], "call_ms": m["call_ms"],
           "lane_ops": ops, "valu_share": ops / (m["nn_ms"] * 1e-3) / VALU_LANE_OPS if m["nn_ms"] > 0 else None}
    res["rows"].append(row)
    print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
