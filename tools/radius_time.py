#!/usr/bin/env python3
"""Developer probe: what the radius search costs (csrc/radius.hip), phase by phase, next to the k-NN it stands beside.

    python tools/radius_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points), queried with its own points.  Two radii, found by bisection on the counts of a
20 k-point sample: a mean count of about 15 and about 60.  With PCR_RADIUS_TIMES=1 the library brackets the count kernel and,
in a query call, fill / sort / unpack with HIP events on the context's stream and reports their milliseconds on stderr; this
tool collects those lines (stderr goes through a temporary file) and prints the median of the timed calls after the warm-ups.
A call's phases are summed over its chunks (PCR_RADIUS_CHUNK).  Beside them, by events around the whole call -- upload,
kernels and copy-back, what a caller of the C ABI pays: the count and the query call, pcr_knn_query at k = 16 and 64 on the
same queries, and (tools/knn_time.py's figure) estimate_normals at those k, whose kernel is the k-NN search plus a 3x3
eigen-solve and which copies nothing back."""
import json
import os
import sys

import numpy as np

os.environ["PCR_RADIUS_TIMES"] = "1"              # (read once, by the first radius call)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, quiet, radius_for, timed  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import street  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None

ctx = _capi.get_context(0)
pts = street(n, seed=0)
t = _capi.Target.points(ctx, pts)
sample = pts[np.random.default_rng(3).choice(n, min(n, 20_000), replace=False)]

res = {"n": n, "queries": n, "warmups": WARM, "timed_calls": REPS, "rows": []}
for want in (15, 60):
    r = radius_for(t, sample, want)
    counts = quiet(lambda: t.radius_count(pts, r))
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    dist, idx = np.empty(int(offsets[-1]), np.float32), np.empty(int(offsets[-1]), np.int64)
    row = {"what": f"radius, mean count {counts.mean():.1f}", "r": r, "entries": int(offsets[-1]), "longest_segment": int(counts.max())}
    c = timed(lambda: t.radius_count(pts, r), ("count_ms",))
    q = timed(lambda: t.radius_query(pts, r, offsets=offsets, out=(dist, idx)), ("fill_ms", "sort_ms", "unpack_ms"))
    row.update({"count_kernel_ms": c["count_ms"], "count_call_ms": c["call_ms"], "fill_ms": q["fill_ms"], "sort_ms": q["sort_ms"],
                "unpack_ms": q["unpack_ms"], "query_call_ms": q["call_ms"]})
    res["rows"].append(row)
    print(row, flush=True)
for k in (16, 64):
    row = {"what": f"knn k={k}", "knn_query_call_ms": timed(lambda: t.knn_query(pts, k))["call_ms"],
           "estimate_normals_call_ms": timed(lambda: t.estimate_normals(k, compat=True, want=False))["call_ms"]}
    res["rows"].append(row)
    print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
