#!/usr/bin/env python3
"""Developer probe: what a VGICP pass costs with direct voxel neighbourhoods (csrc/vgicp_direct.hip) beside the nearest-centroid
pass (csrc/vgicp.hip: a float64 centroid search + k_vgicp_reduce).

    python tools/direct_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points) in 1 m voxels against its own perturbed scan (perturbed_scan(target, None, seed=2), every
point), the scan's covariances estimated once (k = 10, plane).  Per form -- VGICP() and neighbors = 1 / 7 / 27, gate 2.0, plain
and under a Cauchy kernel -- the whole pass (pcr_vgicp_linearize / pcr_vgicp_direct_linearize on the uploaded scan) by HIP events
around the call on the context's stream, which, the call ending synchronised, spans what the host does in it as well.  The
direct kernel and the fold alone come from the library's own events (PCR_DIRECT_TIMES=1), taken in a second process so that the
whole-pass times above carry no bracket.  Every figure: the median of the timed calls after the warm-ups (tools/timing.py: five
after two).  The kept pairs of every form are printed beside the times."""
import json
import os
import subprocess
import sys

import numpy as np

KERNELS = os.environ.get("PCR_DIRECT_TIMES") == "1"          # the second process: kernel and fold times
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, quiet, timed  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import perturbed_scan, street  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
MAX_DIST = 2.0
PHASES = ("kernel_ms", "fold_ms") if KERNELS else ()

ctx = _capi.get_context(0)
target = street(n, seed=0)
scan = perturbed_scan(target, None, seed=2)[0]
t = _capi.Target.voxels(ctx, target, 1.0)
t.set_voxel_covariances(_capi.COV_PLANE, 1e-3)
s = _capi.Scan(ctx, scan, flags=_capi.FLAG_KEEP_ORDER)
s.estimate_covariances(10, _capi.COV_PLANE, 1e-3, want=False)
T = np.eye(4)
T[:3, 3] = [0.01, -0.02, 0.015]

rows = []
if not KERNELS:
    out = quiet(lambda: _capi.vgicp_linearize(t, s, T, MAX_DIST))
    rows.append({"what": "VGICP(), nearest centroid", "pairs": int(out[28]), **timed(lambda: _capi.vgicp_linearize(t, s, T, MAX_DIST))})
    print(rows[-1], flush=True)
for nb in _capi.NEIGHBORS:
    for robust, label in ((None, ""), ((_capi.ROBUST_CAUCHY, 1.0), ", Cauchy")):
        out = quiet(lambda: _capi.vgicp_direct_linearize(t, s, T, MAX_DIST, nb, robust=robust))
        rows.append({"what": f"neighbors = {nb}{label}", "pairs": int(out[28]),
                     **timed(lambda: _capi.vgicp_direct_linearize(t, s, T, MAX_DIST, nb, robust=robust), PHASES)})
        print(rows[-1], flush=True)
if KERNELS:
    print("KERNEL_ROWS " + json.dumps(rows))
    sys.exit(0)

child = subprocess.run([sys.executable, os.path.abspath(__file__), str(n)], env=dict(os.environ, PCR_DIRECT_TIMES="1"),
                       capture_output=True, text=True, check=True)
kernels = json.loads(next(line for line in child.stdout.splitlines() if line.startswith("KERNEL_ROWS "))[len("KERNEL_ROWS "):])
for row in rows:
    for k in kernels:
        if k["what"] == row["what"]:
            row["kernel_ms"], row["fold_ms"] = k["kernel_ms"], k["fold_ms"]
res = {"n": n, "scan": len(scan), "kept_voxels": t.size(), "max_dist": MAX_DIST, "warmups": WARM, "timed_calls": REPS, "rows": rows}
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
