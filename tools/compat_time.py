#!/usr/bin/env python3
"""Developer probe: what the compatibility kernels cost (csrc/compat.hip), kernel by kernel, and what sc2_pose costs beside
ransac_pose and fgr_pose.

    python tools/compat_time.py [out.json] [M ...]

With PCR_COMPAT_TIMES=1 the library brackets k_compat_bits, k_compat_degrees and k_compat_consensus of a pcr_compat_consensus
call with HIP events on the context's stream and reports their milliseconds on stderr; this tool collects those lines (stderr
goes through a temporary file) and prints the median of five timed calls after two warm-ups, beside the time of the whole call
by events around it.

Rows: M = 2 000, 8 192 and 32 768 matches (or the M given), 64 seeds, k = 20, each on two scenes -- "sparse": 1.5 % of the
matches a rigid copy with noise 0.02, the rest unrelated points of a 20 x 20 x 4 slab, d = 0.1 (C has a density of 1-2 %);
"dense": every match an inlier, the bad case of one wave per row, which reads a row of C for every set bit.  What
k_compat_degrees reads is counted from the result: the sum of deg1 rows of W 64-bit words; the rate printed is that over its
time.  Then, on the sparse scene of M = 2 000: sc2_pose, ransac_pose and fgr_pose at their defaults, whole calls by the host
clock (each ends synchronised), with the planted matches each one finds."""
import json
import os
import sys
import time

import numpy as np

os.environ["PCR_COMPAT_TIMES"] = "1"              # (read once, by the first call)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from timing import WARM, REPS, timed, quiet  # noqa: E402
import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.math_tools import expSO3  # noqa: E402

args = sys.argv[1:]
out_path = args[0] if args and not args[0].isdigit() else None
sizes = [int(a) for a in args if a.isdigit()] or [2000, 8192, 32768]
D, NOISE, SEEDS, K = 0.1, 0.02, 64, 20

ctx = _capi.get_context(0)


def scene(m, share, seed):
    """m matches in a 20 x 20 x 4 slab, a share of them under a rotation by 2 rad and t = (3, -2, 1) with noise, the rest
    unrelated points -> (src, dst, planted)"""
    rng = np.random.default_rng(seed)
    src = (rng.uniform(-10, 10, (m, 3)) * [1, 1, 0.2]).astype(np.float32)
    w = rng.normal(size=3)
    R, t = expSO3(w * (2.0 / np.linalg.norm(w))), np.array([3.0, -2.0, 1.0])
    dst = rng.uniform(-10, 10, (m, 3)) * [1, 1, 0.2]
    rows = rng.permutation(m)[:int(round(share * m))]
    dst[rows] = src[rows] @ R.T + t + rng.normal(size=(len(rows), 3)) * NOISE
    planted = np.zeros(m, bool)
    planted[rows] = True
    return src, np.ascontiguousarray(dst, np.float32), planted


res = {"warmups": WARM, "timed_calls": REPS, "n_seeds": SEEDS, "k": K, "d": D, "rows": [], "poses": []}
for m in sizes:
    for what, share in (("sparse", 0.015), ("dense", 1.0)):
        src, dst, _ = scene(m, share, seed=m)
        box = []
        t, line = timed(lambda: box.append(_capi.compat_consensus(ctx, src, dst, D, SEEDS, K)), ("bits_ms", "degrees_ms", "consensus_ms"), report=True)
        deg1 = box[-1]["deg1"]
        words = (m + 63) // 64
        read = float(deg1.sum()) * words * 8
        row = {"what": f"{what} M {m}", "density": float(deg1.sum()) / (float(m) * m), "bits_kernel_ms": t["bits_ms"],
               "degrees_kernel_ms": t["degrees_ms"], "consensus_kernel_ms": t["consensus_ms"], "call_ms": t["call_ms"],
               "degrees_row_bytes": read, "degrees_row_TB_per_s": read / (t["degrees_ms"] * 1e-3) / 1e12 if t["degrees_ms"] > 0 else None,
               "report": line}
        res["rows"].append(row)
        print(row, flush=True)

# the three ways from matches to a pose on one 1.5 % scene, at their defaults
m = 2000
src, dst, planted = scene(m, 0.015, seed=0)
rows = np.arange(m)
for name, fn in (("sc2_pose", pcr.sc2_pose), ("ransac_pose", pcr.ransac_pose), ("fgr_pose", pcr.fgr_pose)):
    ms, info = [], None
    for r in range(WARM + REPS):
        t0 = time.perf_counter()
        _, info = quiet(lambda: fn(src, dst, rows, rows, D, return_info=True))
        if r >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    row = {"what": f"{name} M {m}, {int(planted.sum())} planted", "call_ms": float(np.median(ms)), "count": int(info["count"]),
           "planted_found": int((info["inliers"] & planted).sum())}
    res["poses"].append(row)
    print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
