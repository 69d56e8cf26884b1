#!/usr/bin/env python3
"""Developer probe: what the RANSAC kernels cost (csrc/ransac.hip), kernel by kernel.

    python tools/ransac_time.py [out.json]

With PCR_RANSAC_TIMES=1 the library brackets k_ransac_fit, k_pose_score and k_ransac_best of a pcr_ransac_poses call, and
k_pose_score of a pcr_pose_score call, with HIP events on the context's stream and reports their milliseconds on stderr; this
tool collects those lines (stderr goes through a temporary file) and prints the median of five timed calls after two warm-ups,
beside the time of the whole call by events around it.

Rows: (M, H) = (5 000, 2^20) and (50 000, 2^20) correspondences x hypotheses -- k_pose_score scores every valid and invalid
hypothesis alike, so its time does not depend on the data -- and a pcr_pose_score call of 16 poses over 10^6 rows, the shape of
the refinement, where the rows are split over blocks.  The arithmetic of the inlier rule is 27 float32 operations and one
integer add per (pose, row) pair; the floor printed is that count over the packed float32 rate of the chip, two operations per
lane and cycle on every CU: 256 CUs x 64 lanes x 2 x 2.4 GHz = 78.6 T operations/s."""
import json
import os
import sys

import numpy as np

os.environ["PCR_RANSAC_TIMES"] = "1"              # (read once, by the first call)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import WARM, REPS, timed  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
PACKED_OPS = 256 * 64 * 2 * 2.4e9
OPS_PER_PAIR = 28

ctx = _capi.get_context(0)
def pairs(m, seed):
    """Half of the rows a rigid copy with noise, the rest unrelated points."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    src = rng.uniform(-50, 50, (m, 3))
    dst = src @ R.T + [4.0, -7.0, 1.5]
    out = rng.random(m) < 0.5
    dst[out] = rng.uniform(-50, 50, (int(out.sum()), 3))
    return np.ascontiguousarray(src + rng.normal(0, 0.01, (m, 3)), np.float32), np.ascontiguousarray(dst, np.float32)


res = {"warmups": WARM, "timed_calls": REPS, "packed_ops_per_s": PACKED_OPS, "rows": []}
H = 1 << 20
for m in (5_000, 50_000):
    src, dst = pairs(m, seed=m)
    box = []
    t, line = timed(lambda: box.append(_capi.ransac_poses(ctx, src, dst, H, 0, 0.1, 0.9, 1.0)), ("fit_ms", "score_ms", "best_ms"), report=True)
    floor = OPS_PER_PAIR * float(H) * m / PACKED_OPS * 1e3
    row = {"what": f"ransac M {m} H 2^20", "fit_kernel_ms": t["fit_ms"], "score_kernel_ms": t["score_ms"], "best_kernel_ms": t["best_ms"],
           "call_ms": t["call_ms"], "score_floor_ms": floor, "score_share_of_packed_peak": floor / t["score_ms"] if t["score_ms"] > 0 else None,
           "n_valid": box[-1]["n_valid"], "best_count": box[-1]["count"], "report": line}
    res["rows"].append(row)
    print(row, flush=True)
m, b = 1_000_000, 16
src, dst = pairs(m, seed=1)
poses = np.tile(np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), (b, 1))
t, line = timed(lambda: _capi.pose_score(ctx, src, dst, poses, 0.1), ("score_ms",), report=True)
row = {"what": f"pose_score b {b} M {m}", "score_kernel_ms": t["score_ms"], "call_ms": t["call_ms"], "splits": _capi.pose_score_splits(m, b), "report": line}
res["rows"].append(row)
print(row, flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
