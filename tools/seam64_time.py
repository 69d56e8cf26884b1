#!/usr/bin/env python3
"""Developer probe: what the float64 query seam costs (csrc/seam64.hip) next to the float32-query calls it stands beside.

    python tools/seam64_time.py [n_points] [out.json]

Cloud: street(n) (default 1.06 M points) shifted to (500, -300, 20) in float64.  Queries: as many, half of them a few
micrometres off the bisector plane of a target point and its nearest neighbour (near-ties), half ordinary (a target point
moved by centimetres).  Timed with HIP events on the context's stream around each call -- upload, kernel and copy-back,
what a caller of the C ABI pays -- three warm-ups, median of ten:

    pcr_nn_query_dd(q64)            against  pcr_nn_query_f64(float32(q64))
    pcr_knn_query_f64(q64, k)       against  pcr_knn_query(float32 copy of the target, float32(q64), k)     k = 5, 15, 64

and, where the library brackets the kernel itself (profiling, "nn"), the kernel's own milliseconds per call."""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import street  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_060_000
out_path = sys.argv[2] if len(sys.argv) > 2 else None
WARM, REPS = 3, 10

ctx = _capi.get_context(0)
hip = ctypes.CDLL("libamdhip64.so.7")             # (already in the process: the library's own runtime)
stream = ctypes.c_void_p(ctx.stream())
e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0


def timed(fn):
    """(median ms by events around the call, median ms of the bracketed kernel or None)"""
    ms, kern = [], []
    for r in range(WARM + REPS):
        ctx.profile_reset()
        assert hip.hipEventRecord(e0, stream) == 0
        fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        t = ctypes.c_float(0)
        assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
        prof = ctx.profile_read()
        if r >= WARM:
            ms.append(t.value)
            kern.append(prof["nn"][1] if prof["nn"][0] else np.nan)          # (launches, total ms)
    k = float(np.median(kern))
    return float(np.median(ms)), (None if np.isnan(k) else k)


rng = np.random.default_rng(5)
cloud = street(n, seed=0).astype(np.float64) + np.array([500.0, -300.0, 20.0])
t64 = _capi.Target.points(ctx, cloud.astype(np.float32))
assert t64.set_points_f64(cloud)
t32 = _capi.Target.points(ctx, cloud.astype(np.float32))

half = n // 2
pick = rng.choice(n, half, replace=False)
_, nb = t64.knn_query(cloud[pick], 2)
a, b = cloud[pick], cloud[nb[:, 1]]
u = b - a
u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-300)
q64 = np.ascontiguousarray(np.vstack([(a + b) / 2 + u * rng.normal(0, 3e-6, (half, 1)),
                                      cloud[rng.choice(n, n - half)] + rng.normal(0, 0.03, (n - half, 3))]))
q32 = q64.astype(np.float32)
moved = int((t64.nn_query(q64)[1] != t64.nn_query(q32)[1]).sum())

ctx.profile_enable(True)
res = {"n": n, "queries": len(q64), "neighbours_moved_by_rounding_the_query": moved, "rows": []}
rows = [("nn", lambda: t64.nn_query(q64), lambda: t64.nn_query(q32))]
for k in (5, 15, 64):
    rows.append((f"knn{k}", (lambda k=k: t64.knn_query(q64, k)), (lambda k=k: t32.knn_query(q32, k))))
for name, new, old in rows:
    (ms_new, k_new), (ms_old, k_old) = timed(new), timed(old)
    row = {"what": name, "f64_ms": ms_new, "f32_ms": ms_old, "ratio": ms_new / ms_old, "f64_kernel_ms": k_new, "f32_kernel_ms": k_old}
    res["rows"].append(row)
    print(row, flush=True)
ctx.profile_enable(False)
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
