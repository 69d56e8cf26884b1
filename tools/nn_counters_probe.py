"""Developer probe (developer build: PCR_LIB=.../libpcr_hip_dev.so): work counters of the point search per query at every pose of
a bench config's Gauss-Newton trajectory -- row segments, candidates tested, and, on a target in the old order (PCR_XORDER=0),
how many of those candidates a scan that knew the order of x inside a row could NOT have skipped: against the best distance at
the time of the test (x_now) and against the final best (x_final); and the queries outside the target's grid box against those
inside it (nn_counters_edge; PCR_EDGE_SEED=0 in the environment: without their seed).   python tools/nn_counters_probe.py [config ...]"""
import os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B
from point_cloud_registration_amd import _capi
ctx = _capi.get_context(0)
for cfg in sys.argv[1:] or ["plane_b01"]:
    kind_name, n_target, n_scan, vs, _ = B.CONFIGS[cfg]
    target = B.make_cloud(n_target, seed=0, config=cfg); scan, _ = B.make_scan(cfg, target, n_scan, seed=2)
    tgt = _capi.Target.points(ctx, target); tgt.estimate_normals(15, compat=n_target <= 2_000_000, want=False)
    sc = _capi.Scan(ctx, scan)
    print(cfg, "x_ordered", tgt.index_info()["x_ordered"], flush=True)
    T, it, tr = _capi.align(tgt, sc, _capi.PLANE, np.eye(4), 30, 1e-3, 2.0, want_trace=True)
    for k in range(it):
        c = _capi.nn_counters(tgt, sc, tr[k, :16].reshape(4, 4), 2.0)
        print(cfg, "pose", k, {a: round(b, 2) for a, b in c.items()},
              {a: round(b, 2) for a, b in _capi.nn_counters_x(tgt, sc, tr[k, :16].reshape(4, 4), 2.0).items()}, flush=True)
        print(cfg, "pose", k, "edge", {a: round(b, 3) for a, b in _capi.nn_counters_edge(tgt, sc, tr[k, :16].reshape(4, 4), 2.0).items()}, flush=True)
