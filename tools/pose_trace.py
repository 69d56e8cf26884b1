#!/usr/bin/env python3
"""Developer probe: per-pose kernel means of a point-target bench config's host-driven passes (tools/pass_gaps.py gives the
means over all poses and the gaps between kernels).  `run` walks the config's Gauss-Newton trajectory ten times; `show` reads the
rocprofv3 rocpd database of that run and prints, per pose, mean / min / max of k_nn_scan and k_reduce_finalize over the last 30
passes (6 rounds of a 5-pose trajectory).  PCR_LIB selects the library (tools/build_rev_lib.sh builds a revision's).
    rocprofv3 --kernel-trace --output-format rocpd -d DIR -o r -- python tools/pose_trace.py run plane_b01
    python tools/pose_trace.py show DIR TAG"""
import glob, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROUNDS = 10


def run(config):
    import numpy as np
    import bench as B
    from point_cloud_registration_amd import _capi
    kind_name, n_target, n_scan, voxel_size, desc = B.CONFIGS[config]
    kind = {"icp": _capi.ICP, "plane": _capi.PLANE}[kind_name]
    ctx = _capi.get_context(0)
    target = B.make_cloud(n_target, seed=0, config=config)
    scan, T_true = B.make_scan(config, target, n_scan, seed=2)
    tgt = _capi.Target.points(ctx, target)
    if kind_name == "plane":
        tgt.estimate_normals(15, compat=n_target <= 2_000_000, want=False)
    sc = _capi.Scan(ctx, scan)
    T_fin, iters, trace = _capi.align(tgt, sc, kind, np.eye(4), 30, 1e-3, 2.0, want_trace=True)
    traj = [trace[i, :16].reshape(4, 4).copy() for i in range(iters)]
    for r in range(ROUNDS):
        for T in traj:
            _capi.linearize(tgt, sc, kind, T, 2.0)
    print(config, "poses", len(traj), "passes", ROUNDS * len(traj), flush=True)


def show(d, tag, nposes=5):
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))
    cur = sqlite3.connect(dbs[-1]).cursor()
    ev = sorted((s, e, re.sub(r"\(.*", "", nm).replace("void ", "")) for nm, s, e in cur.execute("select name, start, end from kernels").fetchall())
    for pat in (r"k_nn_scan", r"k_reduce_finalize"):
        k = [(e - s) / 1e3 for s, e, nm in ev if re.match(pat, nm)][-6 * nposes:]
        names = sorted({nm for s, e, nm in ev if re.match(pat, nm)})
        out = []
        for p in range(nposes):
            v = k[p::nposes]
            out.append(f"pose{p} mean {sum(v) / len(v):6.1f} min {min(v):6.1f} max {max(v):6.1f}")
        print(f"TRACE {tag} {pat} n={len(k)} | " + " | ".join(out) + f" | all-mean {sum(k) / len(k):6.1f}  {names[-1][:60]}", flush=True)


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else show(sys.argv[2], sys.argv[3])
