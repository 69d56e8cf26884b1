#!/usr/bin/env python3
"""Developer probe: the depth of ring 0's extended lists (PCR_HALO, x cell) against the per-pose time and work of k_nn_scan on a
point-target bench config.  One process builds one target per depth (PCR_HALO is read when a target is built; PCR_DEEP_LISTS=0
keeps the lazy second set out, so every pass reads the one depth) and walks the config's Gauss-Newton trajectory on them.
  time: segments of ROUNDS x poses host-driven passes, `0.1, d, 0.1, d' ...`, the whole list TRACES times; `show` reads the
        rocprofv3 rocpd database of that run and prints, per segment and pose, mean / min / max of k_nn_scan over the last 30 passes
        (pose_trace.py's window), then per depth the mean over its segments and, for 0.1, the min-max spread of its segment means.
  counters (developer build, PCR_LIB=.../libpcr_hip_dev.so): row segments and candidates per query and at wave maximum per pose,
        list records per point, MB of the lists, and the ms a target build takes beyond one without lists (min of 3).
    rocprofv3 --kernel-trace --output-format rocpd -d DIR -o r -- python tools/list_depth_sweep.py time plane_b01 0.25,0.45,1.0 PLAN.json
    python tools/list_depth_sweep.py show DIR PLAN.json
    PCR_LIB=.../libpcr_hip_dev.so python tools/list_depth_sweep.py counters plane_b01 0.1,0.25,0.45,1.0"""
import glob, json, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["PCR_DEEP_LISTS"] = "0"
ROUNDS, KEEP, TRACES, BASE = 10, 6, 2, "0.1"


def setup(config):
    import numpy as np
    import bench as B
    from point_cloud_registration_amd import _capi
    kind_name, n_target, n_scan, voxel_size, desc = B.CONFIGS[config]
    kind = {"icp": _capi.ICP, "plane": _capi.PLANE}[kind_name]
    ctx = _capi.get_context(0)
    target = B.make_cloud(n_target, seed=0, config=config)
    scan, T_true = B.make_scan(config, target, n_scan, seed=2)

    def make(depth, normals=True):
        os.environ["PCR_HALO"] = depth
        tgt = _capi.Target.points(ctx, target)
        if normals and kind_name == "plane":
            tgt.estimate_normals(15, compat=n_target <= 2_000_000, want=False)
        return tgt
    sc = _capi.Scan(ctx, scan)
    t0 = make(BASE)
    T_fin, iters, trace = _capi.align(t0, sc, kind, np.eye(4), 30, 1e-3, 2.0, want_trace=True)
    traj = [trace[i, :16].reshape(4, 4).copy() for i in range(iters)]
    return _capi, kind, sc, make, t0, traj


def run_time(config, depths, plan_path):
    _capi, kind, sc, make, t0, traj = setup(config)
    tg = {BASE: t0, **{d: make(d) for d in depths if d != BASE}}
    order = [d for _ in range(TRACES) for x in depths if x != BASE for d in (BASE, x)]
    for d in order:
        for r in range(ROUNDS):
            for T in traj:
                _capi.linearize(tg[d], sc, kind, T, 2.0)
    json.dump({"config": config, "order": order, "nposes": len(traj), "rounds": ROUNDS}, open(plan_path, "w"))
    print(config, "poses", len(traj), "segments", len(order), flush=True)


def show(d, plan_path):
    import sqlite3
    plan = json.load(open(plan_path))
    npz, per, cfg = plan["nposes"], plan["nposes"] * plan["rounds"], plan["config"]
    dbs = sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True))
    cur = sqlite3.connect(dbs[-1]).cursor()
    ev = sorted((s, e, re.sub(r"\(.*", "", nm).replace("void ", "")) for nm, s, e in cur.execute("select name, start, end from kernels").fetchall())
    k = [(e - s) / 1e3 for s, e, nm in ev if re.match(r"k_nn_scan", nm)][-per * len(plan["order"]):]
    assert len(k) == per * len(plan["order"]), (len(k), per, len(plan["order"]))
    means = {}
    for i, depth in enumerate(plan["order"]):
        seg = k[i * per:(i + 1) * per][-KEEP * npz:]
        row = []
        for p in range(npz):
            v = seg[p::npz]
            row.append(sum(v) / len(v))
            print(f"DEPTHSEG {cfg} seg {i:2d} halo {depth} pose{p} mean {row[-1]:6.1f} min {min(v):6.1f} max {max(v):6.1f}", flush=True)
        means.setdefault(depth, []).append(row)
    for depth, rows in means.items():
        m = [sum(r[p] for r in rows) / len(rows) for p in range(npz)]
        sp = [max(r[p] for r in rows) - min(r[p] for r in rows) for p in range(npz)]
        print(f"DEPTH {cfg} halo {depth} segments {len(rows)} | " + " | ".join(f"pose{p} {m[p]:6.1f} (spread {sp[p]:4.1f})" for p in range(npz))
              + f" | all {sum(m) / npz:6.1f}", flush=True)


def run_counters(config, depths):
    _capi, kind, sc, make, t0, traj = setup(config)
    def build_ms(depth):
        best = 1e9
        for _ in range(3):
            t = time.perf_counter(); tg = make(depth, normals=False); best = min(best, (time.perf_counter() - t) * 1e3); del tg
        return best
    none_ms = build_ms("0")
    for depth in depths:
        ms = build_ms(depth)
        tgt = make(depth)
        info = tgt.index_info()
        print(f"DEPTHSET {config} halo {depth} records {info['halo_records']} per_point {info['halo_records'] / info['n']:.2f} "
              f"MB {(info['halo_records'] * 20 + 4 * info['dims'][0] * info['dims'][1] * info['dims'][2]) / 1048576:.1f} "
              f"build_ms {ms:.2f} without_lists_ms {none_ms:.2f} heavy {info['heavy']}", flush=True)
        for p, T in enumerate(traj):
            c = _capi.nn_counters(tgt, sc, T, 2.0)
            print(f"DEPTHCTR {config} halo {depth} pose{p} rows {c['rows_loaded']:.2f} wave_rows {c['wave_rows_loaded']:.2f} "
                  f"cand {c['candidates']:.2f} wave_cand {c['wave_candidates']:.2f}", flush=True)
        del tgt


if __name__ == "__main__":
    if sys.argv[1] == "time":
        run_time(sys.argv[2], sys.argv[3].split(","), sys.argv[4])
    elif sys.argv[1] == "counters":
        run_counters(sys.argv[2], sys.argv[3].split(","))
    else:
        show(sys.argv[2], sys.argv[3])
