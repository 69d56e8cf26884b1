"""The cases tests/test_gpu_direct_bits.py compares and tools/make_golden_direct_bits.py records: what the direct VGICP entry
points return on g2_mini_street (218 kept voxels, scans of at most 2000 points) -- every neighbourhood, both gates, the scan
prefixes that walk a lane, a partial wave, a wave, a partial block and more than one block, plain and under two robust kernels;
residuals; a five-iteration align with its trace; the target with no kept voxel -- and one plain, one robust and two adaptive
passes of each of the four match-list aligners, whose launches go through the same host scaffold (csrc/match_pass.h).

The inputs are those of tests/test_gpu_direct.py (its "plane" and "spd" sides) or seeded here; every call takes milliseconds."""
import numpy as np

import gicp_cases as gc

EPS = 1e-3
COVS = ("plane", "spd")
NEIGHBORS = (1, 7, 27)
GATES = (0.8, 2.0)
PREFIXES = (0, 1, 63, 64, 65, 257, 2000)
KERNELS = (None, ("cauchy", 1.0), ("tukey", 1.0))
RESIDUALS_AT = 257
RESIDUALS_GATE = 2.0
ALIGN_ITERATIONS = 5
UNITS = ("gicp", "vgicp", "symm", "color")
UNIT_ROBUST = ("cauchy", 1.0)
UNIT_ADAPTIVE = (("trim", 0.8, 1.0), ("huber", 0.5, 1.0))
LAMBDA = 0.968


def _scan(capi, ctx, g2, n, setter, payload):
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER)
    getattr(s, setter)(np.ascontiguousarray(payload[:n]))
    return s


def direct_sides(capi, ctx, g2):
    """name -> (scan covariances float32 (2000, 6), voxel target with its covariances set), as the ``sides`` of
    tests/test_gpu_direct.py build "plane" and "spd"."""
    rng = np.random.default_rng(0)
    cp_plane = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER).estimate_covariances(10, capi.COV_PLANE, EPS)
    cp_spd = gc.random_spd(len(g2["source"]), rng)
    cv_spd = gc.random_spd(218, rng).astype(np.float64)
    out = {}
    for name in COVS:
        t = capi.Target.voxels(ctx, g2["target"], float(g2["voxel_size"]), 10)
        if name == "plane":
            t.set_voxel_covariances(capi.COV_PLANE, EPS)
        else:
            t.set_voxel_covariances(cov=cv_spd)
        out[name] = (cp_spd if name == "spd" else cp_plane, t)
    return out


def run_direct(capi, ctx, g2):
    res = {}
    sides = direct_sides(capi, ctx, g2)
    T = g2["T"]
    for name, (cp, t) in sides.items():
        scans = {n: _scan(capi, ctx, g2, n, "set_covariances", cp) for n in PREFIXES}
        for nb in NEIGHBORS:
            for gate in GATES:
                # [prefix][kernel][29]
                res[f"linearize/{name}/{nb}/{gate}"] = np.stack([np.stack([
                    capi.vgicp_direct_linearize(t, scans[n], T, gate, nb, robust=k and capi.check_robust(*k)) for k in KERNELS]) for n in PREFIXES])
    cp, t = sides["plane"]
    s = _scan(capi, ctx, g2, RESIDUALS_AT, "set_covariances", cp)
    full = _scan(capi, ctx, g2, 2000, "set_covariances", cp)
    for nb in NEIGHBORS:
        res[f"residuals/plane/{nb}"] = capi.vgicp_direct_residuals(t, s, T, RESIDUALS_GATE, nb)
        for k in KERNELS[:2]:
            Tout, iters, trace = capi.vgicp_direct_align(t, full, T, ALIGN_ITERATIONS, 1e-12, 2.0, nb, robust=k and capi.check_robust(*k),
                                                         want_trace=True)
            # T (16), the iteration count, then the trace rows
            res[f"align/plane/{nb}/{k[0] if k else 'plain'}"] = np.concatenate([np.asarray(Tout).reshape(16), [float(iters)], trace.reshape(-1)])
    empty = capi.Target.voxels(ctx, np.ascontiguousarray(g2["target"][:5]), 1.0)
    empty.set_voxel_covariances(capi.COV_RAW)
    for nb in NEIGHBORS:
        res[f"empty/linearize/{nb}"] = capi.vgicp_direct_linearize(empty, s, T, 0.8, nb)
        res[f"empty/residuals/{nb}"] = capi.vgicp_direct_residuals(empty, s, T, 0.8, nb)
    return res


def unit_sides(capi, ctx, g2):
    """unit -> (target, scan, the unit's pass parameter): g2's clouds with seeded payloads -- random SPD covariances, random unit
    scan normals against the fixture's plane normals, a random intensity field with random gradients."""
    src, tgt = g2["source"], g2["target"]
    rng = np.random.default_rng(18)
    cp, cq, cv = gc.random_spd(len(src), rng), gc.random_spd(len(tgt), rng), gc.random_spd(218, rng).astype(np.float64)
    n_p = rng.normal(size=(len(src), 3))
    n_p = (n_p / np.linalg.norm(n_p, axis=1, keepdims=True)).astype(np.float32)
    I_q, I_p = rng.uniform(0, 1, len(tgt)).astype(np.float32), rng.uniform(0, 1, len(src)).astype(np.float32)
    G = (0.3 * rng.normal(size=(len(tgt), 3))).astype(np.float32)
    gicp = capi.Target.points(ctx, tgt)
    gicp.set_covariances(cq)
    vgicp = capi.Target.voxels(ctx, tgt, float(g2["voxel_size"]), 10)
    vgicp.set_voxel_covariances(cov=cv)
    symm = capi.Target.points(ctx, tgt)
    symm.set_normals(g2["plane_normals"])
    color = capi.Target.points(ctx, tgt)
    color.set_normals(g2["plane_normals"])
    color.set_intensity(I_q, G)
    return {"gicp": (gicp, _scan(capi, ctx, g2, 2000, "set_covariances", cp), ()),
            "vgicp": (vgicp, _scan(capi, ctx, g2, 2000, "set_covariances", cp), ()),
            "symm": (symm, _scan(capi, ctx, g2, 2000, "set_normals", n_p), (0.0,)),
            "color": (color, _scan(capi, ctx, g2, 2000, "set_intensity", I_p), (LAMBDA,))}


def run_units(capi, ctx, g2):
    res = {}
    T, md = g2["T"], float(g2["max_dist"])
    for unit, (t, s, extra) in unit_sides(capi, ctx, g2).items():
        res[f"unit/{unit}/linearize"] = getattr(capi, f"{unit}_linearize")(t, s, T, md, *extra)
        res[f"unit/{unit}/robust"] = getattr(capi, f"{unit}_linearize_robust")(t, s, T, md, *extra, robust=capi.check_robust(*UNIT_ROBUST))
        for ad in UNIT_ADAPTIVE:
            out, stats = getattr(capi, f"{unit}_linearize_adaptive")(t, s, T, md, *extra, adaptive=capi.check_adaptive(*ad))
            res[f"unit/{unit}/adaptive/{ad[0]}"] = np.concatenate([out, stats])          # 29 sums, then tau, c, n_le, k
    return res


def run_all(capi, ctx, g2):
    res = run_direct(capi, ctx, g2)
    res.update(run_units(capi, ctx, g2))
    return {k: np.array(v, dtype=np.float64) for k, v in res.items()}
