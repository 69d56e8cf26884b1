"""Cases for the list sets of a point target (near / mid / far: pcr_internal.h, PCR_HALO2_FRAC, PCR_HALO3_FRAC) and one function,
``run_all``, that pushes every case through the split pass (search + reduce: the only reader of the deeper sets), the fused
small-scan pass, both Gauss-Newton loops and ``align_batch``.  tests/test_gpu_list_sets.py runs it in its own process with the
developer switch PCR_LIST_SET unset (the sets by the size of the step) and set to 0, 1 and 2 (one set whatever the step), and as
``python tests/list_set_cases.py OUT.npz`` in child processes under PCR_DEEP_LISTS=0 (the first set only) and PCR_XORDER=0.

Hand-placed targets use a cell of 1 m (cell_hint) and queries in the scan's own order (FLAG_NO_SCAN_SORT), so a pass' matches
(``Scan.matches``: cell-sorted target indices) map back to the caller's indices through a probe pass of the target's own points
over the target: point i matches itself, which gives its cell-sorted position.  The same fourteen probe passes earn the target
its deeper sets.  The poses of a hand-placed case are pure translations along x by float32 amounts, so the moved queries are
exact in NumPy; their steps straddle the three thresholds (0.12, 0.4 and 1.5 cell, from which on a pass reads the near set
again): 0.11, 0.13, 0.39, 0.41, 1.49 and 1.51 cell, then back by 4.04.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import edge_seed_cases as ec                                                    # noqa: E402
import rows_once_cases as rc                                                    # noqa: E402
from edge_seed_cases import _f32, _moved, _sums_both, brute                     # noqa: E402,F401

GATE = 2.0
HALOS = (0.1, 0.25, 0.35)                              # x cell: near, mid, far
SHIFTS = tuple(float(np.float32(v)) for v in (0.0, 0.11, 0.24, 0.63, 1.04, 2.53, 4.04, 0.0))
WARM = 14
Q0 = (5.5, 3.5, 2.5)                                   # the middle of cell (5, 3, 2): 0.5 from every wall


def shift_pose(dx):
    T = np.eye(4)
    T[0, 3] = dx
    return T


def hand_cases():
    """[(name, target points, queries)]"""
    cases = [("grid_6x6x4", ec.hand_target(), ec.hand_queries()[1])]
    byname = {n: (p, q) for n, p, q, _ in rc.hand_cases()}
    cases.append(("min_grid", *byname["single_row"]))                           # ny = nz = 2
    anchors = list(rc.ANCHORS)
    # the certificate's edge: the match exactly at fmin + halo of a set along x (ring 0 certifies a match closer than that), one
    # ulp nearer and one ulp farther; a decoy a millimetre farther along y, in another cell
    for k, halo in enumerate(HALOS):
        edge = np.float32(np.float32(Q0[0]) + np.float32(0.5) + np.float32(halo))
        for tag, x in (("below", np.nextafter(edge, np.float32(0))), ("at", edge), ("above", np.nextafter(edge, np.float32(9)))):
            decoy = (Q0[0], Q0[1] + float(x) - Q0[0] + 1e-3, Q0[2])
            cases.append((f"edge_set{k}_{tag}", _f32(anchors + [(float(x), Q0[1], Q0[2]), decoy]), _f32([Q0])))
    # an empty own cell whose list exists from the mid set on (the nearest point 0.2 into the next cell) and in the far set
    # only (0.3 into it); each with a farther point two cells away
    cases.append(("empty_cell_mid", _f32(anchors + [(6.2, 3.45, 2.6), (3.7, 3.1, 2.9)]), _f32([(5.6, 3.4, 2.6)])))
    cases.append(("empty_cell_far", _f32(anchors + [(6.3, 3.45, 2.6), (3.6, 3.1, 2.9)]), _f32([(5.6, 3.4, 2.6)])))
    # an equidistant pair, 0.75 away (exact), each a quarter of a cell into a neighbouring cell: on the edge of the mid lists,
    # inside the far ones, outside the near ones; in both index orders
    a, b = (6.25, 3.5, 2.5), (5.5, 4.25, 2.5)
    cases.append(("tie_ab", _f32(anchors + [a, b]), _f32([Q0])))
    cases.append(("tie_ba", _f32(anchors + [b, a]), _f32([Q0])))
    return cases


def street_case():
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=61)
    scan, _ = perturbed_scan(target, 2_000, seed=62)
    return _f32(target), _f32(street_normals(target)), _f32(scan)


def _warm(capi, ctx, tgt, probe, kind=None):
    with ctx.pipeline(variant=1, reuse=0):
        for _ in range(WARM):
            capi.linearize(tgt, probe, capi.ICP if kind is None else kind, np.eye(4), GATE)


def run_hand(capi, ctx, res):
    for name, pts, q in hand_cases():
        tgt = capi.Target.points(ctx, pts, cell_hint=1.0)
        probe = capi.Scan(ctx, pts, flags=capi.FLAG_NO_SCAN_SORT)
        _warm(capi, ctx, tgt, probe)
        pos = probe.matches()                          # cell-sorted position of every point
        res[name + "/pos"] = pos
        info = tgt.index_info()
        res[name + "/dims"], res[name + "/cell"] = np.array(info["dims"]), np.array(info["cell"])
        res[name + "/sets"] = np.array(info["list_sets"], np.float64)
        back = np.full(pts.shape[0], -1, np.int64)
        back[pos[pos >= 0]] = np.nonzero(pos >= 0)[0]
        sc = capi.Scan(ctx, q, flags=capi.FLAG_NO_SCAN_SORT)
        idx, sums = [], []
        with ctx.pipeline(variant=1, reuse=0):
            for dx in SHIFTS:                          # the first pass has no history: the deepest set
                sums.append(capi.linearize(tgt, sc, capi.ICP, shift_pose(dx), GATE).copy())
                m = sc.matches()
                idx.append(np.where(m >= 0, back[np.maximum(m, 0)], -1))
        res[name + "/idx"], res[name + "/sums"] = np.stack(idx), np.stack(sums)
        with ctx.pipeline(variant=0, reuse=0):
            res[name + "/fused"] = np.stack([capi.linearize(tgt, sc, capi.ICP, shift_pose(dx), GATE).copy() for dx in SHIFTS])
        sc.close(); probe.close(); tgt.close()


def run_trajectory(capi, ctx, res, name, target, normals, scan):
    """the five poses of the scan's own trajectory on a warmed target: matches and sums of host-driven split passes (each after the
    pose before it: the steps of a Gauss-Newton run, large to small), the fused pass, both loops with their traces, align_batch;
    and the same split passes on a fresh target"""
    tgt = capi.Target.points(ctx, target, normals)
    sc = capi.Scan(ctx, scan)
    _warm(capi, ctx, tgt, sc, capi.PLANE)
    info = tgt.index_info()
    res[name + "/heavy"], res[name + "/sets"] = np.array(info["heavy"]), np.array(info["list_sets"], np.float64)
    res[name + "/sets_per_cell"] = res[name + "/sets"][:, 0] / info["cell"]
    both = capi.FLAG_ICP_RR_QUIRK
    for kname, kind in (("icp", capi.ICP), ("plane", capi.PLANE)):
        for lname, flag in (("device", capi.FLAG_DEVICE_LOOP), ("host", capi.FLAG_HOST_LOOP)):
            with ctx.pipeline(variant=1, reuse=0):
                T, it, trace = capi.align(tgt, sc, kind, np.eye(4), 30, 1e-3, GATE, flags=both | flag, want_trace=True)
            res[f"{name}/{lname}_{kname}"] = np.concatenate([np.asarray(T, np.float64).reshape(-1), [float(it)], trace[:it].reshape(-1)])
            if (kname, lname) == ("plane", "device"):
                poses = [trace[k, :16].reshape(4, 4).copy() for k in range(min(it, 5))]
                poses += [np.asarray(T, np.float64).reshape(4, 4).copy()] * (5 - len(poses))
    res[name + "/poses"] = np.stack(poses)
    fresh = capi.Target.points(ctx, target, normals)
    sc_f = capi.Scan(ctx, scan)
    for tag, t, s in (("warm", tgt, sc), ("fresh", fresh, sc_f)):
        sums, ms = [], []
        with ctx.pipeline(variant=1, reuse=0):
            for P in poses:
                for kind in (capi.ICP, capi.PLANE):
                    sums.append(capi.linearize(t, s, kind, P, GATE).copy())
                    ms.append(s.matches())
        res[f"{name}/{tag}_sums"], res[f"{name}/{tag}_matches"] = np.stack(sums), np.stack(ms)
    res[name + "/fresh_sets"] = np.array(fresh.index_info()["list_sets"], np.float64)
    res[name + "/both"] = np.stack([_sums_both(capi, ctx, tgt, sc, kind, P) for P in poses for kind in (capi.ICP, capi.PLANE)])
    batch = capi.ScanBatch(ctx, [scan, scan[:1000]])
    Ts = np.stack([poses[0], poses[1]])
    for kname, kind in (("icp", capi.ICP), ("plane", capi.PLANE)):
        Tb, itb, stb, trb = capi.align_batch(tgt, batch, kind, Ts, 30, 1e-3, GATE, want_trace=True)
        res[f"{name}/batch_{kname}"] = np.concatenate([np.asarray(Tb).reshape(-1), np.asarray(itb, np.float64), np.asarray(stb, np.float64)])
        res[f"{name}/batch_{kname}_sums"] = capi.linearize_batch(tgt, batch, kind, Ts, GATE)
    batch.close()
    sc_f.close(); fresh.close(); sc.close(); tgt.close()


def run_all(capi, ctx):
    res = {}
    run_hand(capi, ctx, res)
    run_trajectory(capi, ctx, res, "street", *street_case())
    run_trajectory(capi, ctx, res, "heavy", *ec.heavy_case())
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from point_cloud_registration_amd import _capi
    np.savez(sys.argv[1], **run_all(_capi, _capi.get_context(0)))
