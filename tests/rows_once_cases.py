"""Cases for the row-once traversal of the plain float32 point search on x-ordered targets (nn_device.h: nn_rows_x) and one
function, ``run_all``, that pushes every case through the library: ``nn_query`` (gated at GATES and ungated), the split pass
(search + reduce) and the fused small-scan pass.  tests/test_gpu_rows_once.py runs it in its own process (the shallow extended
lists, the default), in-process again with PCR_HALO=1 (lists of a whole cell: nn_ring0 returns kstart = 2), and as
``python tests/rows_once_cases.py OUT.npz hand|street`` in child processes under PCR_HALO=0 (no lists) and PCR_XORDER=0 (the old
order inside a cell: the untouched ring loop).

Hand-placed cases use a cell of 1 m (cell_hint): the grid's origin is the min corner of the points and the box has
floor(extent) + 2 cells per axis.  Every hand-placed target carries two anchors, (0, 0, 0) and (11.5, 6.5, 4.5): a box of at
least 13 x 8 x 6 cells from the origin -- wider than the 8 x 6 x 4 the cases were first drawn on, so that a point 5 cells away in
x and a row 3 cells away in y or z fit around one query without an anchor coming nearer than the point under test.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from edge_seed_cases import _f32, _fma32, _moved, _sums_both, brute          # noqa: E402  (the float32 formula, emulated)

GATES = (2.0, 6.5)
ANCHORS = [(0.0, 0.0, 0.0), (11.5, 6.5, 4.5)]
Q0 = (5.5, 3.4, 2.6)                                   # cell (5, 3, 2), 0.5 / 0.4 / 0.6 into it


def _q(dx=0.0, dy=0.0, dz=0.0):
    return (Q0[0] + dx, Q0[1] + dy, Q0[2] + dz)


def hand_cases():
    """[(name, target points, queries, tie)]: `tie` marks the cases with a deliberate equidistant pair"""
    cases = []

    def add(name, placed, queries, tie=False, anchors=True):
        cases.append((name, _f32((ANCHORS if anchors else []) + list(placed)), _f32(queries), tie))

    # the nearest point in the query's own row, 1, 3 and 5 cells away in x, every other row empty; then with a farther
    # point in an adjacent row (rings meet the adjacent row first, rows the own row)
    for d, sgn in ((1, 1), (3, -1), (5, 1)):
        own = _q(dx=sgn * (d + 0.13), dy=0.05, dz=-0.05)
        add(f"own_row_{d}", [own], [Q0])
        adj = {1: _q(dx=0.6, dy=1.1), 3: _q(dx=-3.3, dy=1.05), 5: _q(dx=5.3, dy=-1.05)}[d]
        add(f"own_row_{d}_adjacent_farther", [own, adj], [Q0])
        add(f"own_row_{d}_adjacent_farther_z", [own, (adj[0], Q0[1], Q0[2] + (adj[1] - Q0[1]))], [Q0])
    # the nearest point in a row at |dy| = m or |dz| = m, more than m cells away in x: outside the shell clip cx -+ m of ring m
    for m in (1, 2, 3):
        add(f"row_dy+{m}", [_q(dx=m + 1.6, dy=m + 0.2)], [Q0])
        add(f"row_dy-{m}", [_q(dx=-(m + 1.6), dy=-(m + 0.2))], [Q0])
        add(f"row_dz+{m}", [_q(dx=-(m + 1.6), dy=0.05, dz=m + 0.1)], [Q0])
        if m < 3:
            add(f"row_dz-{m}", [_q(dx=m + 1.6, dy=-0.05, dz=-(m + 0.3))], [Q0])
        else:                                          # (three cells below the query's there is no cell: from the bottom layer up)
            add(f"row_dz-{m}", [(Q0[0] + m + 1.6, Q0[1], 0.3)], [(Q0[0], Q0[1], 3.6)])
        add(f"row_dy{m}_dz{m}", [_q(dx=m + 1.3, dy=-(m + 0.1), dz=(m + 0.2) if m < 3 else 2.3)], [Q0])
    # an equidistant pair (3-4-5 in eighths: exact in float32), one far in x in the own row, one in a neighbouring row; swapped
    tq = (5.5, 3.25, 2.5)
    far_x, beside = (8.0, 3.25, 2.5), (7.5, 4.75, 2.5)
    add("tie_own_row_first", [far_x, beside], [tq], tie=True)
    add("tie_neighbour_row_first", [beside, far_x], [tq], tie=True)
    # the gap field: an own cell with gap 2 and 3 whose only occupied cells sit at |dx| = gap in a row with m < gap
    for gap in (2, 3):
        for m in range(gap):
            left, right = _q(dx=-(gap + 0.2), dy=m * 1.0 + 0.05, dz=0.02), _q(dx=gap + 0.35, dy=-(m * 1.0) - 0.05, dz=-0.02)
            add(f"gap{gap}_m{m}_left", [left], [Q0])
            add(f"gap{gap}_m{m}_right", [right], [Q0])
            add(f"gap{gap}_m{m}_both", [left, right], [Q0])
    # extended lists: certified by the list alone (the match deep inside the own cell); not certified (the own cell's point
    # far, the nearest one 0.3 into the next cell: beyond a halo of 0.1 cell); the match a halo copy; an empty own cell
    add("list_certified", [_q(dx=0.05, dy=0.05, dz=0.02), _q(dx=1.4, dy=0.1)], [Q0])
    add("list_not_certified", [(5.1, 3.4, 2.6), (6.3, 3.45, 2.6), (9.2, 3.4, 2.6)], [(5.95, 3.4, 2.6)])
    add("list_halo_copy", [(5.1, 3.4, 2.6), (6.05, 3.45, 2.6), (5.9, 4.6, 2.6)], [(5.95, 3.4, 2.6)])
    add("list_empty_own_cell", [(6.04, 3.45, 2.6), (4.2, 3.1, 2.9)], [(5.6, 3.4, 2.6)])
    # the gate: a point exactly at max_dist = 2 along x in the own row (strict: no match), and one ulp inside
    gq = (5.5, 3.5, 2.5)
    add("gate_exact", [(7.5, 3.5, 2.5)], [gq])
    add("gate_ulp_inside", [(float(np.nextafter(np.float32(7.5), np.float32(0.0))), 3.5, 2.5)], [gq])
    # a target of a single row of occupied cells (y and z constant: the grid gives such a target ny = nz = 2, the second
    # rows empty) and a target of one point
    line = [(0.37 * i * i / 7.0 + 0.21 * i, 1.0, 1.0) for i in range(15)]
    add("single_row", line, [(-0.6, 1.0, 1.0), (3.3, 1.2, 0.9), (3.3, 2.7, 1.0), (9.1, 1.0, 1.4), (14.9, 0.4, 1.0), (21.0, 1.0, 1.0)], anchors=False)
    add("one_point", [(1.0, 2.0, 3.0)], [(1.2, 2.1, 3.0), (0.2, 2.0, 3.0), (1.0, 3.7, 3.0), (1.0, 2.0, -2.5), (2.6, 3.6, 4.6)], anchors=False)
    # a wide row: 40 points in one row spread over 9 cells, queries at its middle and at both ends (the positional start)
    rng = np.random.default_rng(20271)
    wide = np.stack([np.sort(rng.uniform(1.05, 9.95, 40)), rng.uniform(3.05, 3.95, 40), rng.uniform(2.05, 2.95, 40)], 1)
    add("wide_row", [tuple(p) for p in wide], [(5.5, 3.5, 2.5), (1.2, 3.5, 2.5), (9.8, 3.5, 2.5), (5.5, 4.6, 2.5), (0.4, 3.5, 3.4), (10.7, 2.6, 2.5)])
    return cases


# queries outside the box of a filled target: in x only (the row exists, the range clamps), in y and / or z by 0.3, 1 and 3
# cells, beyond the gate from the box
FILL_BOX = np.array([9.0, 6.0, 4.0])


def fill_target():
    rng = np.random.default_rng(20272)
    p = rng.uniform(0.0, 1.0, (260, 3)) * [7.6, 4.6, 2.6]
    p[0], p[1] = 0.0, [7.6, 4.6, 2.6]
    return _f32(p)


def fill_queries():
    rng = np.random.default_rng(20273)
    names, q = [], []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                for dist in (0.3, 1.0, 3.0, 7.0):
                    inside = rng.uniform(0.15, 0.7, 3) * FILL_BOX
                    names.append(f"out{sx:+d}{sy:+d}{sz:+d}_{dist}")
                    q.append([(-dist if s < 0 else FILL_BOX[a] + dist) if s else inside[a] for a, s in enumerate((sx, sy, sz))])
    for k in range(24):                                # and inside the box
        names.append(f"in_{k}")
        q.append(rng.uniform(0.02, 0.98, 3) * [7.6, 4.6, 2.6])
    return names, _f32(q)


def d2_all(pts, q):
    """(M, N) float32 squared distances by the library's formula"""
    dx, dy, dz = (_f32(q)[:, None, a] - _f32(pts)[None, :, a] for a in range(3))
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


def unique_nearest(pts, q):
    """per query: is the smallest float32 squared distance attained once?"""
    d2 = np.sort(d2_all(pts, q), axis=1)
    return d2.shape[1] < 2 or bool((d2[:, 0] < d2[:, 1]).all()), d2


def street_case():
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=51)
    scan, _ = perturbed_scan(target, 2_000, seed=52)
    return _f32(target), _f32(street_normals(target)), _f32(scan)


def run_hand(capi, ctx):
    res = {}
    eye = np.eye(4)
    sets = [(n, p, q) for n, p, q, _ in hand_cases()] + [("fill", fill_target(), fill_queries()[1])]
    for name, pts, q in sets:
        tgt = capi.Target.points(ctx, pts, cell_hint=1.0)
        info = tgt.index_info()
        res[name + "/x_ordered"], res[name + "/halo"] = np.array(info["x_ordered"]), np.array(info["halo"])
        res[name + "/cell"], res[name + "/dims"] = np.array(info["cell"]), np.array(info["dims"])
        res[name + "/nn_d_inf"], res[name + "/nn_i_inf"] = tgt.nn_query(q)
        sc = capi.Scan(ctx, q)
        for gate in GATES:
            res[f"{name}/nn_d_{gate}"], res[f"{name}/nn_i_{gate}"] = tgt.nn_query(q, gate)
            sums = []
            for variant in (1, 0):                     # search + reduce (the split path), the fused small-scan kernel
                with ctx.pipeline(variant=variant, reuse=0):
                    sums.append(capi.linearize(tgt, sc, capi.ICP, eye, gate).copy())
            res[f"{name}/sums_{gate}"] = np.stack(sums)
        sc.close(); tgt.close()
    return res


def run_street(capi, ctx):
    """matches at the five poses of the scan's own trajectory, the 29 sums of the split and the fused path (ICP and PlaneICP)
    and align_batch with two items"""
    res = {}
    target, normals, scan = street_case()
    tgt = capi.Target.points(ctx, target, normals)
    info = tgt.index_info()
    res["street/x_ordered"] = np.array(info["x_ordered"])
    sc = capi.Scan(ctx, scan)
    T, it, trace = capi.align(tgt, sc, capi.PLANE, np.eye(4), 30, 1e-3, 2.0, want_trace=True)
    poses = [trace[k, :16].reshape(4, 4).copy() for k in range(min(it, 5))]
    poses += [np.asarray(T, np.float64).reshape(4, 4).copy()] * (5 - len(poses))
    res["street/poses"] = np.stack(poses)
    res["street/sums"] = np.stack([_sums_both(capi, ctx, tgt, sc, kind, P) for P in poses for kind in (capi.ICP, capi.PLANE)])
    for k, P in enumerate(poses):
        res[f"street/nn_d{k}"], res[f"street/nn_i{k}"] = tgt.nn_query(_moved(P, scan), 2.0)
    batch = capi.ScanBatch(ctx, [scan, scan[:1000]])
    Ts = np.stack([poses[0], poses[1]])
    for kname, kind in (("icp", capi.ICP), ("plane", capi.PLANE)):
        Tb, itb, stb, trb = capi.align_batch(tgt, batch, kind, Ts, 30, 1e-3, 2.0, want_trace=True)
        res[f"street/batch_{kname}"] = np.concatenate([np.asarray(Tb).reshape(-1), np.asarray(itb, np.float64), np.asarray(stb, np.float64)])
        res[f"street/batch_{kname}_sums"] = capi.linearize_batch(tgt, batch, kind, Ts, 2.0)
    batch.close()
    sc.close(); tgt.close()
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from point_cloud_registration_amd import _capi
    run = {"hand": run_hand, "street": run_street}[sys.argv[2]]
    np.savez(sys.argv[1], **run(_capi, _capi.get_context(0)))
