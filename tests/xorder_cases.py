"""Cases for the x-ordered range scan (nn_device.h: nn_scan_range_x; Geom::xq) -- the smallest shapes at which a scan that
starts at the query's x and stops on either side can go wrong -- and one function, ``run_all``, that pushes every case through
the library.  tests/test_gpu_xorder.py runs it in its own process (targets in x order) and, as ``python tests/xorder_cases.py
OUT.npz`` with PCR_XORDER=0 in the environment, in a child process (targets in the old order): every array must be equal.

Hand-placed cases use a cell of 1 m (cell_hint): the grid's origin is the bounding box's min corner, the x quantum 2^-16 m.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_DIST = 2.0
ROW_SIZES = (1, 3, 4, 5, 8, 9, 17)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _row_queries(xs):
    """Queries around a row of points with the x coordinates ``xs`` (y, z near 0.15): left of, right of and inside the segment,
    exactly on every point's x, and the same from the rows of cells beside, above and diagonal (ring 1, shell and interior rows)."""
    base = np.concatenate([[-0.7, -0.01, xs.min() - 0.3, xs.max() + 0.3, xs.max() + 0.9, 3.4], xs,
                           0.5 * (xs[:-1] + xs[1:]) if len(xs) > 1 else [], np.linspace(-0.4, 3.2, 13)])
    q = []
    for dy, dz in ((0.2, 0.1), (0.0, 0.0), (1.2, 0.1), (-0.6, 0.2), (0.2, 1.3), (1.1, 1.2), (1.7, -0.5)):
        q.append(np.stack([base, np.full_like(base, dy), np.full_like(base, dz)], 1))
    return _f32(np.concatenate(q))


def hand_cases():
    """name -> (target (N, 3) float32, queries (M, 3) float32)"""
    rng = np.random.default_rng(20260)
    out = {}
    # one row of cells with n points over up to three cells: every batch edge of B = 4 and of the fused kernel's B = 8
    for n in ROW_SIZES:
        xs = np.sort(rng.uniform(0.0, 2.6, n)).astype(np.float32)
        xs[0] = 0.0
        pts = np.stack([xs, rng.uniform(0.0, 0.3, n), rng.uniform(0.0, 0.3, n)], 1)
        out[f"row_{n}"] = (_f32(pts[rng.permutation(n)]), _row_queries(xs))
    # two and three occupied cells in a row, 90 % of the points in the last / in the first cell: the guessed start lies on the
    # far side of the nearest point
    for cells in (2, 3):
        for heavy_last in (False, True):
            n = 40
            few = rng.uniform(0.0, cells - 1.0, n // 10)
            many = rng.uniform(cells - 1.0, float(cells) - 0.02, n - n // 10)
            xs = np.concatenate([few, many])
            if not heavy_last:
                xs = (cells - 0.02) - xs
            xs = np.concatenate([[0.0], xs]).astype(np.float32)
            pts = np.stack([xs, rng.uniform(0.0, 0.3, xs.size), rng.uniform(0.0, 0.3, xs.size)], 1)
            out[f"skew_{cells}_{'last' if heavy_last else 'first'}"] = (_f32(pts[rng.permutation(xs.size)]), _row_queries(np.sort(xs)))
    # equal x throughout (a wall normal to x), every point twice: the order carries no information
    w = np.stack([np.full(150, 1.25), rng.uniform(0.0, 3.0, 150), rng.uniform(0.0, 3.0, 150)], 1)
    wall = np.concatenate([w, w])
    qw = np.stack([rng.uniform(-0.5, 3.0, 400), rng.uniform(-0.5, 3.5, 400), rng.uniform(-0.5, 3.5, 400)], 1)
    out["wall_dup"] = (_f32(wall[rng.permutation(300)]), _f32(np.concatenate([qw, w[:40] + [0.3, 0.0, 0.0], w[:40]])))
    # points whose x differ by less than the quantum (2^-16 m = 1.5e-5), in either stored order: 18 points 3e-6 apart on a
    # line (y, z equal), queries on and between them -- the match distance is of the order of the spacing, so the budget of the
    # exit test is far below the quantum
    k = np.arange(18)
    line = np.stack([0.5 + 3e-6 * k, np.full(18, 0.25), np.full(18, 0.25)], 1)
    far = np.array([[0.0, 0.0, 0.0], [2.5, 0.2, 0.1], [1.5, 0.1, 0.2]])
    pts = _f32(np.concatenate([line[rng.permutation(18)], far]))
    lx = pts[:18, 0].astype(np.float64)
    qs = np.concatenate([lx, lx + 1.4e-6, lx - 1.6e-6, [0.5 - 2e-5, 0.5 + 9e-5]])
    ql = np.stack([qs, np.full(qs.size, 0.25), np.full(qs.size, 0.25)], 1)
    out["sub_quantum"] = (pts, _f32(np.concatenate([ql, ql + [0.0, 1e-6, 0.0]])))
    # two points at exactly the same distance on opposite sides of the query, stored in both index orders, among fillers that
    # put them into different batches: the smaller original index wins from either scan direction
    pair = []
    for y, swap in ((0.25, False), (0.75, True)):
        a, b = [1.0 - 0.25, y, 0.5], [1.0 + 0.25, y, 0.5]
        pair += [b, a] if swap else [a, b]
    fill = np.stack([np.concatenate([rng.uniform(0.0, 0.4, 6), rng.uniform(1.6, 2.5, 6)]), rng.uniform(0.0, 0.9, 12), rng.uniform(0.0, 0.9, 12)], 1)
    fill[0] = 0.0
    out["equidistant"] = (_f32(np.concatenate([fill[:5], pair[:2], fill[5:9], pair[2:], fill[9:]])),
                          _f32([[1.0, 0.25, 0.5], [1.0, 0.75, 0.5], [1.0, 0.5, 0.5], [1.0, 0.25, 0.25], [1.0, 0.75, 0.75]]))
    # a cube of cells: the segment that begins at record 0 (the min-corner cell) and the one that ends at the last record (the
    # max-corner cell), queries at and beyond both corners -- the tail pad and the start of the allocation
    cube = rng.uniform(0.0, 3.0, (60, 3))
    cube[0] = 0.0
    cube[1] = 3.0
    cube[2:6] = rng.uniform(0.0, 0.5, (4, 3))
    cube[6:10] = rng.uniform(2.5, 3.0, (4, 3))
    qc = np.concatenate([rng.uniform(-0.8, 0.8, (40, 3)), rng.uniform(2.3, 3.9, (40, 3)), rng.uniform(-0.5, 3.5, (80, 3))])
    out["corners"] = (_f32(cube), _f32(qc))
    # ring-0 lists (halo 0.1 cell): a query in an EMPTY cell that has a list (the point at x = 0.95 is within the halo of the
    # face x = 1), a query in an occupied cell whose match is a halo copy (x = 2.05: the cell's own point is at 2.9, the
    # neighbour's at 1.97), and the same across y and z faces
    lst = np.array([[0.0, 0.0, 0.0], [0.95, 0.5, 0.5], [1.97, 0.5, 0.5], [2.9, 0.5, 0.5], [2.5, 0.96, 0.5], [2.5, 0.5, 0.97],
                    [3.5, 0.5, 0.5], [3.03, 0.93, 0.94], [0.5, 1.5, 0.5], [0.5, 1.03, 0.5]])
    ql = np.array([[1.2, 0.5, 0.5], [1.03, 0.5, 0.5], [2.05, 0.5, 0.5], [2.02, 0.52, 0.47], [2.5, 1.02, 0.5], [2.5, 0.5, 1.03],
                   [2.97, 0.97, 0.97], [3.02, 0.5, 0.5], [0.5, 0.98, 0.5], [0.5, 0.93, 0.52], [1.5, 0.5, 0.5]])
    out["lists"] = (_f32(lst), _f32(np.concatenate([ql, ql + rng.normal(0, 0.01, ql.shape)])))
    return out


def street_case():
    """A 20 k-point street target with normals-free ICP / PlaneICP inputs and a 2 k-point perturbed scan."""
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=41)
    scan, T_true = perturbed_scan(target, 2_000, seed=42)
    return _f32(target), _f32(street_normals(target)), _f32(scan)


def heavy_case():
    from point_cloud_registration_amd.synthetic import lidar_sweep, lidar_normals, perturbed_scan
    target = lidar_sweep(20_000)
    scan, _ = perturbed_scan(target, 2_000, seed=43)
    return _f32(target), _f32(lidar_normals(target)), _f32(scan)


def _sums_both(capi, ctx, tgt, sc, kind, T):
    """the 29 sums of search + reduce (variant 1: batches of 4) and of the fused kernel (variant 0: batches of 8)"""
    out = []
    for variant in (1, 0):
        with ctx.pipeline(variant=variant, reuse=0):
            out.append(capi.linearize(tgt, sc, kind, T, MAX_DIST).copy())
    return np.stack(out)


def run_all(capi, ctx):
    """Every case through the library -> {name: array}."""
    res = {}
    eye = np.eye(4)
    for name, (pts, q) in hand_cases().items():
        tgt = capi.Target.points(ctx, pts, cell_hint=1.0)
        res[name + "/x_ordered"] = np.array(tgt.index_info()["x_ordered"])
        d, i = tgt.nn_query(q)
        res[name + "/nn_d"], res[name + "/nn_i"] = d, i
        sc = capi.Scan(ctx, q)
        res[name + "/sums"] = _sums_both(capi, ctx, tgt, sc, capi.ICP, eye)
        if name == "lists":
            # the deeper list set: built once the target has served a dozen search + reduce passes, read by a pass over a scan
            # without history (tests/test_gpu_parity.py: test_deeper_list_set_is_exact)
            with ctx.pipeline(variant=1, reuse=0):
                for _ in range(14):
                    capi.linearize(tgt, sc, capi.ICP, eye, MAX_DIST)
                info = tgt.index_info()
                res[name + "/halo2_records"] = np.array(info["halo2_records"])
                fresh = capi.Scan(ctx, q)
                res[name + "/sums_deep"] = np.stack([capi.linearize(tgt, fresh, capi.ICP, eye, MAX_DIST).copy(),
                                                     capi.linearize(tgt, fresh, capi.ICP, eye, MAX_DIST).copy()])
                fresh.close()
        sc.close(); tgt.close()
    for name, (target, normals, scan) in (("street", street_case()), ("heavy", heavy_case())):
        tgt = capi.Target.points(ctx, target, normals)
        res[name + "/x_ordered"] = np.array(tgt.index_info()["x_ordered"])
        res[name + "/heavy"] = np.array(tgt.index_info()["heavy"])
        sc = capi.Scan(ctx, scan)
        T, it, trace = capi.align(tgt, sc, capi.PLANE, eye, 30, 1e-3, MAX_DIST, want_trace=True)
        poses = [trace[k, :16].reshape(4, 4).copy() for k in range(min(it, 5))]
        poses += [np.asarray(T, np.float64).reshape(4, 4).copy()] * (5 - len(poses))      # (a shorter run: the final pose again)
        res[name + "/poses"] = np.stack(poses)
        res[name + "/sums"] = np.stack([_sums_both(capi, ctx, tgt, sc, kind, P) for P in poses for kind in (capi.ICP, capi.PLANE)])
        for k, P in enumerate(poses):
            q = _f32((P[:3, :3] @ scan.astype(np.float64).T).T + P[:3, 3])
            res[f"{name}/nn_q{k}"] = q
            res[f"{name}/nn_d{k}"], res[f"{name}/nn_i{k}"] = tgt.nn_query(q)
        for loop, flag in (("host", capi.FLAG_HOST_LOOP), ("device", capi.FLAG_DEVICE_LOOP)):
            T, it = capi.align(tgt, capi.Scan(ctx, scan), capi.PLANE, eye, 30, 1e-3, MAX_DIST, flags=capi.FLAG_ICP_RR_QUIRK | flag)
            res[f"{name}/align_{loop}"] = np.concatenate([np.asarray(T).reshape(-1), [it]])
        if name == "street":
            with ctx.pipeline(variant=1, reuse=0):
                for _ in range(14):
                    capi.linearize(tgt, sc, capi.PLANE, eye, MAX_DIST)
                res[name + "/halo2_records"] = np.array(tgt.index_info()["halo2_records"])
                fresh = capi.Scan(ctx, scan)
                res[name + "/sums_deep"] = np.stack([capi.linearize(tgt, fresh, capi.PLANE, P, MAX_DIST).copy() for P in poses])
                fresh.close()
        sc.close(); tgt.close()
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from point_cloud_registration_amd import _capi
    np.savez(sys.argv[1], **run_all(_capi, _capi.get_context(0)))
