"""SymmetricICP on the GPU: normals on a scan, their round trip, the sums of one pass, both gates, the sign rule, align, and
the neighbours it must leave undisturbed.

Fixture: g2_mini_street -- 5000 targets, 2000 scan points, gate 0.8, 1823 kept, non-identity T; no distance within 1e-4 of the
gate and no near-ties, so masks and indices compare exactly; nn_idx / nn_dist are the reference's.  Transformed points come
from orc.transform, which is bit-identical to the kernels' xform.  Target normals are the fixture's plane_normals.

Bounds (tests/symm_cases.py restates include/pcr.h in float64 NumPy, with its expression order):
  scan normals  bit for bit against pcr_target_estimate_normals(compat = 0) where the device order is the caller's; under a
                Morton-sorted scan up to sign within 2^-22 per component (float32 storage, margin 8) on the points whose
                eigen-gap (l1 - l0) / l2 > 0.05 -- at least 95 % of them
  sums          per entry (n_kept + 16) 2^-53 sum_i |term_i| against math.fsum of the restated terms; conftest.step_err <= 1e-10
  PlaneICP      where R n_p = +-n_q up to float32 rounding: 2^-20 max|H|, 2^-20 relative on e2, step_err <= 1e-6 against the golden

A neighbourhood of ONE point (a one-point scan; k = 1) has the zero covariance; the kernel returns (1, 0, 0) for it, the
first column of the identity the Jacobi sweeps start from -- a unit vector, never the zero vector."""

import gc as pygc

import numpy as np
import pytest

import dist_cases as dc
import gicp_cases as gc
import symm_cases as sc
from conftest import step_err

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 63, 64, 65, 257)
SYMM_W = 3                                  # points per lane in flight (symm.hip)


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def case():
    target, scan, T_true = gc.align_case()
    for a in (target, scan, T_true):
        a.setflags(write=False)
    return target, scan, T_true


def neighbours(points, k):
    """The GPU's own exact k-NN of every point within its cloud (pinned bit-exact by the k-NN tests); padding = len(points)."""
    import point_cloud_registration_amd as pcr
    return pcr.KDTree(points).query(points, k)[1].reshape(len(points), -1)


def target_normals(capi, ctx, pts, k):
    return capi.Target.points(ctx, pts).estimate_normals(k, compat=False)


# ----------------------------------------------------------------------------- 1. scan normals
@pytest.mark.parametrize("k", [10, 20])
def test_scan_normals(capi, ctx, g2, k):
    src = g2["source"]
    ref = target_normals(capi, ctx, src, k)
    same = capi.Scan(ctx, src, flags=capi.FLAG_NO_SCAN_SORT).estimate_normals(k)
    assert same.dtype == np.float32 and same.shape == (len(src), 3)
    assert np.array_equal(same, ref)
    # Morton-sorted on the device: another index over the same points
    kept = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_normals(k)
    gap = gc.covariance(src, neighbours(src, k), "raw")[2]
    sel = gap > 0.05
    sign = np.where(np.sum(kept.astype(np.float64) * ref, axis=1) < 0, -1.0, 1.0)
    err = np.max(np.abs(kept * sign[:, None] - ref), axis=1)
    print(f"k={k}: compared {sel.mean():.4f}, max err up to sign {err[sel].max():.3e}, signs flipped {np.mean(sign < 0):.3f}")
    assert np.all(np.isfinite(kept)) and sel.mean() >= 0.95
    assert np.all(err[sel] <= 2.0 ** -22)


def test_scan_normals_edge_sizes(capi, ctx, g2):
    for n in SIZES:
        pts = np.ascontiguousarray(g2["target"][:n])
        for flags in (capi.FLAG_KEEP_ORDER, capi.FLAG_NO_SCAN_SORT):
            nrm = capi.Scan(ctx, pts, flags=flags).estimate_normals(10)
            assert nrm.shape == (n, 3) and np.all(np.isfinite(nrm))
            assert np.all(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22), n
            if n == 1:
                assert np.array_equal(nrm, np.float32([[1, 0, 0]]))          # the single-point neighbourhood (see above)
        assert np.array_equal(capi.Scan(ctx, pts, flags=capi.FLAG_NO_SCAN_SORT).estimate_normals(10), target_normals(capi, ctx, pts, 10))
    pts = np.ascontiguousarray(g2["target"][:64])
    # k = 1: every neighbourhood is the point itself
    assert np.array_equal(capi.Scan(ctx, pts, flags=capi.FLAG_KEEP_ORDER).estimate_normals(1), np.tile(np.float32([1, 0, 0]), (64, 1)))
    for k in (0, 65):
        with pytest.raises(ValueError):
            capi.Scan(ctx, pts, flags=capi.FLAG_KEEP_ORDER).estimate_normals(k)
    # estimating without reading back works on any scan, an empty one included
    capi.Scan(ctx, pts).estimate_normals(10, want=False)
    capi.Scan(ctx, pts[:0]).estimate_normals(10, want=False)
    empty = capi.Scan(ctx, pts[:0], flags=capi.FLAG_KEEP_ORDER)
    assert empty.estimate_normals(10).shape == (0, 3)
    empty.set_normals(np.zeros((0, 3), np.float32))
    assert empty.get_normals().shape == (0, 3)


# ----------------------------------------------------------------------------- 2. round trip
def test_normal_round_trip(capi, ctx, g2):
    src = g2["source"]
    N = sc.unit_normals(len(src), seed=1)
    for flags in (capi.FLAG_KEEP_ORDER, capi.FLAG_NO_SCAN_SORT):
        s = capi.Scan(ctx, src, flags=flags)
        with pytest.raises(ValueError):
            s.get_normals()                                   # none yet
        s.set_normals(N)
        assert np.array_equal(s.get_normals(), N)
        bad = N.copy()
        bad[1234, 1] = np.nan
        with pytest.raises(ValueError):
            s.set_normals(bad)
        bad[1234, 1] = np.inf
        with pytest.raises(ValueError):
            s.set_normals(bad)
        assert np.array_equal(s.get_normals(), N)             # a refused set leaves the old ones
        with pytest.raises(ValueError):
            s.set_normals(N[:-1])
    plain = capi.Scan(ctx, src)
    with pytest.raises(ValueError):
        plain.set_normals(N)
    plain.estimate_normals(10, want=False)
    with pytest.raises(ValueError):
        plain.get_normals()
    with pytest.raises(ValueError):
        plain.estimate_normals(10, want=True)


# ----------------------------------------------------------------------------- 3. sums, kernel-only
@pytest.fixture(scope="module")
def normalsets(capi, ctx, g2):
    """Scan normals, so the sums do not depend on test 1: (a) random unit vectors from default_rng(0), (b) the GPU-estimated
    ones read back.  Computed once, never modified."""
    src = g2["source"]
    out = {"random": sc.unit_normals(len(src)),
           "estimated": capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_normals(10)}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def restated(g2, orc, normalsets):
    """(name, min_cos) -> (terms (N, 28), keep, c): the definition at g2's pose from the GOLDEN correspondences."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    tp = orc.transform(T, src)
    nq = g2["plane_normals"][g2["nn_idx"]]
    out = {}
    for name, n_p in normalsets.items():
        for min_cos in (0.0, 0.5, 1.0):
            t = sc.terms(T, src, tp, tgt[g2["nn_idx"]], n_p, nq, mask, min_cos)
            t.setflags(write=False)
            out[name, min_cos] = (t, sc.kept(T, n_p, nq, mask, min_cos), sc.dots(T, n_p, nq))
    return out


def reference(restated, name, n=None, min_cos=0.0):
    t, keep, _ = restated[name, min_cos]
    n = len(keep) if n is None else n
    return sc.reference(t[:n], keep[:n])


def gpu_sums(capi, ctx, g2, n_p, n=None, flags=None, max_dist=None, min_cos=0.0, nq=None):
    n = len(n_p) if n is None else n
    t = capi.Target.points(ctx, g2["target"])
    t.set_normals(g2["plane_normals"] if nq is None else nq)
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    s.set_normals(np.ascontiguousarray(n_p[:n]))
    md = float(g2["max_dist"]) if max_dist is None else max_dist
    return capi.symm_linearize(t, s, g2["T"], md, min_cos), t, s


@pytest.mark.parametrize("name", ["random", "estimated"])
def test_sums(capi, ctx, g2, normalsets, restated, name):
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    c = restated[name, 0.0][2]
    print(f"{name}: min|c| over the kept points {np.min(np.abs(c[mask])):.3e}, c < 0 on {np.mean(c[mask] < 0):.3f}")
    assert np.min(np.abs(c[mask])) > 1e-6                     # no sign decision within rounding of zero
    out, t, s = gpu_sums(capi, ctx, g2, normalsets[name])
    ref, bound, kept = reference(restated, name)
    assert kept == 1823 and out[28] == kept
    err = np.abs(out[:28] - ref)
    print(f"{name}: max err / bound {np.max(err / bound):.3e}, bound / max|H| {bound[:21].max() / np.abs(ref[:21]).max():.3e}")
    assert np.all(err <= bound)
    H, g, _ = sc.unpack28(out[:28])
    Href, gref, _ = sc.unpack28(ref)
    se = step_err(H, g, Href, gref)
    print(f"{name}: step error {se:.3e}")
    assert se <= 1e-10
    # two consecutive calls return the same bits
    assert np.array_equal(out, capi.symm_linearize(t, s, g2["T"], float(g2["max_dist"]), 0.0))
    # the scan in the caller's order on the device
    nosort = gpu_sums(capi, ctx, g2, normalsets[name], flags=capi.FLAG_NO_SCAN_SORT)[0]
    assert nosort[28] == kept and np.all(np.abs(nosort[:28] - ref) <= bound) and np.all(np.abs(nosort[:28] - out[:28]) <= bound)


# ----------------------------------------------------------------------------- 4. prefixes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_sums_prefixes(capi, ctx, g2, normalsets, restated, n):
    """Correspondences of a subset of the scan are a subset of g2's."""
    for name in ("random", "estimated"):
        out = gpu_sums(capi, ctx, g2, normalsets[name], n=n)[0]
        ref, bound, kept = reference(restated, name, n)
        assert out[28] == kept
        assert np.all(np.abs(out[:28] - ref) <= bound)
        if n == 0:
            assert np.array_equal(out, np.zeros(29))


# ----------------------------------------------------------------------------- 5. more than one trip of the grid
def test_grid_rule_on_this_device(cus):
    """The sizes below make slots and trips live only while the reduce grid is 8 blocks per CU."""
    assert dc.stride_points(cus) == 524288, cus


@pytest.mark.parametrize("order", ["keep_order", "no_scan_sort"])
@pytest.mark.parametrize("k", range(SYMM_W))
def test_live_slots(capi, ctx, cus, g2, normalsets, restated, k, order):
    """Sizes stride + 257, 2 stride + 257, 3 stride + 513: slot 1, slot 2, then the second trip carry live points."""
    n = dc.big_sizes(cus, SYMM_W)[k]
    t, keep, _ = restated["random", 0.0]
    ref, bound, count = sc.tiled(t, keep, n)
    tgt = capi.Target.points(ctx, g2["target"])
    tgt.set_normals(g2["plane_normals"])
    s = capi.Scan(ctx, dc.tile_rows(g2["source"], n), flags=capi.FLAG_KEEP_ORDER if order == "keep_order" else capi.FLAG_NO_SCAN_SORT)
    try:
        s.set_normals(dc.tile_rows(normalsets["random"], n))
        out = capi.symm_linearize(tgt, s, g2["T"], float(g2["max_dist"]), 0.0)
        err = np.abs(out[:28] - ref)
        print(f"n {n} {order}: kept {count}, max err / bound {np.max(err / bound):.3e}")
        assert out[28] == count and 0 < count < n
        assert np.all(err <= bound)
        H, g, _ = sc.unpack28(out[:28])
        Href, gref, _ = sc.unpack28(ref)
        assert step_err(H, g, Href, gref) <= 1e-10
        assert np.array_equal(capi.symm_linearize(tgt, s, g2["T"], float(g2["max_dist"]), 0.0), out)
    finally:
        s.close()


# ----------------------------------------------------------------------------- 6. sign invariance, bit for bit
def test_sign_invariance(capi, ctx, g2, normalsets):
    n_p, nq = normalsets["random"], g2["plane_normals"]
    out = gpu_sums(capi, ctx, g2, n_p)[0]
    rng = np.random.default_rng(7)
    flip_p = rng.random(len(n_p)) < 0.5
    flip_q = rng.random(len(nq)) < 0.5
    assert 0.4 < flip_p.mean() < 0.6 and 0.4 < flip_q.mean() < 0.6
    assert np.array_equal(gpu_sums(capi, ctx, g2, np.where(flip_p[:, None], -n_p, n_p))[0], out)
    assert np.array_equal(gpu_sums(capi, ctx, g2, n_p, nq=np.where(flip_q[:, None], -nq, nq))[0], out)
    assert np.array_equal(gpu_sums(capi, ctx, g2, -n_p, nq=-nq)[0], out)


# ----------------------------------------------------------------------------- 7. normal gate
def test_normal_gate(capi, ctx, g2, normalsets, restated):
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    c = restated["random", 0.0][2]
    assert np.min(np.abs(np.abs(c[mask]) - 0.5)) > 1e-9       # nothing within rounding of the gate
    out = gpu_sums(capi, ctx, g2, normalsets["random"], min_cos=0.5)[0]
    ref, bound, kept = reference(restated, "random", min_cos=0.5)
    assert kept == 912 and out[28] == kept
    assert np.all(np.abs(out[:28] - ref) <= bound)
    assert np.array_equal(gpu_sums(capi, ctx, g2, normalsets["random"], min_cos=1.0)[0], np.zeros(29))
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            gpu_sums(capi, ctx, g2, normalsets["random"], min_cos=bad)


def test_refusals(capi, ctx, g2, normalsets):
    T, md = g2["T"], float(g2["max_dist"])
    s = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER)
    bare = capi.Target.points(ctx, g2["target"])
    with pytest.raises(ValueError, match="scan has no normals"):
        capi.symm_linearize(gpu_sums(capi, ctx, g2, normalsets["random"])[1], s, T, md)
    s.set_normals(normalsets["random"])
    with pytest.raises(ValueError, match="target has no normals"):
        capi.symm_linearize(bare, s, T, md)
    vox = capi.Target.voxels(ctx, g2["target"].astype(np.float64), float(g2["voxel_size"]))
    with pytest.raises(ValueError, match="point target"):
        capi.symm_linearize(vox, s, T, md)
    with pytest.raises(ValueError):
        capi.symm_align(bare, s, T, 5, 1e-3, md)


# ----------------------------------------------------------------------------- 8. distance gate
def test_nothing_inside_the_gate(capi, ctx, g2, normalsets):
    import point_cloud_registration_amd as pcr
    assert np.array_equal(gpu_sums(capi, ctx, g2, normalsets["random"], max_dist=1e-6)[0], np.zeros(29))
    reg = pcr.SymmetricICP(max_dist=1e-6)
    reg.set_target(g2["target"], norm=g2["plane_normals"])
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(g2["source"], init_T=g2["T"], source_normals=normalsets["random"])


def test_gate(case, orc):
    """T = I, max_dist = 0.1: 45.2 % kept, none within 1e-3 relative of the gate: the count equals the restated mask."""
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.SymmetricICP(max_dist=0.1, k=10)
    reg.set_target(target)
    dist = reg.kdtree.query(orc.transform(np.eye(4), scan))[0]
    assert np.min(np.abs(dist / np.float32(0.1) - 1.0)) > 1e-3
    kept = int((dist < np.float32(0.1)).sum())
    assert abs(kept / len(scan) - 0.452) < 0.005, kept / len(scan)
    reg.calc_H_g_e2(np.eye(4), scan)
    assert reg.last_correspondences == kept


# ----------------------------------------------------------------------------- 9. the PlaneICP property
def test_plane_icp_where_the_normals_agree(g2, restated):
    import point_cloud_registration_amd as pcr
    T, src = g2["T"], g2["source"]
    n_p, nq = sc.plane_case(g2)
    reg = pcr.SymmetricICP(max_dist=float(g2["max_dist"]))
    reg.set_target(g2["target"], norm=nq)
    assert np.array_equal(reg.normal, nq)
    H, g, e2 = reg.calc_H_g_e2(T, src, source_normals=n_p)
    assert reg.last_correspondences == 1823
    assert np.array_equal(reg.source_normals(src), n_p)
    eH = np.max(np.abs(H - g2["T_plane_H"])) / np.max(np.abs(g2["T_plane_H"]))
    ee = abs(e2 - float(g2["T_plane_e2"])) / float(g2["T_plane_e2"])
    se = step_err(H, g, g2["T_plane_H"], g2["T_plane_g"])
    print(f"max|dH| / max|H| {eH:.3e}, |de2| / e2 {ee:.3e}, step error {se:.3e}")
    assert eH <= 2.0 ** -20 and ee <= 2.0 ** -20 and se <= 1e-6
    # the per-point host loop over the GPU's correspondences, within the sum bound of the kernel's result
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    t = sc.terms(T, src, sc.xform32(T, src), g2["target"][g2["nn_idx"]], n_p, nq[g2["nn_idx"]], mask)
    ref, bound, kept = sc.reference(t, sc.kept(T, n_p, nq[g2["nn_idx"]], mask))
    kernel = np.concatenate([H[sc.TRIU], g, [e2]])
    assert kept == 1823 and np.all(np.abs(kernel - ref) <= bound)
    Hl, gl, e2l = reg.calc_H_g_e2_no_parallel_ver(T, src, source_normals=n_p)
    assert np.all(np.abs(np.concatenate([Hl[sc.TRIU], gl, [e2l]]) - kernel) <= bound)


# ----------------------------------------------------------------------------- 10. align
@pytest.mark.parametrize("max_dist", [2.0, 0.15])
def test_align(capi, case, max_dist):
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.math_tools import plus
    target, scan, T_true = case
    reg = pcr.SymmetricICP(max_dist=max_dist, k=10)
    reg.set_target(target)
    T = reg.align(scan)
    iters = reg.last_iterations
    dR, dt = np.linalg.norm(T[:3, :3] - T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])
    print(f"max_dist {max_dist}: {iters} iterations, |dR|_F {dR:.3e}, |dt| {dt:.3e}")
    assert dR < 1e-3 and dt < 1e-3
    # the same loop in the test: calc_H_g_e2 + solve + plus
    cur, it = np.eye(4), 0
    for it in range(reg.max_iter):
        H, g, _ = reg.calc_H_g_e2(cur, scan)
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < reg.tol:
            break
        cur = plus(cur, dx)
    assert iters == it + 1
    assert np.max(np.abs(T - cur)) <= 1e-10
    # the Python loop of the class
    slow = pcr.SymmetricICP(max_dist=max_dist, k=10, native_loop=False)
    slow.set_target(target)
    assert np.max(np.abs(slow.align(scan) - T)) <= 1e-10 and slow.last_iterations == iters
    # every trace row's sums are the bits pcr_symm_linearize returns at that row's pose
    dev = reg._symm_scan(scan, None)
    T2, iters2, trace = capi.symm_align(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, max_dist, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(capi.symm_linearize(reg._target, dev, row[:16], max_dist), row[16:])
    # max_iter = 0 returns init_T
    T0 = plus(np.eye(4), np.array([0.01, 0.02, 0.03, 0.001, 0.002, 0.003]))
    reg0 = pcr.SymmetricICP(max_dist=max_dist, k=10, max_iter=0)
    reg0.set_target(target)
    assert np.array_equal(reg0.align(scan, init_T=T0), T0) and reg0.last_iterations == 0


# ----------------------------------------------------------------------------- 11. neighbours undisturbed
def test_neighbours_undisturbed(capi, ctx, g2):
    """ICP / PlaneICP / GICP return the same bits before and after a symmetric pass: over one context and the same scan array,
    and over the very same device scan -- one that carries covariances AND normals."""
    import point_cloud_registration_amd as pcr
    T, src, tgt, md = g2["T"], g2["source"], g2["target"], float(g2["max_dist"])
    icp, plane, gicp, symm = pcr.ICP(max_dist=md), pcr.PlaneICP(max_dist=md), pcr.GICP(max_dist=md), pcr.SymmetricICP(max_dist=md)
    icp.set_target(tgt)
    plane.set_target(tgt, kdree=object(), norm=g2["plane_normals"])
    gicp.set_target(tgt)
    symm.set_target(tgt, norm=g2["plane_normals"])
    for variant in (2, 1):
        with ctx.pipeline(variant=variant):
            before = [reg.calc_H_g_e2(T, src) for reg in (icp, plane, gicp)]
            first = symm.calc_H_g_e2(T, src)
            after = [reg.calc_H_g_e2(T, src) for reg in (icp, plane, gicp)]
            for b, a in zip(before, after):
                assert all(np.array_equal(x, y) for x, y in zip(b, a))
            assert all(np.array_equal(x, y) for x, y in zip(first, symm.calc_H_g_e2(T, src)))
            s = capi.Scan(ctx, src)
            s.estimate_covariances(10, want=False)
            s.estimate_normals(10, want=False)
            o1 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g1 = capi.gicp_linearize(gicp._target, s, T, md)
            s1 = capi.symm_linearize(symm._target, s, T, md)
            o2 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g2_ = capi.gicp_linearize(gicp._target, s, T, md)
            s2 = capi.symm_linearize(symm._target, s, T, md)
            assert np.array_equal(o1, o2) and np.array_equal(g1, g2_) and np.array_equal(s1, s2)
            assert g1[28] == o1[28] == s1[28] == 1823


# ----------------------------------------------------------------------------- 12. the call's parameter decides
def test_min_cos_belongs_to_the_call(capi, ctx, g2):
    """Three calls over ONE uploaded scan, min_cos = 0, 0.9, 0: the first and the third return the same bits, the second keeps
    strictly fewer pairs -- the gate is a parameter of the call, nothing an earlier call leaves on the scan.  The counts are
    the restatement's (symm_cases.kept over brute-force correspondences), no |c| within 1e-9 of the gate."""
    tgt, nq, src, _, j, mask = sc.call_case(g2)
    n_p = sc.unit_normals(len(src), seed=3)
    T, md = g2["T"], sc.CALL_MAX_DIST
    assert np.min(np.abs(np.abs(sc.dots(T, n_p, nq[j])[mask]) - 0.9)) > 1e-9
    all_, few = (int(sc.kept(T, n_p, nq[j], mask, mc).sum()) for mc in (0.0, 0.9))
    assert (all_, few) == (216, 21)
    t = capi.Target.points(ctx, tgt)
    t.set_normals(nq)
    s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    s.set_normals(n_p)
    first, second, third = (capi.symm_linearize(t, s, T, md, mc) for mc in (0.0, 0.9, 0.0))
    assert np.array_equal(first, third)
    assert first[28] == all_ and second[28] == few < first[28]


# ----------------------------------------------------------------------------- 13. device memory
def test_align_device_memory_is_stable(capi, ctx, case):
    import torch
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.SymmetricICP(max_dist=2.0, k=10)
    reg.set_target(target)
    first = reg.align(scan); pygc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        last = reg.align(scan)
    pygc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
    assert np.array_equal(first, last)
