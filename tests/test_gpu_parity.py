"""Parity of the HIP hot path (through the C ABI) against the CPU oracle and the golden vectors.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
Tolerances (BASELINE.json north_star): J^T J within 1e-5 relative (max|dH|/max|H|) and SE(3)
within 1e-4 rad / 1e-4 m of the REFERENCE; against the ORACLE (same arithmetic definitions,
only the summation order differs) the bar is 1e-10.  Correspondence indices are bit-exact.
"""

import numpy as np
import pytest

from conftest import rel_H

pytestmark = pytest.mark.gpu

TOL_REF = 1e-5
TOL_ORC = 1e-10
NAMES = ["icp", "plane", "vplane", "ndt"]


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


def kind_of(capi, name):
    return {"icp": capi.ICP, "plane": capi.PLANE, "vplane": capi.VPLANE, "ndt": capi.NDT}[name]


def make_targets(capi, orc, ctx, target, normals, voxel_size):
    """GPU targets + matching oracle targets.  Voxel statistics come from the oracle here so the
    test isolates the per-iteration kernels; the GPU voxel build has its own tests."""
    o_pts = orc.TargetPoints(target, normals=normals)
    o_vox = orc.TargetVoxels(target, voxel_size)
    g_pts = capi.Target.points(ctx, np.asarray(target, np.float32), normals)
    g_vox = capi.Target.voxels_from_stats(ctx, o_vox.mean, o_vox.norm, o_vox.icov, voxel_size)
    return ({"icp": g_pts, "plane": g_pts, "vplane": g_vox, "ndt": g_vox},
            {"icp": o_pts, "plane": o_pts, "vplane": o_vox, "ndt": o_vox})


def check_against(capi, orc, gt, ot, name, T, src, max_dist, scan=None, tol=TOL_ORC):
    scan = scan or capi.Scan(gt[name].ctx, src)
    out = capi.linearize(gt[name], scan, kind_of(capi, name), T, max_dist)
    H, g, e2, cnt = capi.unpack29(out)
    Ho, go, e2o, cnto = orc.calc_H_g_e2(kind_of(capi, name), ot[name], T, src, max_dist, with_count=True)
    assert cnt == cnto
    assert rel_H(H, Ho) < tol, (name, rel_H(H, Ho))
    assert rel_H(g, go) < tol * 100, (name, rel_H(g, go))       # g cancels: looser relative bar
    assert abs(e2 - e2o) <= tol * max(abs(e2o), 1e-30) * 10
    return H, g, e2


# ----------------------------------------------------------------------------- NN seam
def test_nn_query_bit_exact_small(capi, orc, ctx, g2):
    st = orc.transform(g2["T"], g2["source"])
    tgt = capi.Target.points(ctx, g2["target"])
    d, i = tgt.nn_query(st)
    do, io = orc.nn_brute(g2["target"], st)
    assert np.array_equal(i, io)
    assert np.array_equal(d, do)
    # bounded: beyond r_max -> -1 / inf (scipy's distance_upper_bound convention)
    d, i = tgt.nn_query(st, r_max=0.8)
    keep = do < 0.8
    assert np.array_equal(i[keep], io[keep]) and np.all(i[~keep] == -1) and np.all(np.isinf(d[~keep]))
    # golden (reference KD-tree) agreement up to float32 rounding of the transform
    assert (i[keep] == g2["nn_idx"][keep]).mean() > 0.999


@pytest.mark.parametrize("cell", [0.0, 0.05, 0.3, 2.0])
def test_nn_query_random_clouds(capi, orc, ctx, cell):
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-3, 3, (20000, 3)).astype(np.float32)
    tgt[:500] = tgt[500:1000]                       # exact duplicates -> exact ties, smaller index wins
    q = np.vstack([rng.uniform(-3.5, 3.5, (3000, 3)), rng.uniform(-30, 30, (200, 3)),
                   tgt[:300].astype(np.float64)]).astype(np.float32)
    t = capi.Target.points(ctx, tgt, cell_hint=cell)
    d, i = t.nn_query(q)
    do, io = orc.nn_brute(tgt, q)
    assert np.array_equal(i, io)
    assert np.array_equal(d, do)


def test_nn_query_centroids_f64(capi, orc, ctx, g2):
    vox = orc.TargetVoxels(g2["target"], float(g2["voxel_size"]))
    t = capi.Target.voxels_from_stats(ctx, vox.mean, vox.norm, vox.icov, float(g2["voxel_size"]))
    st = orc.transform(g2["T"], g2["source"])
    d, i = t.nn_query(st)
    do, io = orc.nn_brute_f64(vox.mean, st)
    assert np.array_equal(i, io) and np.array_equal(d, do)


def test_nn_degenerate_targets(capi, orc, ctx):
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    t = capi.Target.points(ctx, one)
    q = np.array([[0, 0, 0], [1, 2, 3], [100, -50, 7]], np.float32)
    d, i = t.nn_query(q)
    do, io = orc.nn_brute(one, q)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    flat = np.zeros((100, 3), np.float32)           # all points identical: zero-extent bounding box
    t = capi.Target.points(ctx, flat)
    d, i = t.nn_query(q)
    assert np.all(i == 0)


# ----------------------------------------------------------------------------- hot path
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag", ["I", "T"])
def test_linearize_reference_fixture(capi, orc, ctx, g1, name, tag):
    gt, ot = make_targets(capi, orc, ctx, g1["target"], g1["plane_normals"], float(g1["voxel_size"]))
    T = np.eye(4) if tag == "I" else g1["T"]
    H, g, e2 = check_against(capi, orc, gt, ot, name, T, g1["source"], float(g1["max_dist"]))
    assert rel_H(H, g1[f"{tag}_{name}_H"]) < TOL_REF
    assert rel_H(g, g1[f"{tag}_{name}_g"]) < TOL_REF
    assert abs(e2 - g1[f"{tag}_{name}_e2"]) < TOL_REF * max(1.0, abs(g1[f"{tag}_{name}_e2"]))


def test_shipped_pipeline_is_the_default(capi, ctx):
    """What the library selects on its own is what bench.py times: the per-launch choice between
    k_nn_scan + k_reduce_finalize (large scans) and k_linearize_finalize (small scans)."""
    from conftest import PIPELINES
    assert ctx.get_pipeline() == PIPELINES["default"]
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(300_000, seed=1)
    tgt = capi.Target.points(ctx, target)
    for n_scan, want in ((20_000, "linearize"), (300_000, "nn")):
        scan, _ = perturbed_scan(target, n_scan if n_scan < 300_000 else None, seed=3)
        sc = capi.Scan(ctx, scan)
        ctx.profile_enable(True); ctx.profile_reset()
        capi.linearize(tgt, sc, capi.ICP, np.eye(4), 2.0)
        prof = ctx.profile_read(); ctx.profile_enable(False)
        assert prof[want][0] == 1 and prof["finalize"][0] == 0, (n_scan, prof)


@pytest.mark.parametrize("name", NAMES)
def test_linearize_masked_multivoxel(capi, orc, ctx, g2, name, pipeline):
    gt, ot = make_targets(capi, orc, ctx, g2["target"], g2["plane_normals"], float(g2["voxel_size"]))
    scan = capi.Scan(ctx, g2["source"])
    H, g, e2 = check_against(capi, orc, gt, ot, name, g2["T"], g2["source"], float(g2["max_dist"]), scan=scan)
    # further passes over the same scan handle at other poses (the "reuse" pipelines certify / re-search the
    # previous pass' matches instead of searching afresh): still exactly the oracle's sums
    T2 = np.array(g2["T"]); T2[:3, 3] += [0.05, -0.03, 0.02]
    check_against(capi, orc, gt, ot, name, T2, g2["source"], float(g2["max_dist"]), scan=scan)
    check_against(capi, orc, gt, ot, name, np.eye(4), g2["source"], float(g2["max_dist"]), scan=scan)
    assert rel_H(H, g2[f"T_{name}_H"]) < TOL_REF
    assert rel_H(g, g2[f"T_{name}_g"]) < 5 * TOL_REF
    assert abs(e2 - g2[f"T_{name}_e2"]) < 5 * TOL_REF * abs(g2[f"T_{name}_e2"])


def test_icp_quirk_flag(capi, orc, ctx, g1):
    gt, ot = make_targets(capi, orc, ctx, g1["target"], g1["plane_normals"], 1.0)
    scan = capi.Scan(ctx, g1["source"])
    q = capi.unpack29(capi.linearize(gt["icp"], scan, capi.ICP, g1["T"], 2.0, capi.FLAG_ICP_RR_QUIRK))
    c = capi.unpack29(capi.linearize(gt["icp"], scan, capi.ICP, g1["T"], 2.0, 0))
    assert rel_H(q[1], g1["T_icp_g"]) < TOL_REF
    _, gc, _ = orc.calc_H_g_e2(orc.ICP, ot["icp"], g1["T"], g1["source"], 2.0, flags=0)
    assert rel_H(c[1], gc) < 1e-9
    assert np.max(np.abs(q[1][3:] - c[1][3:])) > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_linearize_street_200k(capi, orc, ctx, name, pipeline):
    """Mid-size: 200 k-point street target, 60 k scan, oracle via its exact grid search."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(200_000, seed=3)
    scan, T_true = perturbed_scan(target, 60_000, seed=4)
    rng = np.random.default_rng(0)
    normals = rng.normal(size=target.shape).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    gt, ot = make_targets(capi, orc, ctx, target, normals, 1.0)
    T = np.eye(4); T[:3, 3] = [0.02, -0.01, 0.03]
    sc = capi.Scan(gt[name].ctx, scan)                                     # one handle: passes see each other's matches
    check_against(capi, orc, gt, ot, name, T, scan, 2.0, scan=sc, tol=1e-9)
    check_against(capi, orc, gt, ot, name, T_true, scan, 0.25, scan=sc, tol=1e-9)   # tight gate: many masked
    check_against(capi, orc, gt, ot, name, np.eye(4), scan, 2.0, scan=sc, tol=1e-9)


def test_scan_order_independence(capi, ctx, g2):
    """Morton sorting the scan only permutes the summation order."""
    tgt = capi.Target.points(ctx, g2["target"], g2["plane_normals"])
    a = capi.linearize(tgt, capi.Scan(ctx, g2["source"]), capi.PLANE, g2["T"], 0.8)
    b = capi.linearize(tgt, capi.Scan(ctx, g2["source"], flags=capi.FLAG_NO_SCAN_SORT), capi.PLANE, g2["T"], 0.8)
    perm = np.random.default_rng(1).permutation(g2["source"].shape[0])
    c = capi.linearize(tgt, capi.Scan(ctx, g2["source"][perm]), capi.PLANE, g2["T"], 0.8)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12) and np.allclose(a, c, rtol=1e-12, atol=1e-12)
    assert a[28] == b[28] == c[28]
    # determinism: same inputs, same bits
    assert np.array_equal(a, capi.linearize(tgt, capi.Scan(ctx, g2["source"]), capi.PLANE, g2["T"], 0.8))


# ----------------------------------------------------------------------------- classes / align
def _classes(g, **kw):
    import point_cloud_registration_amd as pcr
    md, vs, k = float(g["max_dist"]), float(g["voxel_size"]), int(g["k"])
    return {"icp": pcr.ICP(max_dist=md, **kw), "plane": pcr.PlaneICP(max_dist=md, k=k, **kw),
            "vplane": pcr.VPlaneICP(voxel_size=vs, max_dist=md, **kw), "ndt": pcr.NDT(voxel_size=vs, max_dist=md, **kw)}


def _pose_close(T, ref, tol=1e-4):
    dR = T[:3, :3] @ ref[:3, :3].T
    ang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    return np.max(np.abs(T[:3, 3] - ref[:3, 3])) < tol and ang < tol


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("loop", ["python", "device", "hostloop"])
def test_align_matches_reference(capi, g2, name, loop, pipeline):
    """Reference-style usage: cls(...).set_target(target); align(scan) -> SE(3) within 1e-4 of the
    reference's own result, same number of Gauss-Newton iterations.  Three drivers of the same loop:
    Python (one calc_H_g_e2 per iteration), the device-resident loop behind pcr_align (default), and
    pcr_align's host-driven form."""
    kw = {"native_loop": loop != "python"}
    if loop == "hostloop":
        kw["compat_flags"] = capi.FLAG_ICP_RR_QUIRK | capi.FLAG_HOST_LOOP
    if loop == "device":
        kw["compat_flags"] = capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP     # (small scans default to the host-driven form)
    obj = _classes(g2, **kw)[name]
    with pytest.raises(ValueError):
        obj.align(g2["source"])                           # target not set (registration.py:80-81)
    if name == "plane":
        obj.set_target(g2["target"], None, None)
        # normals estimated on the GPU: the reference's, up to float32 rounding of an ill-conditioned few
        dots = np.abs(np.sum(obj.normal * g2["plane_normals"], axis=1))
        assert np.mean(dots > 0.999) > 0.995
        T_own = obj.align(g2["source"], np.eye(4))                      # end to end with the GPU's own normals
        assert _pose_close(T_own, g2["align_plane_final"])
        obj.set_target(g2["target"], obj.kdtree, g2["plane_normals"])   # then the reference's normals
    else:
        obj.set_target(g2["target"])
    assert obj.is_target_set()
    T = obj.align(g2["source"], np.eye(4))
    assert obj.last_iterations == g2[f"align_{name}_T"].shape[0]
    assert _pose_close(T, g2[f"align_{name}_final"])
    H, g, e2 = obj.calc_H_g_e2(g2["T"], g2["source"])
    assert rel_H(H, g2[f"T_{name}_H"]) < TOL_REF


def test_align_loop_edge_cases(capi, orc, ctx, g2):
    """pcr_align's device-resident loop against its host-driven form: max_iter 0 / 1 / exhausted, a tolerance
    met at the first pass (quirk Q4: the step is discarded), the trace rows, every kind."""
    gt, ot = make_targets(capi, orc, ctx, g2["target"], g2["plane_normals"], float(g2["voxel_size"]))
    md = float(g2["max_dist"])
    scan = capi.Scan(ctx, g2["source"])
    T0 = np.array(g2["T"])
    for name in NAMES:
        kind = kind_of(capi, name)
        for max_iter, tol in ((0, 1e-3), (1, 1e-3), (2, 1e-3), (3, 1e9), (30, 1e-3)):
            Td, itd, trd = capi.align(gt[name], scan, kind, T0, max_iter, tol, md,
                                      capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP, want_trace=True)
            Th, ith, trh = capi.align(gt[name], scan, kind, T0, max_iter, tol, md,
                                      capi.FLAG_ICP_RR_QUIRK | capi.FLAG_HOST_LOOP, want_trace=True)
            assert itd == ith and np.array_equal(Td, Th) and np.array_equal(trd, trh), (name, max_iter, tol)
            if max_iter == 0:
                assert itd == 0 and np.array_equal(Td, T0)
            if tol == 1e9:
                assert itd == 1 and np.array_equal(Td, T0)          # converged at once: pose untouched
            if max_iter in (1, 2):
                assert itd == max_iter
        # the trace's first row is the pass at T0: the oracle's sums
        Ho, go, e2o, cnto = orc.calc_H_g_e2(kind, ot[name], T0, g2["source"], md, with_count=True)
        Hg, gg, e2g, cntg = capi.unpack29(trd[0, 16:])
        assert cntg == cnto and rel_H(Hg, Ho) < TOL_ORC and np.array_equal(trd[0, :16].reshape(4, 4), T0)


def test_no_device_memory_growth(capi, ctx, g2):
    """Targets, scans, voxel builds, k-NN queries created and destroyed in a loop: the per-context cache of
    temporaries is bounded and nothing leaks."""
    import torch
    import point_cloud_registration_amd as pcr

    def cycle():
        for cls, kw in ((pcr.ICP, {}), (pcr.PlaneICP, {"k": 8}), (pcr.VPlaneICP, {}), (pcr.NDT, {})):
            m = cls(max_dist=float(g2["max_dist"]), **kw)
            m.set_target(g2["target"]); m.align(g2["source"]); m.calc_H_g_e2(np.eye(4), g2["source"])
        tree = pcr.KDTree(g2["target"]); tree.query(g2["source"][:100]); tree.query(g2["source"][:50], k=5)
        pcr.voxel_filter(g2["target"], 0.5)

    import gc
    cycle(); gc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(10):
        cycle()
    gc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20


def test_zero_correspondences_is_singular(g2):
    """Quirk Q7: nothing passes the gate -> H = 0 -> numpy.linalg.LinAlgError."""
    import point_cloud_registration_amd as pcr
    far = (g2["source"] + np.float32(500.0)).astype(np.float32)
    for native in (False, True):
        icp = pcr.ICP(max_dist=0.5, native_loop=native)
        icp.set_target(g2["target"])
        H, g, e2 = icp.calc_H_g_e2(np.eye(4), far)
        assert not H.any() and not g.any() and e2 == 0
        with pytest.raises(np.linalg.LinAlgError):
            icp.align(far)
    empty = np.zeros((0, 3), np.float32)
    H, g, e2 = icp.calc_H_g_e2(np.eye(4), empty)
    assert not H.any()


def test_calc_H_g_e2_is_pure_in_its_inputs(capi, orc, g2):
    """The scan cache of calc_H_g_e2 is keyed on the CONTENT of the array: an in-place edit of a single
    point (one the old sampled fingerprint would have missed) is seen, an unchanged array is not
    uploaded again (calc_H_g_e2 is pure w.r.t. its inputs)."""
    import point_cloud_registration_amd as pcr
    icp = pcr.ICP(max_dist=float(g2["max_dist"]))
    icp.set_target(g2["target"])
    src = np.array(g2["source"], dtype=np.float32)
    H0, g0, e0 = icp.calc_H_g_e2(g2["T"], src)
    scan0 = icp._scan
    H1, g1, e1 = icp.calc_H_g_e2(g2["T"], src)
    assert icp._scan is scan0 and np.array_equal(H0, H1)               # same content: device copy reused
    src[1] += np.float32(0.25)                                          # in place, same object, same buffer
    H2, g2_, e2 = icp.calc_H_g_e2(g2["T"], src)
    assert icp._scan is not scan0                                       # re-uploaded
    ot = orc.TargetPoints(g2["target"])
    Ho, go, e2o = orc.calc_H_g_e2(orc.ICP, ot, g2["T"], src, float(g2["max_dist"]))
    assert rel_H(H2, Ho) < TOL_ORC and abs(e2 - e2o) <= 1e-9 * abs(e2o) and abs(e2 - e0) > 1e-6
    src[1] -= np.float32(0.25)
    H3, _, _ = icp.calc_H_g_e2(g2["T"], src)
    assert np.array_equal(H3, H0)


def test_non_finite_target_is_refused(capi, ctx, g2):
    """NaN / inf rows (common in raw PCD files) in a TARGET are an error, not a silent grid blow-up;
    in a SCAN they are simply gated out (test_robustness_edge_inputs)."""
    import point_cloud_registration_amd as pcr
    bad = np.array(g2["target"], dtype=np.float32)
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        capi.Target.points(ctx, bad)
    bad[7, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        pcr.ICP().set_target(bad)
    with pytest.raises(ValueError, match="non-finite"):
        pcr.NDT(voxel_size=1.0).set_target(bad)
    # one far (finite) outlier only coarsens the grid: still exact
    far = np.array(g2["target"], dtype=np.float32)
    far[3] = [9000.0, -7000.0, 400.0]
    t = capi.Target.points(ctx, far)
    d, i = t.nn_query(g2["source"][:500])
    from oracle import oracle as orc
    do, io = orc.nn_brute(far, g2["source"][:500])
    assert np.array_equal(i, io) and np.array_equal(d, do)


def test_planeicp_does_not_touch_a_shared_tree(capi, g2):
    """PlaneICP.set_target(target, tree, normals) keeps its normals in its own index: the caller's tree
    (possibly shared with other registrations) is neither searched nor modified."""
    import point_cloud_registration_amd as pcr
    tree = pcr.KDTree(g2["target"])
    a = pcr.PlaneICP(max_dist=float(g2["max_dist"]), k=int(g2["k"]))
    b = pcr.PlaneICP(max_dist=float(g2["max_dist"]), k=int(g2["k"]))
    a.set_target(g2["target"], tree, g2["plane_normals"])
    flipped = -np.asarray(g2["plane_normals"])[:, [1, 0, 2]]
    b.set_target(g2["target"], tree, flipped)
    Ha, _, _ = a.calc_H_g_e2(g2["T"], g2["source"])
    assert rel_H(Ha, g2["T_plane_H"]) < TOL_REF                          # a still uses ITS normals
    assert a.kdtree is not tree and b.kdtree is not tree and a.kdtree is not b.kdtree
    with pytest.raises(ValueError):
        tree._target.get_normals()                                       # the shared tree never received normals


def test_kdtree_seam(capi, orc, g2):
    import point_cloud_registration_amd as pcr
    tree = pcr.KDTree(g2["target"])
    st = orc.transform(g2["T"], g2["source"])
    d, i = tree.query(st)
    do, io = orc.nn_brute(g2["target"], st)
    assert d.dtype == np.float32 and np.array_equal(i, io) and np.array_equal(d, do)
    d5, i5 = tree.query(st[:500], k=5)
    dk, ik = orc.knn_brute(g2["target"], st[:500], 5)
    assert d5.shape == (500, 5) and np.array_equal(i5, ik) and np.array_equal(d5, dk)


def test_profile_counters(capi, ctx, g2, pipeline):
    """HIP-event launch accounting of each pipeline (no separate fold kernel in the shipped ones)."""
    tgt = capi.Target.points(ctx, g2["target"], g2["plane_normals"])
    scan = capi.Scan(ctx, g2["source"])
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(5):
        capi.linearize(tgt, scan, capi.PLANE, g2["T"], 0.8)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    want = {"default": dict(nn=0, reduce=0, finalize=0, linearize=5),          # a 2 k-point scan: the fused kernel
            "split": dict(nn=5, reduce=5, finalize=0, linearize=0),
            "reuse_auto": dict(nn=5, reduce=5, finalize=0, linearize=0),
            "reuse": dict(nn=5, reduce=5, finalize=0, linearize=0, certify=3),     # full, tracking, 3 x certify + list
            "noreuse": dict(nn=5, reduce=5, finalize=0, linearize=0, certify=0),
            "coop": dict(nn=5, reduce=5, finalize=0, linearize=0),
            "mfma": dict(nn=5, reduce=5, finalize=0, linearize=0),
            "nofilter": dict(nn=5, reduce=5, finalize=0, linearize=0),
            "unfused": dict(nn=5, reduce=5, finalize=5, linearize=0, certify=3),
            "onekernel": dict(nn=0, reduce=0, finalize=0, linearize=5),
            "onekernel_unfused": dict(nn=0, reduce=0, finalize=5, linearize=5)}[pipeline]
    assert {k: prof[k][0] for k in want} == want
    assert all(prof[k][1] > 0 for k, v in want.items() if v)


@pytest.mark.parametrize("name", NAMES)
def test_rccl_single_rank(capi, orc, ctx, g2, name, pipeline):
    """The RCCL exchange step (in-stream ncclAllReduce of the 29 doubles + k_publish hand-off, and
    k_gn_update inside pcr_align) with a 1-rank communicator, every kind, every pipeline: same sums and
    the same Gauss-Newton run as without a communicator; PCR_FLAG_LOCAL_ONLY skips the collective."""
    gt, _ = make_targets(capi, orc, ctx, g2["target"], g2["plane_normals"], float(g2["voxel_size"]))
    kind, md = kind_of(capi, name), float(g2["max_dist"])
    scan = capi.Scan(ctx, g2["source"])
    a = capi.linearize(gt[name], scan, kind, g2["T"], md)
    Ta, ia, tra = capi.align(gt[name], scan, kind, np.eye(4), 30, 1e-3, md, want_trace=True)
    ctx.comm_init(capi.comm_unique_id(), 1, 0)
    try:
        ctx.profile_enable(True); ctx.profile_reset()
        b = capi.linearize(gt[name], scan, kind, g2["T"], md)
        assert ctx.profile_read()["allreduce"][0] == 1
        ctx.profile_reset()
        c = capi.linearize(gt[name], scan, kind, g2["T"], md, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_LOCAL_ONLY)
        assert ctx.profile_read()["allreduce"][0] == 0          # per-call decision: no collective issued
        ctx.profile_enable(False)
        Tb, ib, trb = capi.align(gt[name], scan, kind, np.eye(4), 30, 1e-3, md, want_trace=True)
    finally:
        ctx.profile_enable(False)
        ctx.comm_destroy()
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert ia == ib == g2[f"align_{name}_T"].shape[0]
    assert np.array_equal(Ta, Tb) and np.array_equal(tra, trb)


# ----------------------------------------------------------------------------- set_target side
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("vs", [0.5, 1.0])
def test_voxel_build_gpu(capi, orc, ctx, g3, dt, vs):
    """VoxelGrid.set_points + calc_icov on the GPU vs the reference's own numbers."""
    tag = f"{dt}_vs{vs}"
    pts = g3[f"points_{dt}"]
    t = capi.Target.voxels(ctx, pts, vs, 10)
    st = t.voxel_stats()
    counts = g3[f"{tag}_counts"]
    keep = counts >= 10
    assert np.array_equal(st["keys"], g3[f"{tag}_uniq"][keep])          # integer work: bit-exact
    assert np.array_equal(st["counts"], counts[keep])
    assert np.allclose(st["mean"], g3[f"{tag}_mean"], rtol=0, atol=1e-12)
    assert np.allclose(st["cov"], g3[f"{tag}_cov"], rtol=1e-10, atol=1e-15)
    assert np.allclose(st["icov"], g3[f"{tag}_icov"], rtol=1e-7, atol=0)
    ev = g3[f"{tag}_evals"]
    ok = (ev[:, 1] - ev[:, 0]) > 1e-3 * ev[:, 2]
    dots = np.abs(np.sum(st["norm"] * g3[f"{tag}_norm"], axis=1))
    assert np.all(dots[ok] > 1 - 1e-8)
    # and bit-level agreement with the oracle's restatement of the same sums
    o = orc.voxel_build(pts, vs, 10)
    assert np.array_equal(st["mean"], o["mean"]) and np.array_equal(st["cov"], o["cov"])
    assert np.allclose(st["icov"], orc.calc_icov(o["cov"]), rtol=1e-13, atol=0)


def test_voxel_build_edge_cases(capi, ctx):
    rng = np.random.default_rng(2)
    # negative coordinates, voxels below min_points dropped, one huge voxel
    pts = np.vstack([rng.uniform(-5, 5, (3000, 3)), rng.uniform(0.1, 0.9, (5000, 3)) + [-3, -2, -4]]).astype(np.float32)
    t = capi.Target.voxels(ctx, pts, 1.0, 10)
    st = t.voxel_stats(("counts", "keys", "mean"))
    from point_cloud_registration_amd.voxel import get_keys
    keys = get_keys(pts, 1.0)
    u, c = np.unique(keys, return_counts=True)
    assert np.array_equal(st["keys"], u[c >= 10]) and np.array_equal(st["counts"], c[c >= 10])
    assert st["counts"].max() >= 5000
    # nothing survives the filter -> empty target, zero correspondences
    t0 = capi.Target.voxels(ctx, pts[:50], 0.01, 10)
    assert t0.size() == 0
    out = capi.linearize(t0, capi.Scan(ctx, pts[:100]), capi.VPLANE, np.eye(4), 2.0)
    assert not out.any()


def _compat_cov(pts, nbr):
    """The float32 covariance of estimate_normals.py:56-72 in ITS order (running float32 sums over the neighbours,
    nearest first; cov = E[pp^T] - mu mu^T in float32), as a float64 3x3 matrix."""
    f = np.float32
    s = [f(0)] * 3
    xx = [f(0)] * 6
    for j in nbr:
        x, y, z = (f(v) for v in pts[j])
        s = [s[0] + x, s[1] + y, s[2] + z]
        xx = [xx[0] + x * x, xx[1] + x * y, xx[2] + x * z, xx[3] + y * y, xx[4] + y * z, xx[5] + z * z]
    kf = f(len(nbr))
    m = [v / kf for v in s]
    c = [xx[0] / kf - m[0] * m[0], xx[1] / kf - m[0] * m[1], xx[2] / kf - m[0] * m[2],
         xx[3] / kf - m[1] * m[1], xx[4] / kf - m[1] * m[2], xx[5] / kf - m[2] * m[2]]
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], dtype=np.float64)


def _assert_smallest_eigvec(pts, knn_idx, normals, rows, what):
    """Every normal in `rows` minimises n^T C n over unit vectors up to the solver's precision, C = the float32 covariance
    of its exact neighbours: where the two smallest eigenvalues (nearly) coincide the DIRECTION is not defined -- those are
    the points the |dot| statistics leave out -- but the quotient still is."""
    for r in rows:
        C = _compat_cov(pts, knn_idx[r])
        lam = np.linalg.eigvalsh(C)
        n = normals[r].astype(np.float64)
        q = float(n @ C @ n) / float(n @ n)
        assert q <= lam[0] + 1e-5 * max(abs(lam[0]), abs(lam[2])) + 1e-12, (what, int(r), q, lam)


@pytest.mark.parametrize("k", [5, 15])
def test_knn_and_normals_gpu(capi, orc, ctx, g6, k):
    pts = g6["points"]
    t = capi.Target.points(ctx, pts)
    d, i = t.knn_query(pts, k)
    do, io = orc.knn_brute(pts, pts, k)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    n_gpu = t.estimate_normals(k, compat=True)
    n_orc = orc.normals_from_knn(pts, io, compat=True)
    dots = np.abs(np.sum(n_gpu.astype(np.float64) * n_orc, axis=1))
    assert np.mean(dots > 1 - 1e-6) >= 0.999            # same float32 covariance, same eigen-solver
    dref = np.abs(np.sum(n_gpu * g6[f"normals_k{k}"], axis=1))
    assert np.mean(dref > 0.999) >= 0.999               # vs the reference (float32 LAPACK eigh)
    # the points those two statistics leave out (+ a few hundred of the others): a valid smallest eigenvector all the same
    odd = np.nonzero((dots <= 1 - 1e-6) | (dref <= 0.999))[0]
    _assert_smallest_eigvec(pts, io, n_gpu, np.concatenate([odd, np.arange(0, len(pts), max(len(pts) // 300, 1))]), f"k={k}")
    n64 = t.estimate_normals(k, compat=False)
    d64 = np.abs(np.sum(n64.astype(np.float64) * orc.normals_from_knn(pts, io, compat=False), axis=1))
    assert np.mean(d64 > 1 - 1e-6) >= 0.999
    assert np.allclose(np.linalg.norm(n_gpu, axis=1), 1, atol=1e-5)


@pytest.mark.parametrize("k", [5, 15])
def test_normals_full_scale_gpu(capi, orc, ctx, g7, k):
    """N2 at B-01 scale (1.06 M points, |p| up to 67 m): GPU normals vs the oracle (same arithmetic)
    and vs the REFERENCE's own normals of 20 000 sampled points, far corners included."""
    pts, sample = g7["points"], g7["sample"]
    t = capi.Target.points(ctx, pts)
    n_gpu = t.estimate_normals(k, compat=True)
    dref = np.abs(np.sum(n_gpu[sample].astype(np.float64) * g7[f"normals_k{k}"], axis=1))
    assert np.mean(dref > 0.999) >= 0.999, np.mean(dref > 0.999)
    far = np.argsort(-np.linalg.norm(pts[sample], axis=1))[:1000]
    pick = np.unique(np.concatenate([np.arange(3000), far]))
    dk, ik = t.knn_query(pts[sample[pick]], k)
    n_orc = orc.normals_from_knn(pts, ik, compat=True)
    dorc = np.abs(np.sum(n_gpu[sample[pick]].astype(np.float64) * n_orc, axis=1))
    assert np.mean(dorc > 1 - 1e-6) >= 0.999, np.mean(dorc > 1 - 1e-6)
    dpick = np.abs(np.sum(n_gpu[sample[pick]].astype(np.float64) * g7[f"normals_k{k}"][pick], axis=1))
    odd = np.nonzero((dorc <= 1 - 1e-6) | (dpick <= 0.999))[0]
    _assert_smallest_eigvec(pts, ik, n_gpu[sample[pick]], np.concatenate([odd, np.arange(0, len(pick), 20)]), f"full scale k={k}")
    # and the k-NN itself against brute force on a few hundred of them
    _, ib = orc.knn_brute(pts, pts[sample[pick[:300]]], k)
    assert np.array_equal(ik[:300], ib)


def test_voxel_filter_gpu(g3, g12):
    """voxel_filter (voxel.py:209-241) against the REFERENCE's own output on g3's cloud (tests/golden/make_golden.py: g12;
    VERDICT r5 weak #4): one float32 centroid per occupied voxel, ascending key order, bit for bit (the reference sums with
    float64 bincount weights and rounds once, like the GPU build)."""
    import point_cloud_registration_amd as pcr
    pts = g3["points_f32"]
    for vs in (0.5, 1.0):
        f = pcr.voxel_filter(pts, vs)
        assert f.dtype == np.float32 and np.array_equal(f, g12[f"filter_vs{vs}"]), vs


def test_centroid_tree_knn_matches_reference(g3, g12):
    """VoxelGrid.kdtree.query(points, k) for k > 1 (voxel.py:165: KDTree(means) answers any k; VERDICT r5 missing #5): the
    reference's three nearest centroids and their float64 distances for 500 query points."""
    import point_cloud_registration_amd as pcr
    grid = pcr.VoxelGrid(1.0)
    grid.set_points(g3["points_f32"])
    d, i = grid.kdtree.query(g12["k3_query"], k=3)
    assert np.array_equal(i, g12["k3_idx"])
    assert np.allclose(d, g12["k3_dist"], rtol=1e-12, atol=1e-12)
    d1, i1 = grid.kdtree.query(g12["k3_query"])
    assert np.array_equal(i1, g12["k1_idx"]) and np.allclose(d1, g12["k1_dist"], rtol=1e-12, atol=1e-12)


def test_robustness_edge_inputs(capi, orc, ctx):
    """NaN / inf scan points are gated out, far-away scans give zero sums, huge coordinates and
    duplicated points keep the search exact, collinear voxels hit the det == 0 -> 1e6 rule."""
    rng = np.random.default_rng(9)
    tgt_pts = rng.uniform(-4, 4, (5000, 3)).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (5000, 1))
    tgt = capi.Target.points(ctx, tgt_pts, nrm)
    scan = rng.uniform(-4, 4, (1000, 3)).astype(np.float32)
    clean = capi.linearize(tgt, capi.Scan(ctx, scan), capi.PLANE, np.eye(4), 1.0)
    dirty = scan.copy(); dirty[::10] = np.nan; dirty[5::10, 1] = np.inf
    keep = np.isfinite(dirty).all(1)
    got = capi.linearize(tgt, capi.Scan(ctx, dirty), capi.PLANE, np.eye(4), 1.0)
    want = capi.linearize(tgt, capi.Scan(ctx, scan[keep]), capi.PLANE, np.eye(4), 1.0)
    assert got[28] == want[28] and np.allclose(got, want, rtol=1e-12, atol=1e-12) and got[28] < clean[28]
    # large offsets (|p| ~ 1e4 m): float32 spacing 1e-3 m, the search must still be exact
    big = (tgt_pts.astype(np.float64) * 50 + [12000.0, -9000.0, 300.0]).astype(np.float32)
    q = (big[:800].astype(np.float64) + rng.normal(0, 0.5, (800, 3))).astype(np.float32)
    t2 = capi.Target.points(ctx, big)
    d, i = t2.nn_query(q)
    do, io = orc.nn_brute(big, q)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    # every point duplicated 3x: ties everywhere, smallest index wins
    dup = np.repeat(tgt_pts[:500], 3, axis=0)
    t3 = capi.Target.points(ctx, dup)
    d, i = t3.nn_query(scan)
    do, io = orc.nn_brute(dup, scan)
    assert np.array_equal(i, io) and np.all(i % 3 == 0)
    # collinear voxel: singular covariance -> icov = adjugate / 1e6 (voxel.py:88), no NaN
    line = np.zeros((40, 3)); line[:, 0] = np.linspace(0.05, 0.95, 40)
    tv = capi.Target.voxels(ctx, line, 1.0, 10)
    st = tv.voxel_stats(("cov", "icov", "norm"))
    assert tv.size() == 1 and np.isfinite(st["icov"]).all() and np.isfinite(st["norm"]).all()
    assert np.allclose(st["icov"], orc.calc_icov(st["cov"]), rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- remaining API surface
def test_device_pointer_entry_points(capi, ctx, g2):
    """pcr_target_points_create_device / pcr_scan_create_device with device memory owned by the
    caller (a torch tensor): same sums as the host-pointer path, and torch shares our HIP runtime."""
    import torch
    assert torch.cuda.is_available()
    tgt_host = capi.Target.points(ctx, g2["target"], g2["plane_normals"])
    a = capi.linearize(tgt_host, capi.Scan(ctx, g2["source"]), capi.PLANE, g2["T"], 0.8)
    d_t = torch.from_numpy(np.ascontiguousarray(g2["target"], np.float32)).cuda()
    d_n = torch.from_numpy(np.ascontiguousarray(g2["plane_normals"], np.float32)).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(g2["source"], np.float32)).cuda()
    torch.cuda.synchronize()
    tgt_dev = capi.Target.points_device(ctx, d_t.data_ptr(), d_t.shape[0], d_n.data_ptr())
    scan_dev = capi.Scan(ctx, device_ptr=d_s.data_ptr(), n=d_s.shape[0])
    b = capi.linearize(tgt_dev, scan_dev, capi.PLANE, g2["T"], 0.8)
    assert np.array_equal(a, b)
    import os
    maps = open(f"/proc/{os.getpid()}/maps").read()
    assert len({l.split()[-1] for l in maps.splitlines() if "libamdhip64" in l}) == 1     # one runtime


def test_class_level_helpers(capi, orc, g2, g6, capsys):
    import point_cloud_registration_amd as pcr
    # VoxelGrid.query: nearest kept voxel's statistics + 'dist' (voxel.py:171-179)
    vg = pcr.VoxelGrid(float(g2["voxel_size"]))
    vg.set_points(g2["target"])
    vg.calc_icov()
    st = orc.transform(g2["T"], g2["source"])
    q = vg.query(st, ["mean", "norm", "icov"])
    ov = orc.TargetVoxels(g2["target"], float(g2["voxel_size"]))
    do, io = orc.nn_brute_f64(ov.mean, st)
    assert np.array_equal(q["dist"], do) and np.array_equal(q["mean"], ov.mean[io])
    assert np.allclose(q["icov"], ov.icov[io], rtol=1e-12, atol=0) and q["norm"].shape == (len(st), 3)
    vg.calc_sqrt_icov()
    assert vg.sqrt_icov.shape == vg.icov.shape
    # KDTree.query with an upper bound; estimate_normals at top level
    tree = pcr.KDTree(g2["target"])
    d, i = tree.query(st, distance_upper_bound=0.5)
    dn, inn = orc.nn_brute(g2["target"], st)
    far = ~(dn < 0.5)
    assert np.all(i[far] == -1) and np.all(np.isinf(d[far])) and np.array_equal(i[~far], inn[~far])
    n = pcr.estimate_normals(g6["points"], k=15)
    assert n.shape == g6["points"].shape and n.dtype == np.float32
    assert np.mean(np.abs(np.sum(n * g6["normals_k15"], axis=1)) > 0.999) >= 0.999
    # verbose align prints the reference's line format (registration.py:91-92)
    icp = pcr.ICP(max_dist=float(g2["max_dist"]))
    icp.set_target(g2["target"])
    icp.align(g2["source"], np.eye(4), verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("iter 0, error ") and len(out) == icp.last_iterations


@pytest.fixture(params=["0", "0.05", "0.1", "0.3", "0.45", "0.7", "1.0"])
def halo(request, monkeypatch):
    """PCR_HALO (margin of the extended per-cell lists as a fraction of the cell edge; 0.1 ships, 0 = none):
    read when a point target is built."""
    monkeypatch.setenv("PCR_HALO", request.param)
    return float(request.param)


@pytest.mark.parametrize("name", ["icp", "plane"])
def test_tile_handout_covers_every_point_once(capi, orc, ctx, name):
    """The search hands its tiles out in 1024-point chunks dealt round-robin to the XCDs (round 5: nn_tile_loop's chunk
    interleave; block-local below ~3 M points).  Scan sizes on and around every boundary of that scheme -- one tile, one chunk,
    one round of eight chunks, partial last tiles and chunks, a size that leaves whole XCDs without work -- must give every
    point exactly one match: the correspondence count and the sums of the search + reduce pipeline against the oracle and
    against the one-kernel pipeline, whose loop does not use the hand-out."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    kind = {"icp": capi.ICP, "plane": capi.PLANE}[name]
    okind = {"icp": orc.ICP, "plane": orc.PLANE}[name]
    target = street(60_000, seed=3)
    full, _ = perturbed_scan(target, 40_000, seed=4)
    tgt = capi.Target.points(ctx, target)
    normals = tgt.estimate_normals(10, compat=True)
    ot = orc.TargetPoints(target, normals=normals)
    T = np.eye(4); T[:3, 3] = [0.03, -0.02, 0.05]
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2047, 8191, 8192, 8193, 9000, 16383, 16385, 24577, 33000):
        scan = full[:n]
        with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=0):
            out = capi.linearize(tgt, capi.Scan(ctx, scan), kind, T, 1.0)
        with ctx.pipeline(variant=0, fuse_finalize=1, nn_mode=0, reuse=0):
            one = capi.linearize(tgt, capi.Scan(ctx, scan), kind, T, 1.0)
        H, g, e2, cnt = capi.unpack29(out)
        Ho, go, e2o, cnto = orc.calc_H_g_e2(okind, ot, T, scan, 1.0, with_count=True)
        assert cnt == cnto == int(round(one[28])), (name, n, cnt, cnto)
        assert np.allclose(out, one, rtol=1e-11, atol=1e-9 * max(np.max(np.abs(one)), 1e-30)), (name, n)
        assert rel_H(H, Ho) < 1e-9 or cnto == 0, (name, n)


def test_nn_stress_cell_boundaries(capi, orc, ctx, halo):
    """Exactness where the pruning bounds are tightest (and where the halo lists decide what ring 0 certifies): points and queries ON cell boundaries (lattice
    coordinates that are exact multiples of the cell size), clustered / planar / collinear clouds,
    cell sizes from much smaller to much larger than the point spacing, bounded and unbounded."""
    rng = np.random.default_rng(123)
    for trial in range(12):
        kind = trial % 4
        n = int(rng.integers(200, 4000))
        if kind == 0:                                       # integer lattice, heavy ties
            tgt = rng.integers(-8, 9, (n, 3)).astype(np.float32) * np.float32(0.25)
        elif kind == 1:                                     # thin plane + clusters
            tgt = rng.normal(0, 1, (n, 3)).astype(np.float32); tgt[:, 2] *= np.float32(0.01)
            tgt[: n // 4] = tgt[: n // 4] * np.float32(0.05) + np.float32([3, 3, 0])
        elif kind == 2:                                     # a line along an axis-diagonal
            s = rng.uniform(-5, 5, n).astype(np.float32); tgt = np.stack([s, s, -s], 1)
        else:                                               # uniform volume with a far outlier
            tgt = rng.uniform(-2, 2, (n, 3)).astype(np.float32); tgt[0] = [40, -35, 20]
        cell = float(rng.choice([0.03, 0.1, 0.25, 0.5, 1.0, 4.0]))
        q = np.vstack([rng.uniform(-6, 6, (600, 3)),
                       rng.integers(-10, 11, (300, 3)) * cell,            # queries exactly on cell faces / corners
                       tgt[rng.integers(0, n, 200)].astype(np.float64)]).astype(np.float32)
        t = capi.Target.points(ctx, tgt, cell_hint=cell)
        d, i = t.nn_query(q)
        do, io = orc.nn_brute(tgt, q)
        assert np.array_equal(i, io), (trial, kind, cell)
        assert np.array_equal(d, do), (trial, kind, cell)
        r = float(rng.choice([0.2, 1.0, 3.0]))
        db, ib = t.nn_query(q, r_max=r)
        keep = do < r
        assert np.array_equal(ib[keep], io[keep]) and np.all(ib[~keep] == -1), (trial, kind, cell, r)
        dk, ik = t.knn_query(q[:200], 7)
        dko, iko = orc.knn_brute(tgt, q[:200], 7)
        assert np.array_equal(ik, iko) and np.array_equal(dk, dko), (trial, kind, cell)
        t.close()


# ----------------------------------------------------------------------------- randomised differential test
def _fuzz_cloud(rng, n):
    """One of several point-cloud families; float32, arbitrary scale and offset."""
    fam = int(rng.integers(0, 5))
    if fam == 0:                                   # uniform box
        p = rng.uniform(-1, 1, (n, 3))
    elif fam == 1:                                 # a few noisy planar sheets (LiDAR-like)
        p = rng.uniform(-1, 1, (n, 3))
        sheet = rng.integers(0, 3, n)
        for a in range(3):
            m = sheet == a
            p[m, a] = rng.choice([-0.7, 0.1, 0.6]) + rng.normal(0, 0.002, int(m.sum()))
    elif fam == 2:                                 # tight clusters and empty space between them
        centres = rng.uniform(-1, 1, (max(n // 200, 1), 3))
        p = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.01, (n, 3))
    elif fam == 3:                                 # lattice: exact distance ties everywhere
        side = max(int(np.ceil(n ** (1 / 3) - 1e-9)), 1)
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        p = g / max(side, 1) * 2 - 1
    else:                                          # duplicates of a small set
        base = rng.uniform(-1, 1, (max(n // 4, 1), 3))
        p = base[rng.integers(0, len(base), n)]
    scale = 10.0 ** rng.uniform(-1.5, 2.5)
    offset = rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-1, 3.5)
    return (p * scale + offset).astype(np.float32), scale


@pytest.mark.parametrize("seed", range(32))
def test_fuzz_against_oracle(capi, orc, ctx, seed):
    """Random cloud family / size / scale / offset / pose / gate / kind / kernel pipeline: correspondences
    bit-exact against brute force, the 29 sums against the oracle."""
    from conftest import PIPELINES, DEV_PIPELINES
    from point_cloud_registration_amd.math_tools import makeT, expSO3
    rng = np.random.default_rng(1000 + seed)
    n_t = int(rng.choice([1, 2, 17, 300, 4000, 30000]))
    n_s = int(rng.choice([1, 5, 64, 65, 1000, 9000]))
    target, scale = _fuzz_cloud(rng, n_t)
    n_t = target.shape[0]
    pick = target[rng.integers(0, n_t, n_s)].astype(np.float64)
    source = (pick + rng.normal(0, 0.02 * scale, (n_s, 3)) * rng.choice([0.0, 1.0, 10.0])).astype(np.float32)
    T = makeT(expSO3(rng.normal(0, 0.02, 3)), rng.normal(0, 0.02 * scale, 3))
    max_dist = float(rng.choice([np.inf, 2.0, 0.05 * scale, 1e-4 * scale, 10.0 * scale]))
    # correspondences: exact, index and distance
    st = orc.transform(T, source)
    tgt = capi.Target.points(ctx, target)
    d, i = tgt.nn_query(st)
    do, io = orc.nn_brute(target, st)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    # the pass, every kind that this cloud supports, on a random kernel pipeline
    name = list(PIPELINES)[int(rng.integers(0, len(PIPELINES)))]
    if name in DEV_PIPELINES and not capi.has_dev_kernels():
        # (the developer pipelines run where the developer kernels are: tests/test_gpu_dev_build.py re-runs this test in a
        # process that loaded libpcr_hip_dev.so; the shipped library takes the shipped counterpart)
        name = {"coop": "split", "mfma": "split", "unfused": "reuse", "onekernel_unfused": "onekernel"}[name]
    normals = rng.normal(size=target.shape).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    o_pts = orc.TargetPoints(target, normals=normals)
    g_pts = capi.Target.points(ctx, target, normals)
    sc = capi.Scan(ctx, source)
    with ctx.pipeline(**PIPELINES[name]):
        for kind in (capi.ICP, capi.PLANE):
            out = capi.linearize(g_pts, sc, kind, T, max_dist)
            H, g, e2, cnt = capi.unpack29(out)
            Ho, go, e2o, cnto = orc.calc_H_g_e2(kind, o_pts, T, source, max_dist, with_count=True)
            assert cnt == cnto, (name, kind, cnt, cnto)
            if cnto:
                assert rel_H(H, Ho) < 1e-9, (name, kind, rel_H(H, Ho))
                assert np.max(np.abs(g - go)) <= 1e-9 * max(np.max(np.abs(H)), np.max(np.abs(go)), 1e-300), (name, kind)
                assert abs(e2 - e2o) <= 1e-9 * max(abs(e2o), 1e-300)
            else:
                assert not np.any(out[:28])
        # voxel kinds (statistics from the oracle, as in make_targets): nearest CENTROID in float64
        vs = float(scale * rng.choice([0.2, 0.5, 1.0]))
        o_vox = orc.TargetVoxels(target, vs)
        if n_t >= 300 and o_vox.mean.shape[0] > 0:
            g_vox = capi.Target.voxels_from_stats(ctx, o_vox.mean, o_vox.norm, o_vox.icov, vs)
            dv, iv = g_vox.nn_query(st)
            dvo, ivo = orc.nn_brute_f64(o_vox.mean, st)
            assert np.array_equal(iv, ivo) and np.array_equal(dv, dvo)
            for kind in (capi.VPLANE, capi.NDT):
                out = capi.linearize(g_vox, sc, kind, T, max_dist)
                H, g, e2, cnt = capi.unpack29(out)
                Ho, go, e2o, cnto = orc.calc_H_g_e2(kind, o_vox, T, source, max_dist, with_count=True)
                assert cnt == cnto, (name, kind, cnt, cnto)
                if cnto:
                    assert rel_H(H, Ho) < 1e-9, (name, kind, rel_H(H, Ho))
                    assert np.max(np.abs(g - go)) <= 1e-9 * max(np.max(np.abs(H)), np.max(np.abs(go)), 1e-300), (name, kind)
                    assert abs(e2 - e2o) <= 1e-9 * max(abs(e2o), 1e-300)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_voxel_build(capi, orc, ctx, seed):
    """GPU voxel build (keys, counts, means, covariances, inverse covariances) against the oracle's restatement
    of voxel.py:12-21,69-165 on random cloud families, scales, offsets, voxel sizes and input dtypes."""
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.choice([30, 500, 5000, 40000]))
    pts, scale = _fuzz_cloud(rng, n)
    if rng.integers(0, 2):
        pts = pts.astype(np.float64) + rng.normal(0, 1e-7 * scale, pts.shape)      # float64 input with digits float32 lacks
    vs = float(scale * rng.choice([0.05, 0.2, 1.0, 3.0]))
    min_points = int(rng.choice([1, 10, 10, 25]))
    t = capi.Target.voxels(ctx, pts, vs, min_points)
    o = orc.voxel_build(pts, vs, min_points)
    assert t.size() == o["mean"].shape[0]
    if t.size() == 0:
        return
    st = t.voxel_stats()
    assert np.array_equal(st["keys"], o["keys"]) and np.array_equal(st["counts"], o["counts"])
    assert np.array_equal(st["mean"], o["mean"]) and np.array_equal(st["cov"], o["cov"])
    assert np.allclose(st["icov"], orc.calc_icov(o["cov"]), rtol=1e-13, atol=0)


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_align_against_oracle_loop(capi, orc, ctx, seed):
    """pcr_align (device-resident loop) against the reference's loop (registration.py:89-111) driven by the
    ORACLE's calc_H_g_e2 on random LiDAR-like clouds: same number of iterations, same pose."""
    from point_cloud_registration_amd.math_tools import makeT, expSO3, plus
    from point_cloud_registration_amd.synthetic import street
    rng = np.random.default_rng(3000 + seed)
    target = street(int(rng.choice([20_000, 60_000])), seed=100 + seed)
    target = (target * float(rng.choice([1.0, 0.3, 3.0])) + rng.uniform(-50, 50, 3)).astype(np.float32)
    extent = float(np.max(target.max(0) - target.min(0)))
    T_true = makeT(expSO3(rng.normal(0, 0.01, 3)), rng.normal(0, 0.002 * extent, 3))
    idx = rng.choice(target.shape[0], 5000, replace=False)
    Ri, ti = T_true[:3, :3].T, -T_true[:3, :3].T @ T_true[:3, 3]
    source = ((Ri @ target[idx].astype(np.float64).T).T + ti + rng.normal(0, 1e-4 * extent, (5000, 3))).astype(np.float32)
    max_dist = 0.05 * extent
    normals = rng.normal(size=target.shape).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    vs = 0.02 * extent
    gt, ot = make_targets(capi, orc, ctx, target, normals, vs)
    name = NAMES[seed % 4]
    kind = kind_of(capi, name)
    max_iter, tol = 25, 1e-3
    T = np.eye(4)
    iters = 0
    margin = np.inf                                    # how close any |dx| came to the tolerance
    for it in range(max_iter):
        H, g, e2 = orc.calc_H_g_e2(kind, ot[name], T, source, max_dist)
        dx = -np.linalg.solve(H, g)
        iters = it + 1
        margin = min(margin, abs(np.linalg.norm(dx) - tol))
        if np.linalg.norm(dx) < tol:
            break
        T = plus(T, dx)
    assert iters >= 2                                  # the pose really had to move
    sc = capi.Scan(ctx, source)
    Tg, itg = capi.align(gt[name], sc, kind, np.eye(4), max_iter, tol, max_dist)
    if margin > 1e-6:                                  # a step that lands ON the tolerance may fall either way
        assert itg == iters, (name, itg, iters)
        assert np.max(np.abs(Tg - T)) < 1e-7 * max(extent, 1.0), (name, np.max(np.abs(Tg - T)))


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_knn(capi, orc, ctx, seed):
    """Exact k-NN (estimate_normals.py:27-45's tree query) on random cloud families / scales / offsets, k from 1
    to 20, clouds with fewer points than k included: distances AND indices bit-exact against brute force (ties
    in distance are ordered by the smaller index on both sides)."""
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.choice([3, 40, 700, 6000]))
    pts, scale = _fuzz_cloud(rng, n)
    n = pts.shape[0]
    k = int(rng.choice([1, 2, 5, 15, 20]))
    q = np.vstack([pts[rng.integers(0, n, 200)], (pts[rng.integers(0, n, 100)].astype(np.float64)
                                                  + rng.normal(0, 0.05 * scale, (100, 3))).astype(np.float32)])
    t = capi.Target.points(ctx, pts)
    d, i = t.knn_query(q, k)
    do, io = orc.knn_brute(pts, q, k)
    assert np.array_equal(d, do)
    assert np.array_equal(i, io)


CONSTRUCTED_CLOUDS = ["lattice", "dense_spot", "duplicates", "sheet", "two_scales"]


def constructed_cloud(case):
    """-> (cloud, queries) of one constructed case (test_knn_constructed_cases; tests/test_gpu_knn_range.py).  Queries in
    three groups: 300 points of the cloud, 150 next to it, 50 far outside the grid."""
    rng = np.random.default_rng(7)
    if case == "lattice":
        a = np.arange(12, dtype=np.float32) * np.float32(0.25)
        pts = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
        pts = pts[rng.permutation(len(pts))]
    elif case == "dense_spot":
        pts = np.vstack([rng.normal(0, 0.004, (5000, 3)) + [1.0, 2.0, 0.5], rng.uniform(-5, 5, (2500, 3))]).astype(np.float32)
    elif case == "duplicates":
        base = rng.uniform(-2, 2, (1500, 3)).astype(np.float32)
        pts = np.vstack([base, base, base[:700]])[rng.permutation(3700)]
    elif case == "sheet":
        pts = np.hstack([rng.uniform(-4, 4, (6000, 2)), np.zeros((6000, 1))]).astype(np.float32)
    else:
        pts = np.vstack([rng.uniform(-1, 1, (6000, 3)), rng.uniform(-40, 40, (1500, 3))]).astype(np.float32)
    q = np.vstack([pts[rng.integers(0, len(pts), 300)],
                   (pts[rng.integers(0, len(pts), 150)].astype(np.float64) + rng.normal(0, 0.1, (150, 3))).astype(np.float32),
                   (rng.uniform(-1, 1, (50, 3)) * 300).astype(np.float32)])
    return pts, q


@pytest.mark.parametrize("case", CONSTRUCTED_CLOUDS)
@pytest.mark.parametrize("k", [1, 15, 16, 17])
def test_knn_constructed_cases(capi, orc, ctx, case, k):
    """The k <= 16 search's branches on clouds built to take them (knn_normals.hip: knn_collect): exact ties by the
    hundred (a lattice: order by original index), more points than the queue holds inside the first distance class
    (a dense spot: handed to the list search), repeated points (distance 0 several times), a flat sheet, a cloud
    with two densities (sparse part: no bound from the 27-cell block), queries outside the grid -- and the same
    clouds through the k > 16 list.  Distances and indices bit-exact against brute force."""
    pts, q = constructed_cloud(case)
    t = capi.Target.points(ctx, pts)
    d, i = t.knn_query(q, k)
    do, io = orc.knn_brute(pts, q, k)
    assert np.array_equal(d, do)
    assert np.array_equal(i, io)
    if k in (15, 17):
        n_gpu = t.estimate_normals(k, compat=True)
        _, ip = orc.knn_brute(pts, pts, k)
        rows = np.arange(0, len(pts), max(len(pts) // 150, 1))
        _assert_smallest_eigvec(pts, ip, n_gpu, rows, f"{case} k={k}")


# ----------------------------------------------------------------------------- certified reuse
def _small_steps(rng, T0, n, rot, trans):
    """A pose sequence the way a converging Gauss-Newton loop produces one: steps that shrink."""
    from point_cloud_registration_amd.synthetic import make_T
    out, T = [], np.array(T0, dtype=np.float64)
    for k in range(n):
        s = 0.5 ** k
        T = T @ make_T(rng.normal(0, rot * s, 3), rng.normal(0, trans * s, 3))
        out.append(T.copy())
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("family", ["copy", "resampled", "crop"])
def test_certified_reuse_is_exact(capi, orc, ctx, name, family):
    """Passes that certify the previous matches (k_certify) and search only the rest return the SAME BITS as passes
    that search everything: walk pose sequences with shrinking steps, jumps, a changed gate and (point targets) a
    changed kind on one scan handle with reuse forced on, and compare every pass with a fresh full search.  The
    families: a noisy copy of target points (matches at the noise level), an independent sample of the same
    surfaces (matches at half the point spacing), a 30 %-overlap crop (most points have nothing in reach)."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan, make_T, T_TRUE_SO3, T_TRUE_T
    rng = np.random.default_rng(11)
    target = street(60_000, seed=5)
    normals = None
    if family == "copy":
        scan, T_true = perturbed_scan(target, 20_000, seed=6)
    else:
        T_true = make_T(T_TRUE_SO3, T_TRUE_T)
        other = street(20_000 if family == "resampled" else 40_000, seed=77)
        if family == "crop":
            other = other[other[:, 0] > 24.0]                   # the far 30 % of the street ...
            other[:, 0] += 30.0                                 # ... pushed so that only a 6 m strip overlaps
        Ri = T_true[:3, :3].T
        scan = ((Ri @ other.astype(np.float64).T).T - Ri @ T_true[:3, 3]).astype(np.float32)
    scan[7] = np.nan                                            # a non-finite scan point never matches
    o_vox = orc.TargetVoxels(target, 1.0)
    if name in ("icp", "plane"):
        tgt = capi.Target.points(ctx, target)
        if name == "plane":
            tgt.estimate_normals(10, want=False)
    else:
        tgt = capi.Target.voxels_from_stats(ctx, o_vox.mean, o_vox.norm, o_vox.icov, 1.0)
    kind = kind_of(capi, name)
    poses = [np.eye(4)] + _small_steps(rng, T_true, 6, 2e-3, 2e-2)
    poses += [poses[-1], poses[-1]]                             # a repeated pose: everything certifies
    poses += _small_steps(rng, np.eye(4), 3, 1e-4, 1e-3)        # a jump back, then small steps again
    gates = [2.0] * len(poses)
    gates[4] = 0.5; gates[5] = 3.0                              # the gate may change between passes
    with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=0):
        ref_scan = capi.Scan(ctx, scan)
        ref = [capi.linearize(tgt, ref_scan, kind, T, md) for T, md in zip(poses, gates)]
    for reuse in (2, 1):
        with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=reuse):
            sc = capi.Scan(ctx, scan)
            for k, (T, md) in enumerate(zip(poses, gates)):
                out = capi.linearize(tgt, sc, kind, T, md)
                assert np.array_equal(out, ref[k]), (name, family, reuse, k, sc.reuse_stats())
            st = sc.reuse_stats()
        if reuse == 2:
            assert st["passes_full"] == 1 and st["passes_track"] == 1 and st["passes_list"] == len(poses) - 2
            assert 0 < st["list_searched"] < st["list_points"], st   # some certified, some searched
    # the oracle agrees (the reference chain: oracle == full search == certified reuse)
    ot = orc.TargetPoints(target, normals=tgt.get_normals() if name == "plane" else None) if name in ("icp", "plane") else o_vox
    for k in (3, len(poses) - 1):
        Ho, go, e2o, cnto = orc.calc_H_g_e2(kind, ot, poses[k], scan, gates[k], with_count=True)
        H, g, e2, cnt = capi.unpack29(ref[k])
        assert cnt == cnto and (cnt == 0 or rel_H(H, Ho) < TOL_ORC)
    assert family == "crop" or capi.unpack29(ref[3])[3] > 100


def test_certified_reuse_shared_point_target(capi, ctx):
    """ICP and PlaneICP passes interleaved on ONE scan and ONE point target share the tracked matches."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(50_000, seed=8)
    scan, T_true = perturbed_scan(target, 15_000, seed=9)
    tgt = capi.Target.points(ctx, target)
    tgt.estimate_normals(10, want=False)
    rng = np.random.default_rng(3)
    poses = _small_steps(rng, T_true, 8, 1e-3, 1e-2)
    kinds = [capi.ICP, capi.PLANE] * 4
    with ctx.pipeline(variant=1, reuse=0):
        s0 = capi.Scan(ctx, scan)
        ref = [capi.linearize(tgt, s0, k, T, 2.0) for k, T in zip(kinds, poses)]
    with ctx.pipeline(variant=1, reuse=2):
        s1 = capi.Scan(ctx, scan)
        got = [capi.linearize(tgt, s1, k, T, 2.0) for k, T in zip(kinds, poses)]
        assert s1.reuse_stats()["passes_list"] == 6
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    # another target: the scan's tracked matches are not valid for it -> a fresh full search, same bits
    tgt2 = capi.Target.points(ctx, target[::2].copy())
    with ctx.pipeline(variant=1, reuse=0):
        r2 = capi.linearize(tgt2, s0, capi.ICP, poses[-1], 2.0)
    with ctx.pipeline(variant=1, reuse=2):
        g2_ = capi.linearize(tgt2, s1, capi.ICP, poses[-1], 2.0)
        assert s1.reuse_stats()["last_mode"] == capi.NN_FULL
    assert np.array_equal(r2, g2_)


def test_deeper_list_set_is_exact(capi, orc, ctx):
    """A point target that has served a dozen search + reduce passes gets a second, deeper set of extended lists (halo
    0.25 cell); passes whose scan moved far since the previous one (or that have no history) read it, the others the
    first set -- per launch for host-driven passes, per iteration (k_gn_update) in the device-resident loop.  Whatever
    is picked, matches and sums must be those of a FRESH target (first set only) and of the oracle."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan, make_T
    target = street(200_000, seed=31)
    scan, T_true = perturbed_scan(target, None, seed=32)
    normals = capi.Target.points(ctx, target).estimate_normals(15)     # (real normals: constant ones leave H singular)
    warm = capi.Target.points(ctx, target, normals)
    sc = capi.Scan(ctx, scan)
    rng = np.random.default_rng(5)
    with ctx.pipeline(variant=1, reuse=0):
        for _ in range(14):                                   # the passes that earn the deeper lists
            capi.linearize(warm, sc, capi.PLANE, np.eye(4), 2.0)
    info = warm.index_info()
    assert info["halo2_records"] > info["halo_records"] > 0 and abs(info["halo2"] - 0.25 * info["cell"]) < 1e-6
    poses = [np.eye(4), T_true]
    T = np.eye(4)
    for step in (0.3, 0.3, 0.1, 0.04, 0.01, 0.003, 0.2, 0.0005, 0.0005):      # large and small displacements in turn
        T = T @ make_T(rng.normal(0, 0.02 * step, 3), rng.normal(0, step, 3))
        poses.append(T.copy())
    ot = orc.TargetPoints(target, normals=normals)
    for k, T in enumerate(poses):
        fresh = capi.Target.points(ctx, target, normals)
        sc_f = capi.Scan(ctx, scan)
        with ctx.pipeline(variant=1, reuse=0):
            a = capi.linearize(warm, sc, capi.PLANE, T, 2.0).copy(); ma = sc.matches()
            b = capi.linearize(fresh, sc_f, capi.PLANE, T, 2.0).copy(); mb = sc_f.matches()
        assert np.array_equal(ma, mb) and np.array_equal(a, b), k
        if k in (0, 1, 4, 9):
            Ho, go, e2o, cnto = orc.calc_H_g_e2(orc.PLANE, ot, T, scan, 2.0, with_count=True)
            H, g, e2, cnt = capi.unpack29(a)
            assert cnt == cnto and rel_H(H, Ho) < 1e-9
    # the device-resident loop picks per iteration: same pose, same iteration count, bit for bit
    fresh = capi.Target.points(ctx, target, normals)
    for kind in (capi.ICP, capi.PLANE):
        T1, it1 = capi.align(warm, sc, kind, np.eye(4), 30, 1e-3, 2.0, flags=capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP)
        T2, it2 = capi.align(fresh, capi.Scan(ctx, scan), kind, np.eye(4), 30, 1e-3, 2.0, flags=capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP)
        assert it1 == it2 and np.array_equal(T1, T2)


def test_quirk_q6_float64_target(capi, orc, g9, pipeline):
    """PlaneICP.set_target with a float64 target (quirk Q6, plane_icp.py:20-22; REPRODUCED since round 5): the reference
    searches a tree built on the float64 array and gathers from the float32 copy.  On the fixture 82 of ~720 engineered
    near-ties get another neighbour under the float64 tree than under a float32 one, and H moves by 2.5e-3
    (tests/test_oracle_golden.py::test_g9_quirk_q6_float64_target has the whole story).  The HIP path -- float32 filter
    search over the index, float64 check, float64 box search for what the bound cannot separate -- must return the
    reference's FLOAT64-tree neighbour for every query, the reference class' own H within 1e-5 at all three poses, the
    same final pose; ICP on the same array keeps the float32 tree (icp.py:19-20); a float32 target is untouched."""
    import point_cloud_registration_amd as pcr
    md = float(g9["max_dist"])
    p = pcr.PlaneICP(max_dist=md, k=int(g9["k"]))
    p.set_target(g9["target"], "tree", g9["plane_normals"])
    d, i = p.kdtree.query(g9["source_tie"])
    assert np.array_equal(np.asarray(i), g9["nn_idx_f64_tree"])        # every query, the near-ties included
    assert d.dtype == np.float64 and np.allclose(d, g9["nn_dist_f64_tree"], rtol=1e-12)
    assert (g9["nn_idx_f64_tree"] != g9["nn_idx_f32_tree"]).sum() >= 50
    # bounded queries: the float64 distance decides
    r = float(np.median(g9["nn_dist_f64_tree"]))
    db, ib = p.kdtree.query(g9["source_tie"], distance_upper_bound=r)
    inside = g9["nn_dist_f64_tree"] < r
    assert np.array_equal(np.asarray(ib)[inside], g9["nn_idx_f64_tree"][inside]) and np.all(np.asarray(ib)[~inside] == -1)
    I = np.eye(4)
    tq = orc.TargetPoints(g9["target"], normals=g9["plane_normals"], tree_f64=True)
    for tag, T, sc in (("T", g9["T"], "source"), ("N", g9["T_near"], "source"), ("E", I, "source_tie")):
        H, g, e2 = p.calc_H_g_e2(T, g9[sc])
        assert rel_H(H, g9[f"{tag}_plane_H"]) < TOL_REF, tag
        assert abs(e2 - g9[f"{tag}_plane_e2"]) < (5 * TOL_REF if tag == "E" else 2e-3) * abs(g9[f"{tag}_plane_e2"])
        Ho, go, e2o = orc.calc_H_g_e2(orc.PLANE, tq, T, g9[sc], md)
        assert rel_H(H, Ho) < 1e-9 and abs(e2 - e2o) <= 1e-9 * abs(e2o), tag
    out = capi.linearize(p._target, capi.Scan(capi.get_context(0), g9["source_tie"]), capi.PLANE, I, md)
    assert capi.unpack29(out)[3] == int((g9["nn_dist_f64_tree"] < md).sum())
    # (compared where the data is: 500 m from the origin a rotation difference of 3e-7 rad moves the translation column
    # by 1.5e-4 m although no scan point moves by more than a few 1e-5 m)
    T_fin, ref = p.align(g9["source"], g9["T_near"]), g9["align_final"]
    src = g9["source"].astype(np.float64)
    moved = np.linalg.norm((src @ T_fin[:3, :3].T + T_fin[:3, 3]) - (src @ ref[:3, :3].T + ref[:3, 3]), axis=1)
    assert moved.max() < 1e-4 and _pose_close(T_fin, ref, tol=5e-4)
    # ICP.set_target searches the float32 copy (icp.py:19-20): the float32 tree's neighbours
    ic = pcr.ICP(max_dist=md)
    ic.set_target(g9["target"])
    di, ii = ic.kdtree.query(g9["source_tie"])
    assert np.array_equal(np.asarray(ii), g9["nn_idx_f32_tree"])
    # ... and so does PlaneICP given a float32 array: the reference class on that tree
    p32 = pcr.PlaneICP(max_dist=md, k=int(g9["k"]))
    p32.set_target(g9["target"].astype(np.float32), "tree", g9["plane_normals"])
    H, g, e2 = p32.calc_H_g_e2(I, g9["source_tie"])
    assert rel_H(H, g9["E_plane_H_f32tree"]) < TOL_REF


@pytest.mark.parametrize("offset", [0.0, 3.0e4, 2.0e7])
@pytest.mark.parametrize("vs", [1.0, 2.0])
def test_centroid_filter_is_exact(capi, orc, ctx, vs, offset):
    """Plain passes over a voxel target run a float32 filter search over the rounded centroids and check the winner in
    float64 (k_nn_filter / k_nn_fix); whatever it cannot certify is searched in float64.  The 29 sums must be
    BIT-identical to the float64-only pipeline (nn_mode 3) -- same matches, same reduce kernel -- and match the oracle:
    ordinary poses, a tight gate, queries ON centroids, duplicated centroids (exact ties -> smaller index), and
    coordinates large enough that the filter certifies little (3e4 m) or is not built at all (2e7 m)."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(300_000, seed=11).astype(np.float64) + np.array([offset, -offset, 0.0])
    scan, T_true = perturbed_scan(target.astype(np.float32), 40_000, seed=12)
    o_vox = orc.TargetVoxels(target, vs)
    mean, norm, icov = o_vox.mean.copy(), o_vox.norm.copy(), o_vox.icov.copy()
    nv = mean.shape[0]
    assert nv > 500
    # duplicated centroids: rows 0..49 again at the end (exact distance ties between distinct indices)
    mean = np.concatenate([mean, mean[:50]]); norm = np.concatenate([norm, norm[:50]]); icov = np.concatenate([icov, icov[:50]])
    g_vox = capi.Target.voxels_from_stats(ctx, mean, norm, icov, vs)
    # queries: the scan, plus points exactly on centroids and exactly between two neighbouring centroids
    on = mean[:2000].astype(np.float32)
    mid = (0.5 * (mean[:2000] + mean[1:2001])).astype(np.float32)
    src = np.ascontiguousarray(np.concatenate([scan, on, mid]), dtype=np.float32)
    sc = capi.Scan(ctx, src)
    poses = [np.eye(4), T_true]
    T = np.eye(4); T[:3, 3] = [0.3, -0.2, 0.1]
    poses.append(T)
    for T in poses:
        for md in (2.0, 0.3, 25.0):
            outs = {}
            for name, mode in (("filter", 0), ("f64", 3)):
                with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=mode, reuse=0):
                    outs[name] = [capi.linearize(g_vox, sc, k, T, md).copy() for k in (capi.VPLANE, capi.NDT)]
            for a, b in zip(outs["filter"], outs["f64"]):
                assert np.array_equal(a, b), (vs, offset, md, a[28], b[28])
    # (the filter index is built by the first pass that can use it; refused when float32 rounding is too coarse)
    assert (g_vox.index_info()["halo_records"] > 0) == (offset < 1e6)
    # and the matches themselves against brute force, through the oracle's sums on the un-duplicated target
    g_ref = capi.Target.voxels_from_stats(ctx, o_vox.mean, o_vox.norm, o_vox.icov, vs)
    for kind in (capi.VPLANE, capi.NDT):
        with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=0):
            out = capi.linearize(g_ref, sc, kind, T_true, 2.0)
        H, g, e2, cnt = capi.unpack29(out)
        Ho, go, e2o, cnto = orc.calc_H_g_e2(kind, o_vox, T_true, src, 2.0, with_count=True)
        assert cnt == cnto
        assert rel_H(H, Ho) < 1e-9


def test_fused_kernel_filter_is_exact(capi, orc, ctx):
    """The fused small-scan kernel searches centroids through the float32 filter with two-way settling once a voxel target
    has served 8 fused passes (`linearize_body<KIND, HALO, FILT>`): the pass before the filter index exists (float64
    search) and the passes after it must give the same 29 sums bit for bit, equal to the split pipelines with and without
    the filter; duplicated centroids (exact ties, settled by the original index) and queries ON centroids / between two of
    them included; the oracle on the un-duplicated target."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan, make_T
    rng = np.random.default_rng(77)
    target = street(300_000, seed=41)
    full, _ = perturbed_scan(target, None, seed=42)
    o_vox = orc.TargetVoxels(target, 1.0)
    for trial in range(6):
        dup = trial % 2 == 1
        mean, norm, icov = o_vox.mean, o_vox.norm, o_vox.icov
        if dup:                                           # every 7th centroid again at the end: exact two-way ties
            mean = np.concatenate([mean, mean[::7]]); norm = np.concatenate([norm, norm[::7]]); icov = np.concatenate([icov, icov[::7]])
        n = int(rng.choice([700, 2049, 30_000, 131_072]))
        src = full[rng.permutation(len(full))[:n]]
        on = o_vox.mean[rng.integers(0, len(o_vox.mean), 300)].astype(np.float32)
        mid = (0.5 * (o_vox.mean[:300] + o_vox.mean[1:301])).astype(np.float32)
        src = np.ascontiguousarray(np.concatenate([src, on, mid]), dtype=np.float32)
        T = make_T(rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)) if trial else np.eye(4)
        for kind, okind in ((capi.VPLANE, orc.VPLANE), (capi.NDT, orc.NDT)):
            tv = capi.Target.voxels_from_stats(ctx, mean, norm, icov, 1.0)
            sc = capi.Scan(ctx, src)
            a = capi.linearize(tv, sc, kind, T, 2.0).copy()              # fused kernel, float64 search: no filter index yet
            assert tv.index_info()["filter_band"] == 0
            for _ in range(9):
                capi.linearize(tv, sc, kind, T, 2.0)
            assert tv.index_info()["filter_band"] > 0                    # built by the 9th fused pass
            b = capi.linearize(tv, sc, kind, T, 2.0).copy()              # fused kernel, filter + settling
            with ctx.pipeline(variant=1, nn_mode=3, reuse=0):
                c = capi.linearize(tv, sc, kind, T, 2.0).copy()          # search + reduce, float64 only
            with ctx.pipeline(variant=1, nn_mode=0, reuse=0):
                d = capi.linearize(tv, sc, kind, T, 2.0).copy()          # search + reduce, filter + prologue
            assert np.array_equal(a, b), (trial, kind, a[28], b[28])
            assert np.array_equal(c, d) and a[28] == c[28], (trial, kind)
            assert np.allclose(a, c, rtol=1e-11, atol=1e-9 * np.max(np.abs(c)))     # (another summation order)
            if not dup:
                Ho, go, e2o, cnto = orc.calc_H_g_e2(okind, o_vox, T, src, 2.0, with_count=True)
                H, g, e2, cnt = capi.unpack29(b)
                assert cnt == cnto and rel_H(H, Ho) < 1e-9
            # device-resident loop == host-driven loop, bit for bit, on the filter path (also after a LARGE step: gn_sincos)
            try:
                Td, itd = capi.align(tv, sc, kind, T, 8, 1e-3, 2.0, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP)
                Th, ith = capi.align(tv, sc, kind, T, 8, 1e-3, 2.0, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_HOST_LOOP)
                assert itd == ith and np.array_equal(Td, Th), (trial, kind)
            except np.linalg.LinAlgError:
                pass


def test_loops_agree_after_a_large_step(capi, ctx):
    """tools/soak.py (round 4): a one-voxel target, 24 correspondences, an ill-conditioned H and a 0.3 rad Gauss-Newton
    step -- the full Rodrigues branch of expSO3, where libm's and the device library's sin / cos differed in the last bit
    and the host-driven and device-resident loops parted ways.  Both now run gn_sincos (csrc/gn_math.h)."""
    rng = np.random.default_rng(3)
    blob = np.clip(rng.normal(0, 0.12, (40, 3)), -0.45, 0.45).astype(np.float64) + np.array([5.5, 3.5, 1.5])   # inside ONE 1 m voxel
    tv = capi.Target.voxels(ctx, blob, 1.0, 10)
    assert tv.size() == 1
    src = (blob[:24] + rng.normal(0, 0.05, (24, 3))).astype(np.float32)
    for n_rep in (1, 1200):                       # 24 points (fused kernel) and the same cloud repeated (larger grid)
        sc = capi.Scan(ctx, np.ascontiguousarray(np.tile(src, (n_rep, 1))))
        for kind in (capi.VPLANE, capi.NDT):
            for T in (np.eye(4), _far_pose()):
                try:
                    Td, itd, trd = capi.align(tv, sc, kind, T, 10, 1e-3, 2.0, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP, want_trace=True)
                    Th, ith, trh = capi.align(tv, sc, kind, T, 10, 1e-3, 2.0, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_HOST_LOOP, want_trace=True)
                except np.linalg.LinAlgError:
                    continue
                assert itd == ith and np.array_equal(trd, trh) and np.array_equal(Td, Th), (n_rep, kind)


def _far_pose():
    from point_cloud_registration_amd.synthetic import make_T
    return make_T([0.2, -0.15, 0.1], [0.05, -0.02, 0.03])


def test_centroid_filter_everything_pending(capi, orc, ctx):
    """EVERY centroid duplicated: every matched point is an exact tie the float32 filter cannot certify, so k_nn_fix
    searches all 1.3 M of them in float64; then a small scan, then the large one again (the stamps of consecutive passes).
    Bit-identical to the float64-only pipeline each time."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(300_000, seed=21)
    o_vox = orc.TargetVoxels(target, 1.0)
    mean = np.concatenate([o_vox.mean, o_vox.mean]); norm = np.concatenate([o_vox.norm, o_vox.norm])
    icov = np.concatenate([o_vox.icov, o_vox.icov])
    g_vox = capi.Target.voxels_from_stats(ctx, mean, norm, icov, 1.0)
    big = np.ascontiguousarray(np.tile(perturbed_scan(target, 130_000, seed=22)[0], (10, 1)), dtype=np.float32)
    small = np.ascontiguousarray(big[:50_000])
    T = np.eye(4); T[:3, 3] = [0.05, -0.03, 0.02]
    for src in (big, small, big):
        sc = capi.Scan(ctx, src)
        outs = []
        for mode in (0, 3):
            with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=mode, reuse=0):
                outs.append([capi.linearize(g_vox, sc, k, T, 2.0).copy() for k in (capi.VPLANE, capi.NDT)])
        for a, b in zip(*outs):
            assert a[28] > 0.5 * len(src)
            assert np.array_equal(a, b)


def test_q6_fallback_on_utm_scale_float64_target(capi, ctx):
    """a float64 cloud at UTM-scale coordinates (float32 ulp 0.03-0.5 m) cannot carry the float64 search through the
    float32 index; ``KDTree`` / ``PlaneICP.set_target`` must keep working on the float32 copy (as before quirk Q6 was
    reproduced) with a warning -- not raise a misleading "not those of the target's float32 points"."""
    import warnings
    import point_cloud_registration_amd as pcr
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-20, 20, (20000, 3)) + np.array([4.0e7, 5.0e7, 100.0])     # float32 ulp 4 m: no usable band
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tree = pcr.KDTree(tgt)
        d, i = tree.query(tgt[:100].astype(np.float32))
        reg = pcr.PlaneICP(max_dist=5.0, k=8)
        reg.set_target(tgt)
        H, g, e2 = reg.calc_H_g_e2(np.eye(4), tgt[:5000].astype(np.float32))
    assert any(issubclass(x.category, RuntimeWarning) for x in w)
    assert d.shape == (100,) and np.all(np.isfinite(d)) and np.all(np.isfinite(H))


def test_internal_flag_bits_are_masked(capi, orc, ctx):
    """bits 27-29 of the flags word are internal (gate switch of quirk Q6, developer timing switches); a caller
    passing them must get the ordinary, gated result."""
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    target = street(30000, seed=4)
    scan, _ = perturbed_scan(target, 8000, seed=5)
    t = capi.Target.points(ctx, target)
    sc = capi.Scan(ctx, scan)
    T = np.eye(4); T[:3, 3] = [0.4, 0.3, 0.2]
    a = capi.linearize(t, sc, capi.ICP, T, 0.3, capi.FLAG_ICP_RR_QUIRK)
    b = capi.linearize(t, sc, capi.ICP, T, 0.3, capi.FLAG_ICP_RR_QUIRK | (1 << 27) | (1 << 28) | (1 << 29))
    assert np.array_equal(a, b) and a[28] < scan.shape[0]          # some points ARE gated out at 0.3 m


@pytest.mark.parametrize("seed", range(6))
def test_heavy_index_fuzz(capi, orc, ctx, seed, monkeypatch):
    """The heavy-cell index (round 6: Morton-sorted cells, 16-byte leaf / group boxes, nearest-first box scans) against brute force:
    clouds made of a sparse background, dense blobs and dense LINES (hundreds to thousands of points per cell), at the origin and
    at |p| ~ 1e4 m (where the boxes' quantisation margin has to grow with the coordinates' ulp), queries inside, near and far;
    index and distance bit for bit, for the query seam, the search + reduce kernels and the fused small-scan kernel."""
    rng = np.random.default_rng(100 + seed)
    off = np.array([0.0, 0.0, 0.0]) if seed % 2 == 0 else np.array([9000.0, -7000.0, 300.0])
    n_bg = 20000
    parts = [rng.uniform(-20, 20, (n_bg, 3)) * [1, 1, 0.1]]
    for _ in range(4):                                             # blobs
        c = rng.uniform(-15, 15, 3) * [1, 1, 0.1]
        parts.append(c + rng.normal(0, rng.uniform(0.02, 0.3), (int(rng.integers(500, 6000)), 3)))
    for _ in range(4):                                             # lines
        a, b = rng.uniform(-18, 18, 3) * [1, 1, 0.1], rng.uniform(-18, 18, 3) * [1, 1, 0.1]
        t = rng.uniform(0, 1, int(rng.integers(2000, 20000)))[:, None]
        parts.append(a + t * (b - a) + rng.normal(0, 0.01, (t.shape[0], 3)))
    if seed == 5:                                                  # exact duplicates: ties go to the smaller original index
        parts.append(np.repeat(parts[1][:50], 40, axis=0))
    target = (np.concatenate(parts) + off).astype(np.float32)
    target = target[rng.permutation(target.shape[0])]
    monkeypatch.setenv("PCR_HEAVY", "1")
    if seed == 3:
        monkeypatch.setenv("PCR_GRID_CELL", "1.5")                 # very heavy cells
    t = capi.Target.points(ctx, target)
    info = t.index_info()
    assert info["heavy"] and info["pop_max"] > 64, info
    q = np.concatenate([target[rng.choice(target.shape[0], 3000)] + rng.normal(0, 0.02, (3000, 3)),
                        target[rng.choice(target.shape[0], 2000)] + rng.normal(0, 0.6, (2000, 3)),
                        rng.uniform(-30, 30, (1000, 3)) * [1, 1, 0.3] + off]).astype(np.float32)
    d, i = t.nn_query(q)
    do, io = orc.nn_brute(target, q)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    db, ib = t.nn_query(q, 0.5)                                    # bounded
    keep = do < 0.5
    assert np.array_equal(ib[keep], io[keep]) and np.all(ib[~keep] == -1)
    ot = orc.TargetPoints(target, cell=1.0)
    T = np.eye(4); T[:3, 3] = [0.05, -0.03, 0.02]
    for scan in (q, np.concatenate([q] * 60)):                     # fused small-scan kernel / search + reduce kernels
        sc = capi.Scan(ctx, scan)
        H, g, e2, cnt = capi.unpack29(capi.linearize(t, sc, capi.ICP, T, 1.0))
        Ho, go, e2o, cnto = orc.calc_H_g_e2(orc.ICP, ot, T, scan, 1.0, with_count=True)
        assert cnt == cnto and rel_H(H, Ho) < 1e-9 and abs(e2 - e2o) <= 1e-9 * abs(e2o)
        sc.close()
    t.close()
