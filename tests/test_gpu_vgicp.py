"""VGICP on the GPU: the voxel covariances and their round trip, the sums of one pass, the gate, align, and the neighbours it
must leave undisturbed.

Fixture: g2_mini_street -- voxel size 1.0, 218 kept voxels, 2000 scan points, gate 0.8, 1785 kept (89.25 %), non-identity T.
No centroid distance lies within 1.3e-3 relative of the gate and the smallest gap between first and second centroid is 8.6e-5 m,
so masks and indices compare exactly: a brute force over vox_mean reproduces vox_idx (tests/test_vgicp_api.py).  The sums are
restated (tests/vgicp_cases.py) from the GOLDEN vox_idx and the GPU's own read-back centroids and covariances -- what the pass
used.  Transformed points come from vgicp_cases.xform32, the kernels' float32 transform in their order of operations.

Bounds:
  covariances RAW    the bits of six(VoxelGrid.cov)
  covariances PLANE  |dC| <= 2^-50 per entry against plane_cov(voxels.norm, eps): entries <= 1, three float64 operations per
                     entry; eigenvalues within 1e-12 of (eps, 1, 1) on ALL voxels
  sums               per entry gicp_cases.sum_bound: (n + 16 / eps_min) 2^-53 sum_i |term_i| against math.fsum of the restated
                     terms (eps_min = smallest eigenvalue over the summed covariance matrices); conftest.step_err <= 1e-10
  align              against vgicp_cases.align_numpy fed the read-back Cp and Cv: the same iteration count and
                     max|T - T_numpy| <= 1e-8 = the step_err bound per pass added over at most 30 passes"""

import gc as pygc

import numpy as np
import pytest

import gicp_cases as gc
import vgicp_cases as vc
from conftest import step_err

pytestmark = pytest.mark.gpu

EPS = 1e-3
NAMES = ("raw", "plane", "spd")
KEPT = 1785


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


def voxel_target(capi, ctx, g2):
    return capi.Target.voxels(ctx, g2["target"], float(g2["voxel_size"]))


def check_plane_spectrum(C):
    assert np.all(np.isfinite(C))
    lam = np.linalg.eigvalsh(gc.full3(C))
    assert np.max(np.abs(lam - np.array([EPS, 1.0, 1.0]))) <= 1e-12, np.max(np.abs(lam - np.array([EPS, 1.0, 1.0])))


# ----------------------------------------------------------------------------- 1. voxel covariances
def test_voxel_covariances(capi, ctx, g2):
    import point_cloud_registration_amd as pcr
    t = voxel_target(capi, ctx, g2)
    nv = t.size()
    assert nv == 218
    with pytest.raises(ValueError):
        t.get_voxel_covariances()                             # none yet
    st = t.voxel_stats(("cov", "norm"))
    t.set_voxel_covariances(capi.COV_RAW)
    assert np.array_equal(t.get_voxel_covariances(), gc.six(st["cov"]))
    t.set_voxel_covariances(capi.COV_PLANE, EPS)
    plane = t.get_voxel_covariances()
    err = np.max(np.abs(plane - vc.plane_cov(st["norm"], EPS)))
    print(f"PLANE max err {err:.3e}")
    assert plane.dtype == np.float64 and plane.shape == (nv, 6) and err <= 2.0 ** -50
    check_plane_spectrum(plane)
    # the class reads the same rows: "raw" = six(VoxelGrid.cov) bit for bit, "plane" from VoxelGrid.norm
    reg = pcr.VGICP(voxel_size=float(g2["voxel_size"]), regularization="raw")
    reg.set_target(g2["target"])
    assert np.array_equal(reg.covariance, gc.six(reg.voxels.cov)) and np.array_equal(reg.voxels.cov, st["cov"])
    reg = pcr.VGICP(voxel_size=float(g2["voxel_size"]), eps=EPS)
    reg.set_target(g2["target"])
    assert np.array_equal(reg.covariance, plane)
    # given by the caller: both shapes come back bit for bit
    rng = np.random.default_rng(1)
    C = rng.normal(size=(nv, 6))
    t.set_voxel_covariances(cov=C)
    assert np.array_equal(t.get_voxel_covariances(), C)
    t.set_voxel_covariances(capi.COV_RAW)
    t.set_voxel_covariances(cov=gc.full3(C))                  # (Nv, 3, 3) form
    assert np.array_equal(t.get_voxel_covariances(), C)
    reg.set_covariance(C)
    assert np.array_equal(reg.covariance, C)
    # refused: non-finite entries (the old ones stay), wrong shapes, point targets
    for bad_value in (np.nan, np.inf):
        bad = C.copy()
        bad[123, 4] = bad_value
        with pytest.raises(ValueError):
            t.set_voxel_covariances(cov=bad)
        assert np.array_equal(t.get_voxel_covariances(), C)
    for shape in ((nv - 1, 6), (nv, 5), (nv, 3, 2), (nv * 6,)):
        with pytest.raises(ValueError):
            t.set_voxel_covariances(cov=np.zeros(shape))
    with pytest.raises(ValueError):
        t.set_voxel_covariances(capi.COV_PLANE, 0.0)
    with pytest.raises(ValueError):
        t.set_voxel_covariances(7, EPS)
    assert np.array_equal(t.get_voxel_covariances(), C)
    p = capi.Target.points(ctx, g2["target"])
    with pytest.raises(ValueError):
        p.set_voxel_covariances(capi.COV_PLANE, EPS)
    with pytest.raises(ValueError):
        p.get_voxel_covariances()


# ----------------------------------------------------------------------------- 2. sums, kernel-only
@pytest.fixture(scope="module")
def sides(capi, ctx, g2):
    """name -> (Cp float32 (N, 6), target with its voxel covariances set, Cv read back, centroids read back): raw / plane
    voxel covariances under the scan's estimated PLANE ones, and random SPD matrices with condition <= 100 from
    default_rng(0) on both sides (the voxel side widened to float64).  Computed once, never modified."""
    src = g2["source"]
    rng = np.random.default_rng(0)
    cp_plane = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances(10, capi.COV_PLANE, EPS)
    cp_spd = gc.random_spd(len(src), rng)
    cv_spd = gc.random_spd(218, rng).astype(np.float64)
    out = {}
    for name in NAMES:
        t = voxel_target(capi, ctx, g2)
        if name == "raw":
            t.set_voxel_covariances(capi.COV_RAW)
        elif name == "plane":
            t.set_voxel_covariances(capi.COV_PLANE, EPS)
        else:
            t.set_voxel_covariances(cov=cv_spd)
        cp = cp_spd if name == "spd" else cp_plane
        cv, mean = t.get_voxel_covariances(), t.voxel_stats(("mean",))["mean"]
        for a in (cp, cv, mean):
            a.setflags(write=False)
        out[name] = (cp, t, cv, mean)
    return out


@pytest.fixture(scope="module")
def restated(g2, sides):
    """name -> (terms (N, 28), eps_min, mask): the definition at g2's pose from the GOLDEN centroid matches."""
    T, src, idx, md = g2["T"], g2["source"], g2["vox_idx"], float(g2["max_dist"])
    tp = vc.xform32(T, src)
    out = {}
    for name, (cp, _, cv, mean) in sides.items():
        d = tp.astype(np.float64) - mean[idx]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        mask = dist < md
        assert int(mask.sum()) == KEPT and np.array_equal(mask, g2["vox_dist"] < md)
        t, eps_min = vc.terms(T, src, tp, mean[idx], cp, cv[idx], mask)
        t.setflags(write=False)
        out[name] = (t, eps_min, mask)
    return out


def reference(restated, name, n=None):
    t, eps_min, mask = restated[name]
    n = len(mask) if n is None else n
    ref, mag = gc.fsum_cols(t[:n])
    kept = int(mask[:n].sum())
    return ref, gc.sum_bound(kept, eps_min, mag), kept


def gpu_sums(capi, ctx, g2, sides, name, n=None, flags=None, max_dist=None):
    cp, t = sides[name][:2]
    n = len(cp) if n is None else n
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    s.set_covariances(np.ascontiguousarray(cp[:n]))
    md = float(g2["max_dist"]) if max_dist is None else max_dist
    return capi.vgicp_linearize(t, s, g2["T"], md), t, s


@pytest.mark.parametrize("name", NAMES)
def test_sums(capi, ctx, g2, sides, restated, name):
    out, t, s = gpu_sums(capi, ctx, g2, sides, name)
    ref, bound, kept = reference(restated, name)
    assert kept == KEPT and out[28] == kept
    err = np.abs(out[:28] - ref)
    H, g, _ = gc.unpack28(out[:28])
    Href, gref, _ = gc.unpack28(ref)
    se = step_err(H, g, Href, gref)
    print(f"{name}: eps_min {restated[name][1]:.3e}, max err / bound {np.max(err / bound):.3e}, "
          f"bound / max|H| {bound[:21].max() / np.abs(ref[:21]).max():.3e}, step_err {se:.3e}")
    assert np.all(err <= bound)
    assert se <= 1e-10
    # two consecutive calls return the same bits
    again = capi.vgicp_linearize(t, s, g2["T"], float(g2["max_dist"]))
    assert np.array_equal(out, again)
    # the scan in the caller's order on the device
    nosort = gpu_sums(capi, ctx, g2, sides, name, flags=capi.FLAG_NO_SCAN_SORT)[0]
    assert nosort[28] == kept and np.all(np.abs(nosort[:28] - ref) <= bound) and np.all(np.abs(nosort[:28] - out[:28]) <= bound)


# one lane, a wave edge, a block edge, one trip plus one point for two and for three points per lane, the full scan
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 513, 769, 2000])
def test_sums_prefixes(capi, ctx, g2, sides, restated, n):
    """Correspondences of a subset of the scan are a subset of g2's."""
    for name in NAMES:
        out = gpu_sums(capi, ctx, g2, sides, name, n=n)[0]
        ref, bound, kept = reference(restated, name, n)
        assert out[28] == kept
        assert np.all(np.abs(out[:28] - ref) <= bound)
        if n == 0:
            assert np.array_equal(out, np.zeros(29))


def test_nothing_inside_the_gate(capi, ctx, g2, sides):
    import point_cloud_registration_amd as pcr
    out = gpu_sums(capi, ctx, g2, sides, "spd", max_dist=1e-6)[0]
    assert np.array_equal(out, np.zeros(29))
    reg = pcr.VGICP(voxel_size=float(g2["voxel_size"]), max_dist=1e-6)
    reg.set_target(g2["target"])
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(g2["source"], init_T=g2["T"], source_cov=sides["spd"][0])


def test_errors(capi, ctx, g2, sides):
    """A point target, a voxel target without covariances and a scan without covariances are refused with a message."""
    cp, t = sides["plane"][:2]
    T, md = g2["T"], float(g2["max_dist"])
    s = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER)
    with pytest.raises(ValueError, match="scan has no covariances"):
        capi.vgicp_linearize(t, s, T, md)
    s.set_covariances(cp)
    with pytest.raises(ValueError, match="voxel target"):
        capi.vgicp_linearize(capi.Target.points(ctx, g2["target"]), s, T, md)
    with pytest.raises(ValueError, match="target has no covariances"):
        capi.vgicp_linearize(voxel_target(capi, ctx, g2), s, T, md)
    with pytest.raises(ValueError, match="target has no covariances"):
        capi.vgicp_align(voxel_target(capi, ctx, g2), s, T, 3, 1e-3, md)


# ----------------------------------------------------------------------------- 5. single-voxel target
def test_single_voxel_target(capi, ctx, g1):
    """g1's 100 target points form one kept voxel: every scan point inside the gate matches it."""
    T, src, md = g1["T"], g1["source"], float(g1["max_dist"])
    t = capi.Target.voxels(ctx, g1["target"], float(g1["voxel_size"]))
    assert t.size() == 1
    t.set_voxel_covariances(capi.COV_PLANE, EPS)
    cv, mean = t.get_voxel_covariances(), t.voxel_stats(("mean",))["mean"]
    check_plane_spectrum(cv)
    s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    cp = s.estimate_covariances(10, capi.COV_PLANE, EPS)
    tp = vc.xform32(T, src)
    dist, idx = vc.nearest_centroid(tp, mean)
    mask = dist < md
    terms, eps_min = vc.terms(T, src, tp, mean[idx], cp, cv[idx], mask)
    ref, mag = gc.fsum_cols(terms)
    kept = int(mask.sum())
    assert kept == 100                                       # (no distance within 0.3 relative of the gate)
    out = capi.vgicp_linearize(t, s, T, md)
    assert out[28] == kept
    assert np.all(np.abs(out[:28] - ref) <= gc.sum_bound(kept, eps_min, mag))


# ----------------------------------------------------------------------------- 6. target with no kept voxel
def test_target_with_no_kept_voxel(g2):
    """Five points stay below min_points: VGICP.set_target ends as NDT.set_target ends on the same input."""
    import point_cloud_registration_amd as pcr
    pts = np.ascontiguousarray(g2["target"][:5])

    def outcome(reg):
        try:
            reg.set_target(pts)
        except Exception as exc:                             # noqa: BLE001
            return type(exc).__name__, None
        return "ok", reg.voxels.mean.shape

    ndt, vgicp = pcr.NDT(voxel_size=1.0), pcr.VGICP(voxel_size=1.0)
    o_ndt, o_vgicp = outcome(ndt), outcome(vgicp)
    print(f"NDT: {o_ndt}, VGICP: {o_vgicp}")
    assert o_ndt == o_vgicp
    if o_vgicp[0] == "ok":
        assert vgicp.covariance.shape == (0, 6)
        H, g, e2 = vgicp.calc_H_g_e2(np.eye(4), g2["source"])
        assert not H.any() and not g.any() and e2 == 0.0 and vgicp.last_correspondences == 0


# ----------------------------------------------------------------------------- 7. the per-point loop of the class
def test_no_parallel_ver(g2, sides, restated):
    import point_cloud_registration_amd as pcr
    cp, _, cv, _ = sides["plane"]
    reg = pcr.VGICP(voxel_size=float(g2["voxel_size"]), max_dist=float(g2["max_dist"]), eps=EPS)
    reg.set_target(g2["target"])
    assert np.array_equal(reg.covariance, cv)
    H, g, e2 = reg.calc_H_g_e2_no_parallel_ver(g2["T"], g2["source"], source_cov=cp)
    ref, bound, _ = reference(restated, "plane")
    assert np.all(np.abs(np.concatenate([H[gc.TRIU], g, [e2]]) - ref) <= bound)
    Hk, gk, e2k = reg.calc_H_g_e2(g2["T"], g2["source"], source_cov=cp)
    assert np.all(np.abs(np.concatenate([Hk[gc.TRIU], gk, [e2k]]) - ref) <= bound)
    assert reg.last_correspondences == KEPT
    assert np.all(np.abs(np.concatenate([(H - Hk)[gc.TRIU], g - gk, [e2 - e2k]])) <= bound)


# ----------------------------------------------------------------------------- 8. gate
@pytest.fixture(scope="module")
def case():
    target, scan, T_true = gc.align_case()
    for a in (target, scan, T_true):
        a.setflags(write=False)
    return target, scan, T_true


def test_gate(case):
    """T = I, max_dist = 0.45 over 200 kept voxels: 65.0 % kept (666 of 1024), none within 2.6e-3 relative of the gate: the
    count equals the mask recomputed from the class's own centroid search."""
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.VGICP(voxel_size=1.0, max_dist=0.45, k=10)
    reg.set_target(target)
    assert len(reg.voxels.mean) == 200
    dist = reg.voxels.kdtree.query(vc.xform32(np.eye(4), scan))[0]
    assert np.min(np.abs(dist / 0.45 - 1.0)) > 1e-3
    kept = int((dist < 0.45).sum())
    assert abs(kept / len(scan) - 0.650) < 0.005, kept / len(scan)
    reg.calc_H_g_e2(np.eye(4), scan)
    assert reg.last_correspondences == kept


# ----------------------------------------------------------------------------- 9. align
@pytest.mark.parametrize("regularization", ["plane", "raw"])
@pytest.mark.parametrize("max_dist", [2.0, 0.6])
def test_align(capi, case, max_dist, regularization):
    """The NumPy restatement converges in 3 iterations in all four runs and reaches |dR|_F 3.4e-3 to 5.4e-3, |dt| 6.9e-3 to
    9.3e-3 m from 3.8e-2 / 0.114: centroids of 1 m voxels bias the pose, so accuracy against T_true is a sanity condition."""
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.math_tools import plus
    target, scan, T_true = case
    reg = pcr.VGICP(voxel_size=1.0, max_dist=max_dist, k=10, regularization=regularization)
    reg.set_target(target)
    T = reg.align(scan)
    iters = reg.last_iterations
    dR, dt = np.linalg.norm(T[:3, :3] - T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])
    dR0, dt0 = np.linalg.norm(np.eye(3) - T_true[:3, :3]), np.linalg.norm(T_true[:3, 3])
    print(f"{regularization} max_dist {max_dist}: {iters} iterations, |dR|_F {dR:.3e} (start {dR0:.3e}), |dt| {dt:.3e} (start {dt0:.3e})")
    assert dR < 0.5 * dR0 and dt < 0.5 * dt0
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
    # every trace row's sums are the bits pcr_vgicp_linearize returns at that row's pose
    dev = reg._gicp_scan(scan, None)
    T2, iters2, trace = capi.vgicp_align(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, max_dist, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(capi.vgicp_linearize(reg._target, dev, row[:16], max_dist), row[16:])
    # max_iter = 0 returns init_T
    T0 = plus(np.eye(4), np.array([0.01, 0.02, 0.03, 0.001, 0.002, 0.003]))
    reg0 = pcr.VGICP(voxel_size=1.0, max_dist=max_dist, k=10, max_iter=0, regularization=regularization)
    reg0.set_target(target)
    assert np.array_equal(reg0.align(scan, init_T=T0), T0) and reg0.last_iterations == 0
    # the NumPy restatement of the whole loop, fed what the GPU used
    Tn, itn = vc.align_numpy(scan, reg.voxels.mean, reg.source_covariance(scan), reg.covariance, max_dist,
                             max_iter=reg.max_iter, tol=reg.tol)
    print(f"    against align_numpy: {itn} iterations, max|T - T_numpy| {np.max(np.abs(T - Tn)):.3e}")
    assert itn == iters
    assert np.max(np.abs(T - Tn)) <= 1e-8


# ----------------------------------------------------------------------------- 10. device memory
def test_align_device_memory_is_stable(capi, ctx, case):
    import torch
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.VGICP(voxel_size=1.0, max_dist=2.0, k=10)
    reg.set_target(target)
    first = reg.align(scan); pygc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        last = reg.align(scan)
    pygc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
    assert np.array_equal(first, last)


# ----------------------------------------------------------------------------- 11. neighbours undisturbed
def test_neighbours_undisturbed(capi, ctx, g2):
    """NDT / VPlaneICP return the same bits before and after a VGICP pass on one context; pcr_linearize(NDT) on the very same
    pcr_target returns the same bits before and after its voxel covariances are set and a VGICP pass has run over it; one
    device scan serves GICP, then VGICP, with the covariances GICP put on it."""
    import point_cloud_registration_amd as pcr
    T, src, tgt, md, vs = g2["T"], g2["source"], g2["target"], float(g2["max_dist"]), float(g2["voxel_size"])
    ndt, vplane = pcr.NDT(voxel_size=vs, max_dist=md), pcr.VPlaneICP(voxel_size=vs, max_dist=md)
    vgicp, gicp = pcr.VGICP(voxel_size=vs, max_dist=md), pcr.GICP(max_dist=md)
    for reg in (ndt, vplane, vgicp, gicp):
        reg.set_target(tgt)
    for variant in (2, 1):
        with ctx.pipeline(variant=variant):
            before = [reg.calc_H_g_e2(T, src) for reg in (ndt, vplane)]
            vgicp.calc_H_g_e2(T, src)
            assert vgicp.last_correspondences == KEPT
            after = [reg.calc_H_g_e2(T, src) for reg in (ndt, vplane)]
            for b, a in zip(before, after):
                assert all(np.array_equal(x, y) for x, y in zip(b, a))
            # the very same pcr_target and the very same device scan
            t = voxel_target(capi, ctx, g2)
            s = capi.Scan(ctx, src)
            s.estimate_covariances(10, want=False)
            o1 = capi.linearize(t, s, capi.NDT, T, md)
            t.set_voxel_covariances(capi.COV_PLANE, EPS)
            v1 = capi.vgicp_linearize(t, s, T, md)
            o2 = capi.linearize(t, s, capi.NDT, T, md)
            v2 = capi.vgicp_linearize(t, s, T, md)
            assert np.array_equal(o1, o2) and np.array_equal(v1, v2) and v1[28] == o1[28] == KEPT
            # GICP, then VGICP over one uploaded scan: estimated once, the same bits on it afterwards
            h = gicp.upload(src, keep_order=True)
            estimates = []
            estimate = h._scan.estimate_covariances
            h._scan.estimate_covariances = lambda *a, **kw: (estimates.append(a), estimate(*a, **kw))[1]
            gicp.calc_H_g_e2(T, h)
            c1 = h._scan.get_covariances()
            vgicp.calc_H_g_e2(T, h)
            c2 = h._scan.get_covariances()
            assert len(estimates) == 1 and np.array_equal(c1, c2)
            assert np.array_equal(vgicp.source_covariance(h), c1) and vgicp.last_correspondences == KEPT
            h.close()
