"""GICP on the GPU: estimated covariances, the covariance round trip, the sums of one pass, the gate, align, and the
neighbours it must leave undisturbed.

Fixture: g2_mini_street -- 5000 targets, 2000 scan points, gate 0.8, 91.15 % kept (1823), non-identity T with ~0.07 rad of
rotation.  No distance lies within 1e-4 of the gate and there are no near-ties (smallest gap between first and second
neighbour 1.4e-5 m), so masks and indices compare exactly; nn_idx / nn_dist are the reference's.  Transformed points come from
orc.transform, which is bit-identical to the kernels' xform.

Bounds (tests/gicp_cases.py restates the definition in float64 NumPy):
  covariances RAW    |dC| <= 2^-23 max|C_ref| per point: float32 storage rounds at 2^-25 relative, margin 4
  covariances PLANE  |dC| <= 2^-23 per entry (entries <= 1) on the points whose reference eigen-gap (l1 - l0) / l2 > 0.05 --
                     at least 95 % of them; eigenvalues within 1e-6 of (eps, 1, 1) on ALL points
  sums               per entry (n + 16 / eps_min) 2^-53 sum_i |term_i| against math.fsum of the restated terms: summation error
                     of n kept terms plus the conditioning of the 3x3 inverse (eps_min = smallest eigenvalue over the summed
                     covariance matrices); conftest.step_err <= 1e-10."""

import gc as pygc

import numpy as np
import pytest

import gicp_cases as gc
from conftest import step_err

pytestmark = pytest.mark.gpu

EPS = 1e-3
SIZES = (1, 5, 63, 64, 65, 257)


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


def neighbours(points, k):
    """The GPU's own exact k-NN of every point within its cloud (pinned bit-exact by the k-NN tests); padding = len(points)."""
    import point_cloud_registration_amd as pcr
    idx = pcr.KDTree(points).query(points, k)[1]
    return idx.reshape(len(points), -1)


def estimate(capi, ctx, side, points, k, mode):
    if side == "target":
        return capi.Target.points(ctx, points).estimate_covariances(k, mode, EPS)
    return capi.Scan(ctx, points, flags=capi.FLAG_KEEP_ORDER).estimate_covariances(k, mode, EPS)


def check_plane_spectrum(C):
    assert np.all(np.isfinite(C))
    lam = np.linalg.eigvalsh(gc.full3(C))
    assert np.max(np.abs(lam - np.array([EPS, 1.0, 1.0]))) <= 1e-6, np.max(np.abs(lam - np.array([EPS, 1.0, 1.0])))


# ----------------------------------------------------------------------------- 1. estimated covariances
@pytest.mark.parametrize("k", [10, 20])
@pytest.mark.parametrize("side", ["target", "scan"])
def test_estimated_covariances(capi, ctx, g2, side, k):
    pts = g2["target"] if side == "target" else g2["source"]
    nbr = neighbours(pts, k)
    ref_plane, ref_raw, gap = gc.covariance(pts, nbr, "plane", EPS)
    raw = estimate(capi, ctx, side, pts, k, capi.COV_RAW)
    plane = estimate(capi, ctx, side, pts, k, capi.COV_PLANE)
    assert raw.dtype == np.float32 and raw.shape == (len(pts), 6) and plane.shape == (len(pts), 6)
    err_raw = np.max(np.abs(raw - ref_raw), axis=1) / np.max(np.abs(ref_raw), axis=1)
    sel = gap > 0.05
    err_plane = np.max(np.abs(plane - ref_plane), axis=1)
    print(f"{side} k={k}: RAW max rel err {err_raw.max():.3e}; PLANE compared {sel.mean():.4f}, max err {err_plane[sel].max():.3e}")
    assert np.all(np.isfinite(raw)) and np.all(err_raw <= 2.0 ** -23)
    assert sel.mean() >= 0.95
    assert np.all(err_plane[sel] <= 2.0 ** -23)
    check_plane_spectrum(plane)


@pytest.mark.parametrize("side", ["target", "scan"])
def test_estimated_covariances_edge_sizes(capi, ctx, g2, side):
    for n in SIZES:
        pts = np.ascontiguousarray(g2["target"][:n])
        nbr = neighbours(pts, 10)
        ref_raw = gc.covariance(pts, nbr, "raw")[0]
        raw = estimate(capi, ctx, side, pts, 10, capi.COV_RAW)
        assert raw.shape == (n, 6) and np.all(np.isfinite(raw))
        assert np.all(np.max(np.abs(raw - ref_raw), axis=1) <= 2.0 ** -23 * np.max(np.abs(ref_raw), axis=1)), n
        check_plane_spectrum(estimate(capi, ctx, side, pts, 10, capi.COV_PLANE))
    pts = np.ascontiguousarray(g2["target"][:64])
    for k in (0, 65):
        with pytest.raises(ValueError):
            estimate(capi, ctx, side, pts, k, capi.COV_PLANE)
    # estimating without reading back works on any scan, an empty one included
    capi.Scan(ctx, pts).estimate_covariances(10, want=False)
    capi.Scan(ctx, pts[:0]).estimate_covariances(10, want=False)


# ----------------------------------------------------------------------------- 2. round trip
def test_covariance_round_trip(capi, ctx, g2):
    rng = np.random.default_rng(1)
    tgt, src = g2["target"], g2["source"]
    Cq, Cp = rng.normal(size=(len(tgt), 6)).astype(np.float32), rng.normal(size=(len(src), 6)).astype(np.float32)
    t = capi.Target.points(ctx, tgt)
    with pytest.raises(ValueError):
        t.get_covariances()                                   # none yet
    t.set_covariances(Cq)
    assert np.array_equal(t.get_covariances(), Cq)
    for flags in (capi.FLAG_KEEP_ORDER, capi.FLAG_NO_SCAN_SORT):
        s = capi.Scan(ctx, src, flags=flags)
        s.set_covariances(Cp)
        assert np.array_equal(s.get_covariances(), Cp)
        s.set_covariances(gc.full3(Cp))                       # (N, 3, 3) form
        assert np.array_equal(s.get_covariances(), Cp)
    plain = capi.Scan(ctx, src)
    with pytest.raises(ValueError):
        plain.set_covariances(Cp)
    plain.estimate_covariances(10, want=False)
    with pytest.raises(ValueError):
        plain.get_covariances()
    with pytest.raises(ValueError):
        plain.estimate_covariances(10, want=True)
    bad = Cp.copy()
    bad[1234, 3] = np.nan
    with pytest.raises(ValueError):
        capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).set_covariances(bad)
    badq = Cq.copy()
    badq[7, 0] = np.inf
    with pytest.raises(ValueError):
        t.set_covariances(badq)
    assert np.array_equal(t.get_covariances(), Cq)            # a refused set leaves the old ones


# ----------------------------------------------------------------------------- 3. sums, kernel-only
@pytest.fixture(scope="module")
def covsets(capi, ctx, g2):
    """Covariances for both sides, so the sums do not depend on test 1: the PLANE ones read back from the GPU, and random
    SPD matrices with condition <= 100 from default_rng(0).  Computed once, never modified."""
    tgt, src = g2["target"], g2["source"]
    rng = np.random.default_rng(0)
    out = {"plane": (capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances(10, capi.COV_PLANE, EPS),
                     capi.Target.points(ctx, tgt).estimate_covariances(10, capi.COV_PLANE, EPS)),
           "spd": (gc.random_spd(len(src), rng), gc.random_spd(len(tgt), rng))}
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def restated(g2, orc, covsets):
    """name -> (terms (N, 28), eps_min, mask): the definition at g2's pose from the GOLDEN correspondences."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    tp = orc.transform(T, src)
    out = {}
    for name, (Cp, Cq) in covsets.items():
        t, eps_min = gc.terms(T, src, tp, tgt[g2["nn_idx"]], Cp, Cq[g2["nn_idx"]], mask)
        t.setflags(write=False)
        out[name] = (t, eps_min, mask)
    return out


def reference(restated, name, n=None):
    t, eps_min, mask = restated[name]
    n = len(mask) if n is None else n
    ref, mag = gc.fsum_cols(t[:n])
    kept = int(mask[:n].sum())
    return ref, gc.sum_bound(kept, eps_min, mag), kept


def gpu_sums(capi, ctx, g2, covsets, name, n=None, flags=None, max_dist=None):
    Cp, Cq = covsets[name]
    n = len(Cp) if n is None else n
    t = capi.Target.points(ctx, g2["target"])
    t.set_covariances(Cq)
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    s.set_covariances(np.ascontiguousarray(Cp[:n]))
    md = float(g2["max_dist"]) if max_dist is None else max_dist
    return capi.gicp_linearize(t, s, g2["T"], md), t, s


@pytest.mark.parametrize("name", ["plane", "spd"])
def test_sums(capi, ctx, g2, covsets, restated, name):
    out, t, s = gpu_sums(capi, ctx, g2, covsets, name)
    ref, bound, kept = reference(restated, name)
    assert kept == 1823 and out[28] == kept
    err = np.abs(out[:28] - ref)
    print(f"{name}: max err / bound {np.max(err / bound):.3e}, bound / max|H| {bound[:21].max() / np.abs(ref[:21]).max():.3e}")
    assert np.all(err <= bound)
    H, g, _ = gc.unpack28(out[:28])
    Href, gref, _ = gc.unpack28(ref)
    assert step_err(H, g, Href, gref) <= 1e-10
    # two consecutive calls return the same bits
    again = capi.gicp_linearize(t, s, g2["T"], float(g2["max_dist"]))
    assert np.array_equal(out, again)
    # the scan in the caller's order on the device
    nosort = gpu_sums(capi, ctx, g2, covsets, name, flags=capi.FLAG_NO_SCAN_SORT)[0]
    assert nosort[28] == kept and np.all(np.abs(nosort[:28] - ref) <= bound) and np.all(np.abs(nosort[:28] - out[:28]) <= bound)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_sums_prefixes(capi, ctx, g2, covsets, restated, n):
    """Correspondences of a subset of the scan are a subset of g2's."""
    for name in ("plane", "spd"):
        out = gpu_sums(capi, ctx, g2, covsets, name, n=n)[0]
        ref, bound, kept = reference(restated, name, n)
        assert out[28] == kept
        assert np.all(np.abs(out[:28] - ref) <= bound)
        if n == 0:
            assert np.array_equal(out, np.zeros(29))


def test_nothing_inside_the_gate(capi, ctx, g2, covsets):
    import point_cloud_registration_amd as pcr
    out = gpu_sums(capi, ctx, g2, covsets, "spd", max_dist=1e-6)[0]
    assert np.array_equal(out, np.zeros(29))
    Cp, Cq = covsets["spd"]
    reg = pcr.GICP(max_dist=1e-6)
    reg.set_target(g2["target"], cov=Cq)
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(g2["source"], init_T=g2["T"], source_cov=Cp)


def test_no_parallel_ver(g2, covsets, restated):
    import point_cloud_registration_amd as pcr
    Cp, Cq = covsets["plane"]
    reg = pcr.GICP(max_dist=float(g2["max_dist"]))
    reg.set_target(g2["target"], cov=Cq)
    assert np.array_equal(reg.covariance, Cq)
    H, g, e2 = reg.calc_H_g_e2_no_parallel_ver(g2["T"], g2["source"], source_cov=Cp)
    ref, bound, _ = reference(restated, "plane")
    assert np.all(np.abs(np.concatenate([H[gc.TRIU], g, [e2]]) - ref) <= bound)
    Hk, gk, e2k = reg.calc_H_g_e2(g2["T"], g2["source"], source_cov=Cp)
    assert np.all(np.abs(np.concatenate([Hk[gc.TRIU], gk, [e2k]]) - ref) <= bound)
    assert reg.last_correspondences == 1823


# ----------------------------------------------------------------------------- 4. gate
@pytest.fixture(scope="module")
def case():
    target, scan, T_true = gc.align_case()
    for a in (target, scan, T_true):
        a.setflags(write=False)
    return target, scan, T_true


def test_gate(case, orc):
    """T = I, max_dist = 0.1: 45.2 % kept, none within 1e-3 relative of the gate: the count equals the restated mask."""
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.GICP(max_dist=0.1, k=10)
    reg.set_target(target)
    dist = reg.kdtree.query(orc.transform(np.eye(4), scan))[0]
    assert np.min(np.abs(dist / np.float32(0.1) - 1.0)) > 1e-3
    kept = int((dist < np.float32(0.1)).sum())
    assert abs(kept / len(scan) - 0.452) < 0.005, kept / len(scan)
    reg.calc_H_g_e2(np.eye(4), scan)
    assert reg.last_correspondences == kept


# ----------------------------------------------------------------------------- 5. align
@pytest.mark.parametrize("max_dist", [2.0, 0.15])
def test_align(capi, case, max_dist):
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.math_tools import plus
    target, scan, T_true = case
    reg = pcr.GICP(max_dist=max_dist, k=10)
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
    # every trace row's sums are the bits pcr_gicp_linearize returns at that row's pose
    dev = reg._gicp_scan(scan, None)
    T2, iters2, trace = capi.gicp_align(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, max_dist, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(capi.gicp_linearize(reg._target, dev, row[:16], max_dist), row[16:])
    # max_iter = 0 returns init_T
    T0 = plus(np.eye(4), np.array([0.01, 0.02, 0.03, 0.001, 0.002, 0.003]))
    reg0 = pcr.GICP(max_dist=max_dist, k=10, max_iter=0)
    reg0.set_target(target)
    assert np.array_equal(reg0.align(scan, init_T=T0), T0) and reg0.last_iterations == 0


def test_align_device_memory_is_stable(capi, ctx, case):
    import torch
    import point_cloud_registration_amd as pcr
    target, scan, _ = case
    reg = pcr.GICP(max_dist=2.0, k=10)
    reg.set_target(target)
    first = reg.align(scan); pygc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        last = reg.align(scan)
    pygc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
    assert np.array_equal(first, last)


# ----------------------------------------------------------------------------- 6. neighbours undisturbed
def test_neighbours_undisturbed(capi, ctx, g2):
    """ICP / PlaneICP return the same bits before and after a GICP pass: over one context and the same scan array, and --
    under the search + reduce pipeline, where a scan keeps its matches -- over the very same device scan."""
    import point_cloud_registration_amd as pcr
    T, src, tgt, md = g2["T"], g2["source"], g2["target"], float(g2["max_dist"])
    icp, plane, gicp = pcr.ICP(max_dist=md), pcr.PlaneICP(max_dist=md), pcr.GICP(max_dist=md)
    icp.set_target(tgt)
    plane.set_target(tgt, kdree=object(), norm=g2["plane_normals"])
    gicp.set_target(tgt)
    for variant in (2, 1):
        with ctx.pipeline(variant=variant):
            before = [reg.calc_H_g_e2(T, src) for reg in (icp, plane)]
            gicp.calc_H_g_e2(T, src)
            after = [reg.calc_H_g_e2(T, src) for reg in (icp, plane)]
            for b, a in zip(before, after):
                assert all(np.array_equal(x, y) for x, y in zip(b, a))
            s = capi.Scan(ctx, src)
            s.estimate_covariances(10, want=False)
            o1 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g1 = capi.gicp_linearize(gicp._target, s, T, md)
            o2 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g2_ = capi.gicp_linearize(gicp._target, s, T, md)
            assert np.array_equal(o1, o2) and np.array_equal(g1, g2_) and g1[28] == o1[28]
