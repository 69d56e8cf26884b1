"""Radius and hybrid neighbourhoods (csrc/ball_moments.hip) on the GPU against the NumPy restatement of tests/ball_cases.py.

  count        equal everywhere, no tolerance
  mean, cov    of pcr_target_ball_moments within count * 2^-53 * sum|term| of the restatement (``bound_mean`` / ``bound_cov``
               there: the library sums in another set-determined order about another anchor; the compiler may contract the
               products, so bit equality is not asked)
  normals      exactly zero where count < 3; elsewhere |cos| >= 1 - 1e-6 against the restated eigenvector, except at the fragile
               points (l1 - l0 < 1e-6 l2), at most 1 % of a case
  covariances  through mode / eps within float32 rounding of the restated finish (plus what the bound on the moments allows)
  the plumbing PlaneICP(normal_radius=), SymmetricICP(radius=), GICP(radius=) against the same estimates handed in, bit for bit
  the case the unit exists for: estimate_normals(lidar_sweep(100_000), radius=1.0) against the analytic normals
"""

import ctypes

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd.synthetic import lidar_normals, lidar_sweep

import ball_cases as bc
from test_gpu_parity import capi, ctx, orc  # noqa: F401

pytestmark = pytest.mark.gpu

CLOUDS = ("grid", "planes", "sphere", "lidar", "duplicates", "single")
EPS = 1e-3
F32 = 2.0 ** -24          # half an ulp of float32, relative
TINY = 1e-45              # (the smallest float32 subnormal: what rounding to float32 may cost near zero)


@pytest.fixture(scope="module")
def targets(capi, ctx):
    """case -> point target: built once, shared; the estimates replace its normals and covariances, nothing else."""
    return {name: capi.Target.points(ctx, bc.cloud(name)) for name in CLOUDS}


def assert_moments(got, ref, what):
    count, mean, cov = got
    assert count.dtype == np.int64 and mean.dtype == cov.dtype == np.float64
    assert mean.shape == (len(count), 3) and cov.shape == (len(count), 6)
    assert np.array_equal(count, ref["count"]), what
    em, ec = np.abs(mean - ref["mean"]), np.abs(cov - ref["cov"])
    if len(count):
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"{what}: largest |mean - ref| / bound = {np.nanmax(np.where(ref['bound_mean'] > 0, em / ref['bound_mean'], 0)):.3g}, "
                  f"|cov - ref| / bound = {np.nanmax(np.where(ref['bound_cov'] > 0, ec / ref['bound_cov'], 0)):.3g}")
    assert np.all(em <= ref["bound_mean"]), what
    assert np.all(ec <= ref["bound_cov"]), what


def assert_normals(nrm, ref, what):
    assert nrm.dtype == np.float32 and nrm.shape == ref["normal"].shape
    none = ref["count"] < 3
    assert not nrm[none].any(), what
    ok = ~none & ~ref["fragile"]
    cos = np.abs(np.sum(nrm[ok].astype(np.float64) * ref["normal"][ok], axis=1))
    if ok.any():
        print(f"{what}: smallest |cos| = {cos.min():.9f} over {int(ok.sum())} points, {int(ref['fragile'].sum())} fragile skipped")
    assert np.all(cos >= 1.0 - 1e-6), what
    n2 = np.sum(nrm[~none].astype(np.float64) ** 2, axis=1)
    assert np.all(np.abs(n2 - 1.0) <= 1e-6), what             # (unit vectors at the fragile points too)


def assert_covariances(got, ref, mode, what):
    assert got.dtype == np.float32 and got.shape == ref["cov"].shape
    want, ok = bc.cov_finish(ref, mode, EPS)
    if mode == bc.COV_RAW:
        tol = F32 * np.abs(want) + (1.0 + F32) * ref["bound_cov"] + TINY
    else:
        # an eigenvector that turns by theta moves every n_i n_j by at most 2 theta
        zero = ~np.any(ref["cov"] != 0.0, axis=1)
        theta = np.where(zero, 0.0, bc.angle_bound(ref))
        tol = F32 * np.abs(want) + (2.0 * theta)[:, None] + TINY
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err[ok] <= tol[ok]), what
    assert np.all(np.isfinite(got)), what


# ---- the seam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLOUDS)
def test_moments_equal_the_restatement(orc, targets, name):
    t = targets[name]
    for r in bc.CASES[name][1]:
        for m in bc.MAX_NN:
            ref = bc.case_ref(orc, name, r, m)
            bc.assert_cap(ref, name)
            got = t.ball_moments(r, m)
            assert_moments(got, ref, f"{name} r={r} max_nn={m}")
            again = t.ball_moments(r, m)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
            if m == 0 and len(ref["set_id"]) > 1:
                # the radius set: equal sets, equal bits
                order = np.argsort(ref["set_id"], kind="stable")
                same = ref["set_id"][order][1:] == ref["set_id"][order][:-1]
                for a in got[1:]:
                    bits = a.view(np.uint64)[order]
                    assert np.all(bits[1:][same] == bits[:-1][same])


def test_max_nn_none_is_the_whole_ball(targets):
    t = targets["sphere"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(t.ball_moments(0.5), t.ball_moments(0.5, 0)))
    count, mean, cov = pcr.ball_moments(bc.cloud("sphere"), 0.5, max_nn=17)
    c2, m2, v2 = t.ball_moments(0.5, 17)
    assert cov.shape == (len(count), 3, 3) and np.array_equal(count, c2) and np.array_equal(mean, m2)
    assert np.array_equal(cov, bc.full3(v2))


def test_empty_and_refused_clouds(capi, ctx, orc):
    t = capi.Target.points(ctx, bc.cloud("empty"))
    for m in (0, 3, 17):
        count, mean, cov = t.ball_moments(1.0, m)
        assert count.shape == (0,) and mean.shape == (0, 3) and cov.shape == (0, 6)
        assert t.estimate_normals_radius(1.0, m).shape == (0, 3) and t.estimate_covariances_radius(1.0, m).shape == (0, 6)
        s = capi.Scan(ctx, bc.cloud("empty"), flags=capi.FLAG_KEEP_ORDER)
        assert s.estimate_normals_radius(1.0, m).shape == (0, 3) and s.estimate_covariances_radius(1.0, m).shape == (0, 6)
    # a point with a non-finite coordinate never reaches the kernel: no index is built over such a cloud (the restatement
    # gives it the empty set, tests/test_ball_cases.py)
    assert bc.case_ref(orc, "nan", 0.5, 0)["count"][17] == 0
    with pytest.raises(ValueError, match="non-finite"):
        capi.Target.points(ctx, bc.cloud("nan"))


# ---- normals and covariances ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLOUDS)
def test_normals_equal_the_restatement(capi, ctx, orc, targets, name):
    t = targets[name]
    scan = capi.Scan(ctx, bc.cloud(name), flags=capi.FLAG_KEEP_ORDER)
    for r in bc.CASES[name][1]:
        for m in bc.MAX_NN:
            ref = bc.case_ref(orc, name, r, m)
            what = f"{name} r={r} max_nn={m}"
            nrm, cnt = t.estimate_normals_radius(r, m, want_counts=True)
            assert cnt.dtype == np.int64 and np.array_equal(cnt, ref["count"]), what
            assert_normals(nrm, ref, what)
            assert np.array_equal(t.get_normals(), nrm)                      # what PlaneICP, SymmetricICP and ColoredICP read
            assert t.estimate_normals_radius(r, m).tobytes() == nrm.tobytes()
            t.estimate_normals_radius(r, m, want=False)
            assert np.array_equal(t.get_normals(), nrm)
            # the scan's entry point: its own index, another order of the sums
            snrm, scnt = scan.estimate_normals_radius(r, m, want_counts=True)
            assert np.array_equal(scnt, ref["count"]), what
            assert_normals(snrm, ref, what + " (scan)")
            assert np.array_equal(scan.get_normals(), snrm)


@pytest.mark.parametrize("mode", [bc.COV_PLANE, bc.COV_RAW])
@pytest.mark.parametrize("name", CLOUDS)
def test_covariances_equal_the_restated_finish(capi, ctx, orc, targets, name, mode):
    t = targets[name]
    scan = capi.Scan(ctx, bc.cloud(name), flags=capi.FLAG_KEEP_ORDER)
    for r in bc.CASES[name][1]:
        for m in bc.MAX_NN:
            ref = bc.case_ref(orc, name, r, m)
            what = f"{name} r={r} max_nn={m} mode={mode}"
            cov, cnt = t.estimate_covariances_radius(r, m, mode, EPS, want_counts=True)
            assert np.array_equal(cnt, ref["count"]), what
            assert_covariances(cov, ref, mode, what)
            assert np.array_equal(t.get_covariances(), cov)                  # what GICP reads
            assert t.estimate_covariances_radius(r, m, mode, EPS).tobytes() == cov.tobytes()
            scov, scnt = scan.estimate_covariances_radius(r, m, mode, EPS, want_counts=True)
            assert np.array_equal(scnt, ref["count"]), what
            assert_covariances(scov, ref, mode, what + " (scan)")
            assert np.array_equal(scan.get_covariances(), scov)


def test_one_member_is_the_knn_estimate_at_k_1(capi, ctx, targets):
    """A set of one member: the zero covariance, finished as pcr_target_estimate_covariances(k = 1) finishes it."""
    t = targets["sphere"]
    for mode in (bc.COV_PLANE, bc.COV_RAW):
        assert np.array_equal(t.estimate_covariances_radius(1e-4, None, mode, EPS), t.estimate_covariances(1, mode, EPS))
        assert np.array_equal(t.estimate_covariances_radius(0.5, 1, mode, EPS), t.estimate_covariances(1, mode, EPS))


def test_heavy_index_form(capi, ctx, orc, monkeypatch):
    """PCR_HEAVY is read at every index build: the heavy-cell form orders the cells otherwise, the sets stay what they are."""
    monkeypatch.setenv("PCR_HEAVY", "1")
    t = capi.Target.points(ctx, bc.cloud("lidar"))
    monkeypatch.setenv("PCR_HEAVY", "0")
    plain = capi.Target.points(ctx, bc.cloud("lidar"))
    monkeypatch.delenv("PCR_HEAVY")
    assert t.index_info()["heavy"] and not plain.index_info()["heavy"]
    for r in bc.CASES["lidar"][1]:
        for m in bc.MAX_NN:
            ref = bc.case_ref(orc, "lidar", r, m)
            for tt, form in ((t, "heavy"), (plain, "plain")):
                assert_moments(tt.ball_moments(r, m), ref, f"lidar ({form}) r={r} max_nn={m}")
                assert_normals(tt.estimate_normals_radius(r, m), ref, f"lidar ({form}) r={r} max_nn={m}")
            if m:       # the list order does not depend on the index: the same bits
                assert all(a.tobytes() == b.tobytes() for a, b in zip(t.ball_moments(r, m), plain.ball_moments(r, m)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(capi, ctx, targets):
    L = capi.lib()
    pts = bc.cloud("sphere")
    n = len(pts)
    t = targets["sphere"]
    vox = capi.Target.voxels(ctx, pts, 1.0, min_points=1)
    keep = capi.Scan(ctx, pts, flags=capi.FLAG_KEEP_ORDER)
    plain = capi.Scan(ctx, pts)
    I, D3, D6 = np.full(n, -7, np.int64), np.full((n, 3), -7.0), np.full((n, 6), -7.0)
    F3, F6 = np.full((n, 3), -7, np.float32), np.full((n, 6), -7, np.float32)
    p = capi._ptr
    before = t.estimate_normals_radius(0.5)
    bad = [(r, 0) for r in (-1.0, -1e-30, float("nan"), float("inf"))] + [(0.5, -1), (0.5, 65)]
    calls = []
    for r, m in bad:
        calls += [lambda r=r, m=m: L.pcr_target_ball_moments(t.handle, r, m, I, D3, D6),
                  lambda r=r, m=m: L.pcr_target_estimate_normals_radius(t.handle, r, m, p(F3), p(I)),
                  lambda r=r, m=m: L.pcr_scan_estimate_normals_radius(keep.handle, r, m, p(F3), p(I)),
                  lambda r=r, m=m: L.pcr_target_estimate_covariances_radius(t.handle, r, m, capi.COV_PLANE, EPS, p(F6), p(I)),
                  lambda r=r, m=m: L.pcr_scan_estimate_covariances_radius(keep.handle, r, m, capi.COV_PLANE, EPS, p(F6), p(I))]
    # NULL handles, a voxel target, a bad mode / eps, a scan that does not know the caller's order where an output is asked for
    calls += [lambda: L.pcr_target_ball_moments(None, 0.5, 0, I, D3, D6),
              lambda: L.pcr_target_estimate_normals_radius(None, 0.5, 0, p(F3), p(I)),
              lambda: L.pcr_scan_estimate_normals_radius(None, 0.5, 0, p(F3), p(I)),
              lambda: L.pcr_target_estimate_covariances_radius(None, 0.5, 0, capi.COV_PLANE, EPS, p(F6), p(I)),
              lambda: L.pcr_scan_estimate_covariances_radius(None, 0.5, 0, capi.COV_PLANE, EPS, p(F6), p(I)),
              lambda: L.pcr_target_ball_moments(vox.handle, 0.5, 0, I, D3, D6),
              lambda: L.pcr_target_estimate_normals_radius(vox.handle, 0.5, 0, p(F3), p(I)),
              lambda: L.pcr_target_estimate_covariances_radius(vox.handle, 0.5, 0, capi.COV_PLANE, EPS, p(F6), p(I)),
              lambda: L.pcr_target_estimate_covariances_radius(t.handle, 0.5, 0, 7, EPS, p(F6), p(I)),
              lambda: L.pcr_target_estimate_covariances_radius(t.handle, 0.5, 0, capi.COV_PLANE, 0.0, p(F6), p(I)),
              lambda: L.pcr_scan_estimate_covariances_radius(keep.handle, 0.5, 0, capi.COV_PLANE, 2.0, p(F6), p(I)),
              lambda: L.pcr_scan_estimate_normals_radius(plain.handle, 0.5, 0, p(F3), None),
              lambda: L.pcr_scan_estimate_normals_radius(plain.handle, 0.5, 0, None, p(I)),
              lambda: L.pcr_scan_estimate_covariances_radius(plain.handle, 0.5, 0, capi.COV_PLANE, EPS, p(F6), None)]
    for i, call in enumerate(calls):
        assert call() == capi.PCR_ERR_INVALID, i
        assert L.pcr_last_error()
    for a in (I, D3, D6, F3, F6):
        assert np.all(a == -7)
    assert np.array_equal(t.get_normals(), before)           # a refused call leaves the target's normals too
    # the wrappers refuse before the library does
    for r, m in bad + [(None, 3)]:
        with pytest.raises(ValueError):
            t.ball_moments(r, m)
    # no output asked: any scan will do
    plain.estimate_normals_radius(0.5, 3, want=False)
    plain.estimate_covariances_radius(0.5, want=False)
    with pytest.raises(ValueError):
        plain.get_normals()


# ---- the plumbing -----------------------------------------------------------------------------------------------------------
def pose():
    T = np.eye(4)
    T[:3, :3] = pcr.expSO3(np.array([0.01, -0.02, 0.015]))
    T[:3, 3] = [0.02, -0.01, 0.03]
    return T


def same_sums(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("max_nn", [None, 16, 30])
def test_plane_icp_takes_its_normals_from_the_ball(max_nn):
    tgt, src = bc.cloud("planes"), np.ascontiguousarray(bc.cloud("planes")[::3] + np.float32(0.004))
    r = 0.35
    a = pcr.PlaneICP(max_dist=0.5, normal_radius=r, normal_max_nn=max_nn)
    a.set_target(tgt)
    nrm = pcr.estimate_normals(tgt, radius=r, max_nn=max_nn)
    assert np.array_equal(a.normal, nrm)
    b = pcr.PlaneICP(max_dist=0.5)
    b.set_target(tgt, pcr.KDTree(tgt), norm=nrm)
    got, want = a.calc_H_g_e2(pose(), src), b.calc_H_g_e2(pose(), src)
    assert same_sums(got, want) and a.last_correspondences == b.last_correspondences > 100
    knn = pcr.PlaneICP(max_dist=0.5)
    knn.set_target(tgt)
    assert not same_sums(got, knn.calc_H_g_e2(pose(), src))                  # (and not the k nearest neighbours')


@pytest.mark.parametrize("max_nn", [None, 30])
def test_symmetric_icp_takes_both_normals_from_the_ball(capi, ctx, max_nn):
    tgt, src = bc.cloud("planes"), np.ascontiguousarray(bc.cloud("planes")[::3] + np.float32(0.004))
    r = 0.35
    a = pcr.SymmetricICP(max_dist=0.5, radius=r, max_nn=max_nn)
    a.set_target(tgt)
    nq = pcr.estimate_normals(tgt, radius=r, max_nn=max_nn)
    np_ = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_normals_radius(r, max_nn)
    assert np.array_equal(a.normal, nq) and np.array_equal(a.source_normals(src), np_)
    b = pcr.SymmetricICP(max_dist=0.5)
    b.set_target(tgt, norm=nq)
    assert same_sums(a.calc_H_g_e2(pose(), src), b.calc_H_g_e2(pose(), src, source_normals=np_))
    assert a.last_correspondences == b.last_correspondences > 100


@pytest.mark.parametrize("regularization", ["plane", "raw"])
def test_gicp_takes_both_covariances_from_the_ball(capi, ctx, regularization):
    tgt, src = bc.cloud("planes"), np.ascontiguousarray(bc.cloud("planes")[::3] + np.float32(0.004))
    r, m = 0.35, 30
    mode = {"plane": capi.COV_PLANE, "raw": capi.COV_RAW}[regularization]
    a = pcr.GICP(max_dist=0.5, radius=r, max_nn=m, regularization=regularization)
    a.set_target(tgt)
    cq = capi.Target.points(ctx, tgt).estimate_covariances_radius(r, m, mode, a.eps)
    cp = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances_radius(r, m, mode, a.eps)
    assert np.array_equal(a.covariance, cq) and np.array_equal(a.source_covariance(src), cp)
    b = pcr.GICP(max_dist=0.5, regularization=regularization)
    b.set_target(tgt, cov=cq)
    assert same_sums(a.calc_H_g_e2(pose(), src), b.calc_H_g_e2(pose(), src, source_cov=cp))
    assert a.last_correspondences == b.last_correspondences > 100
    v = pcr.VGICP(voxel_size=1.0, max_dist=1.0, radius=r, max_nn=m, regularization=regularization)
    v.set_target(tgt)
    assert np.array_equal(v.source_covariance(src), cp)


def test_a_cached_scan_is_estimated_again_for_another_neighbourhood(capi, ctx):
    """Two aligners that share an uploaded scan (pcr.UploadedScan is not needed: the cache is the aligner's own, keyed by the
    array; here ONE aligner changes its neighbourhood, which is what the key has to see)."""
    tgt, src = bc.cloud("planes"), np.ascontiguousarray(bc.cloud("planes")[::3] + np.float32(0.004))
    g = pcr.GICP(max_dist=0.5, k=10)
    g.set_target(tgt)
    knn = g.source_covariance(src)
    scan = g._scan
    assert np.array_equal(knn, capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances(10, capi.COV_PLANE, g.eps))
    ball = pcr.GICP(max_dist=0.5, k=10, radius=0.35, max_nn=30)
    ball.set_target(tgt)
    ball._scan, ball._scan_key = g._scan, g._scan_key                       # the scan that served the k = 10 aligner
    got = ball.source_covariance(src)
    assert ball._scan is scan                                               # (the same device copy: no second upload)
    want = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances_radius(0.35, 30, capi.COV_PLANE, ball.eps)
    assert np.array_equal(got, want) and not np.array_equal(got, knn)
    assert np.array_equal(g.source_covariance(src), knn)                     # and back: estimated again from the k nearest
    ball._scan = None                                                       # (one owner closes it)
    s = pcr.SymmetricICP(max_dist=0.5, k=10)
    s.set_target(tgt)
    n_knn = s.source_normals(src)
    s2 = pcr.SymmetricICP(max_dist=0.5, k=10, radius=0.35)
    s2.set_target(tgt)
    s2._scan, s2._scan_key = s._scan, s._scan_key
    assert s2._symm_scan(src, None) is s._scan
    assert np.array_equal(s._scan.get_normals(), capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_normals_radius(0.35))
    assert not np.array_equal(s._scan.get_normals(), n_knn)
    s2._scan = None


# ---- the case the unit exists for -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    pts = lidar_sweep(100_000, seed=0)
    return pts, lidar_normals(pts).astype(np.float64)


def share(nrm, analytic):
    return float(np.mean(np.abs(np.sum(nrm.astype(np.float64) * analytic, axis=1)) > 0.95))


@pytest.mark.parametrize("max_nn", [None, 30])
def test_lidar_sweep_normals(sweep, max_nn):
    pts, analytic = sweep
    nrm, cnt = pcr.estimate_normals(pts, radius=1.0, max_nn=max_nn, return_counts=True)
    knn = pcr.estimate_normals(pts, k=15)
    got = share(nrm, analytic)
    print(f"lidar_sweep(100 000): |cos| > 0.95 to the analytic normal at {got:.4f} of the points with radius 1.0 m, max_nn {max_nn} "
          f"(counts {cnt.min()} .. {cnt.max()}, mean {cnt.mean():.1f}); at {share(knn, analytic):.4f} with k = 15")
    assert cnt.min() >= 3
    assert cnt.max() <= (max_nn or len(pts))
    assert got >= 0.98
