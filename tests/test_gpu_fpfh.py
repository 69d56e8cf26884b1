"""FPFH descriptors and exact feature matching on the GPU (csrc/fpfh.hip) against the NumPy restatement of
tests/fpfh_cases.py: SPFH counts and k equal, FPFH within one float32 ulp (the float64 sums differ in order only), the
matches bit-equal -- on every point the restatement does not exclude as fragile, under its 1 % cap."""

import numpy as np
import pytest

import point_cloud_registration_amd as pcr

import fpfh_cases as fc
from radius_cases import radius_ref_f32
from test_gpu_parity import capi, ctx, orc  # noqa: F401

pytestmark = pytest.mark.gpu

BLOCK_SUM_TOL = 33 * 2.0 ** -23 * 200


@pytest.fixture(scope="module")
def targets(capi, ctx):
    """named cloud -> point target with the cloud's normals: built once, shared and left unchanged."""
    return {name: capi.Target.points(ctx, fc.cloud(name)[0], fc.cloud(name)[1]) for name in fc.CLOUDS}


def assert_spfh(got, ref, cap_name=None):
    counts, k = got
    assert counts.dtype == np.uint32 and k.dtype == np.int64 and counts.shape == (len(k), 33)
    if cap_name:
        fc.assert_cap(ref, cap_name)
    ok = ~ref["excluded"]
    assert np.array_equal(counts[ok], ref["counts"][ok]) and np.array_equal(k[ok], ref["k"][ok])
    assert np.array_equal(k, ref["k"])                                   # (membership is never fragile)
    assert np.array_equal(counts.reshape(-1, 3, 11).sum(axis=2), np.repeat(k[:, None], 3, axis=1).astype(np.uint32))


def assert_fpfh(G, ref, name):
    assert G.dtype == np.float32 and G.shape == ref["fpfh"].shape
    ok = ~ref["excluded"]
    R32 = ref["fpfh"].astype(np.float32)
    ulp = np.spacing(np.abs(R32))
    diff = np.abs(G.astype(np.float64) - R32.astype(np.float64))
    exact = float(np.mean(G[ok] == R32[ok])) if ok.any() else 1.0
    print(f"{name}: largest |G - fl32(R)| / ulp {float(np.max(diff[ok] / ulp[ok])) if ok.any() else 0.0:.3g}, exactly equal {exact:.6f}")
    assert np.all(diff[ok] <= ulp[ok])
    assert exact >= 0.999
    sums = G.astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    k = ref["k"]
    assert np.all(np.abs(sums[k > 0] - 200.0) <= BLOCK_SUM_TOL) and np.all(G[k == 0] == 0)


# ---- the named clouds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "second"])
def test_spfh_counts_equal_the_restatement(orc, targets, name):
    ref = fc.cloud_ref(orc, name)
    assert_spfh(targets[name].spfh(fc.cloud(name)[2]), ref, cap_name=name)
    if name == "main":
        assert not np.any(ref["excluded"])                               # here: every point is compared


@pytest.mark.parametrize("name", ["main", "second"])
def test_fpfh_within_one_ulp(orc, targets, name):
    ref = fc.cloud_ref(orc, name)
    fc.assert_cap(ref, name)
    G, k = targets[name].fpfh(fc.cloud(name)[2], want_k=True)
    assert k.dtype == np.int64 and np.array_equal(k, ref["k"])
    assert_fpfh(G, ref, name)
    assert np.array_equal(G, targets[name].fpfh(fc.cloud(name)[2]))      # (without k: the same rows)


# ---- edges ----------------------------------------------------------------------------------------------------------------
def cluster(n, seed=21):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32), fc._unit32(rng.normal(size=(n, 3)))


def check_cloud(capi, orc, ctx, pts, nrm, r, name):
    ref = fc.fpfh_ref(orc, pts, nrm, r)
    t = capi.Target.points(ctx, pts, nrm)
    assert_spfh(t.spfh(r), ref)
    assert_fpfh(t.fpfh(r), ref, name)
    return ref


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_sizes_around_one_block(capi, orc, ctx, n):
    pts, nrm = cluster(n)
    ref = check_cloud(capi, orc, ctx, pts, nrm, 0.4, f"n={n}")
    assert np.sum(ref["excluded"]) <= n // 10
    if n >= 63:
        assert ref["k"].mean() > 5


def test_radius_zero(targets):
    counts, k = targets["main"].spfh(0.0)
    assert not counts.any() and not k.any()
    F, k = targets["main"].fpfh(0.0, want_k=True)
    assert F.shape == (2048, 33) and not F.any() and not k.any()


def test_duplicates_and_isolated_points(capi, orc, ctx):
    """Exact duplicates (d2 == 0) are no neighbours, on either pass; points with nobody within r give zero rows."""
    pts, nrm = cluster(100)
    other = fc._unit32(np.random.default_rng(22).normal(size=(20, 3)))
    far = np.float32([[30, 0, 0], [0, -40, 0], [0, 0, 50], [30, 0, 0]])  # (the last: a duplicate pair with nobody else around)
    pts = np.vstack([pts, pts[:20], far])
    nrm = np.vstack([nrm, other, np.tile(np.float32([0, 1, 0]), (4, 1))])
    ref = check_cloud(capi, orc, ctx, pts, nrm, 0.4, "duplicates")
    k = capi.Target.points(ctx, pts, nrm).spfh(0.4)[1]
    found = np.diff(radius_ref_f32(orc, pts, pts, 0.4)[2])               # what the radius search finds: self and duplicates included
    coincident = np.where(np.arange(len(pts)) < 20, 2, 1)
    coincident[100:120] = 2
    coincident[[120, 123]] = 2
    assert np.array_equal(k, found - coincident)
    assert np.all(k[120:] == 0) and np.all(ref["fpfh"][120:] == 0)
    assert np.array_equal(ref["k"][:20], ref["k"][100:120])              # a point and its duplicate: the same neighbours


def test_three_points_and_the_parallel_rule(capi, orc, ctx):
    """p = (0,0,0), q = (0,0,1), s = (1,0,0), all normals (0,0,1): d parallel to n1 between p and q gives alpha = theta = 0.
    Every pair is an exact role tie, which the strict rule settles (no swap) -- all arithmetic here is exact, so the counts are
    compared on every point, whatever the restatement marks."""
    pts = np.float32([[0, 0, 0], [0, 0, 1], [1, 0, 0]])
    nrm = np.tile(np.float32([0, 0, 1]), (3, 1))
    ref = fc.fpfh_ref(orc, pts, nrm, 1.5)
    t = capi.Target.points(ctx, pts, nrm)
    counts, k = t.spfh(1.5)
    assert k.tolist() == [2, 2, 2] and np.array_equal(counts, ref["counts"])
    want_p = np.zeros(33, np.uint32)
    want_p[[5, 11 + 10, 11 + 5, 22 + 5]] = [2, 1, 1, 2]
    assert np.array_equal(counts[0], want_p)
    F = t.fpfh(1.5)
    R32 = ref["fpfh"].astype(np.float32)
    assert np.all(np.abs(F.astype(np.float64) - R32) <= np.spacing(np.abs(R32)))
    counts, k = t.spfh(1.2)                                              # q and s are sqrt 2 apart
    assert k.tolist() == [2, 1, 1] and np.array_equal(counts, fc.fpfh_ref(orc, pts, nrm, 1.2)["counts"])


def test_zero_normal(capi, orc, ctx):
    """One normal is (0, 0, 0): as n1 it gives v . v == 0, as n2 an atan2(+-0, +-0) the restatement marks fragile."""
    pts, nrm = cluster(100, seed=23)
    pts[0] = [0.5, 0.5, 0.5]                                            # in a corner: few neighbours to exclude with it
    nrm = nrm.copy()
    nrm[0] = 0
    ref = check_cloud(capi, orc, ctx, pts, nrm, 0.4, "zero normal")
    assert ref["k"][0] > 0 and np.sum(~ref["excluded"]) >= 50


def test_refusals_of_the_library(capi, ctx, targets):
    L = capi.lib()
    pts = fc.cloud("main")[0]
    counts, k, F = np.zeros((2048, 33), np.uint32), np.zeros(2048, np.int64), np.zeros((2048, 33), np.float32)
    bare = capi.Target.points(ctx, pts)
    assert L.pcr_target_spfh(bare.handle, 0.5, counts, k) == capi.PCR_ERR_NO_TARGET
    assert L.pcr_target_fpfh(bare.handle, 0.5, F, None) == capi.PCR_ERR_NO_TARGET
    with pytest.raises(ValueError, match="normals"):
        bare.fpfh(0.5)
    bare.set_normals(fc.cloud("main")[1])                                # pcr_target_set_normals supplies them
    assert np.array_equal(bare.spfh(fc.MAIN_R)[0], targets["main"].spfh(fc.MAIN_R)[0])
    vox = capi.Target.voxels(ctx, np.random.default_rng(3).uniform(-2, 2, (5000, 3)).astype(np.float32), 1.0)
    assert L.pcr_target_spfh(vox.handle, 0.5, counts, k) == capi.PCR_ERR_INVALID
    assert L.pcr_target_fpfh(vox.handle, 0.5, F, None) == capi.PCR_ERR_INVALID
    for r in (-1.0, np.nan, np.inf):
        assert L.pcr_target_spfh(targets["main"].handle, r, counts, k) == capi.PCR_ERR_INVALID
        assert L.pcr_target_fpfh(targets["main"].handle, r, F, None) == capi.PCR_ERR_INVALID
    a = np.zeros((4, 70), np.float32)
    idx, d = np.zeros(4, np.int64), np.zeros(4, np.float32)
    for dim in (0, 65, -1):
        assert L.pcr_feature_match(ctx.handle, a, 4, a, 4, dim, idx, d, d.copy()) == capi.PCR_ERR_INVALID
    assert not counts.any() and not F.any()


# ---- order and repeatability ----------------------------------------------------------------------------------------------
def test_order_and_repeatability(capi, ctx, targets):
    pts, nrm, r = fc.cloud("main")
    counts, k = targets["main"].spfh(r)
    perm = np.random.default_rng(31).permutation(len(pts))
    pc, pk = capi.Target.points(ctx, pts[perm], nrm[perm]).spfh(r)
    assert np.array_equal(pc, counts[perm]) and np.array_equal(pk, k[perm])
    F = targets["main"].fpfh(r)
    assert np.array_equal(F, targets["main"].fpfh(r)) and np.array_equal(counts, targets["main"].spfh(r)[0])


def test_non_interference(capi, ctx):
    """KDTree.query_radius and PlaneICP on the same context return the same bits before and after an FPFH call."""
    pts, nrm, r = fc.cloud("second")
    tree = pcr.KDTree(pts)
    picp = pcr.PlaneICP(max_dist=1.0, k=10)
    picp.set_target(pts)
    scan = fc.cloud("main")[0]
    T = np.eye(4); T[:3, 3] = [0.01, -0.02, 0.015]
    before_r, before_p = tree.query_radius(scan, 0.3), picp.calc_H_g_e2(T, scan)
    F = pcr.compute_fpfh(pts, nrm, radius=r)
    pcr.match_features(F[:500], F[500:1000])
    after_r, after_p = tree.query_radius(scan, 0.3), picp.calc_H_g_e2(T, scan)
    for a, b in zip(before_r + tuple(before_p), after_r + tuple(after_p)):
        assert np.array_equal(a, b)
    assert len(before_r[0]) > 0 and np.any(before_p[0] != 0)


# ---- matching -------------------------------------------------------------------------------------------------------------
def assert_match(capi, ctx, A, B):
    got, want = capi.feature_match(ctx, A, B), fc.match_ref(A, B)
    assert got[0].dtype == np.int64 and got[1].dtype == got[2].dtype == np.float32
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return got


# rows of B go through LDS 64 at a time and are split over blockIdx.y in chunks of at least two tiles: (1000, 1500) runs
# 12 splits of two tiles each, (65, 257) two splits of three and two tiles (the last one of a single row), (63, 65) one split
# of two tiles
@pytest.mark.parametrize("dim", [1, 33, 64])
@pytest.mark.parametrize("na, nb", [(1000, 1500), (1, 1), (63, 65), (64, 64), (65, 257), (257, 1)])
def test_match_equals_the_restatement(capi, ctx, na, nb, dim):
    rng = np.random.default_rng(1000 * dim + na + nb)
    A, B = rng.uniform(0, 10, (na, dim)).astype(np.float32), rng.uniform(0, 10, (nb, dim)).astype(np.float32)
    idx, d1, d2 = assert_match(capi, ctx, A, B)
    assert np.all((idx >= 0) & (idx < nb)) and np.all(d1 <= d2)
    if nb == 1:
        assert np.all(np.isinf(d2)) and np.all(np.isfinite(d1))


@pytest.mark.parametrize("dim", [20, 33])
def test_match_planted_cases(capi, ctx, dim):
    rng = np.random.default_rng(41 + dim)
    A, B = rng.uniform(0, 10, (300, dim)).astype(np.float32), rng.uniform(0, 10, (400, dim)).astype(np.float32)
    B[390] = B[70] = B[200]                  # duplicate rows in different tiles and splits: the lowest index wins
    A[10] = B[70]
    B[[5, 130, 399]] = A[[20, 21, 22]]       # rows of A copied into B: d2 = 0
    B[64] = np.nan                           # never chosen
    idx, d1, d2 = assert_match(capi, ctx, A, B)
    assert idx[10] == 70 and d1[10] == 0 and d2[10] == 0
    assert idx[[20, 21, 22]].tolist() == [5, 130, 399] and np.all(d1[[20, 21, 22]] == 0) and np.all(d2[[20, 21, 22]] > 0)
    assert not np.any(idx == 64) and np.all(np.isfinite(d2))
    idx, d1, d2 = assert_match(capi, ctx, A, B[64:65])                     # nothing but a NaN row
    assert np.all(idx == -1) and np.all(np.isinf(d1)) and np.all(np.isinf(d2))
    # squares and sums in float32's subnormal range (nothing is flushed to zero), and sums that overflow to inf
    tiny_a, tiny_b = (A[:65] * np.float32(1e-21)).astype(np.float32), (B[:130] * np.float32(1e-21)).astype(np.float32)
    tiny_b[64] = tiny_b[3]
    idx, d1, d2 = assert_match(capi, ctx, tiny_a, tiny_b)
    assert np.count_nonzero(d1) >= 60 and np.all(d2 < np.finfo(np.float32).tiny)
    huge_b = (B[:130] * np.float32(3e18)).astype(np.float32)
    huge_b[64] = huge_b[3]
    idx, d1, d2 = assert_match(capi, ctx, tiny_a, huge_b)
    assert np.any(np.isinf(d1)) and np.all(idx >= 0)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_descriptors_survive_a_rigid_motion(orc):
    pa, na_, r = fc.cloud("main")
    pb, nb_, _ = fc.cloud("main_moved")
    Fa, Fb = pcr.compute_fpfh(pa, na_, radius=r), pcr.compute_fpfh(pb, nb_, radius=r)
    assert Fa.shape == Fb.shape == (2048, 33) and Fa.dtype == np.float32
    ia, ib, dist = pcr.match_features(Fa, Fb, mutual=True)
    share = float(np.sum(ia == ib)) / len(pa)
    print(f"mutual matches {len(ia)} of {len(pa)}, i -> i for a share of {share:.4f}, largest matched distance {float(dist.max()):.3g}")
    assert ia.dtype == ib.dtype == np.int64 and dist.dtype == np.float32 and np.all(np.diff(ia) > 0)
    assert share >= 0.99
    # estimated normals (normals=None) run the same path
    Fe = pcr.compute_fpfh(fc.cloud("second")[0], radius=fc.SECOND_R)
    k = fc.cloud_ref(orc, "second")["k"]
    sums = Fe.astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.all(np.abs(sums[k > 0] - 200.0) <= BLOCK_SUM_TOL) and np.all(Fe[k == 0] == 0)
