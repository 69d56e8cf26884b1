"""ISS keypoints (csrc/keypoints.hip) and FPFH at chosen rows (k_fpfh_rows of csrc/fpfh.hip) on the GPU against the NumPy
restatement of tests/iss_cases.py: k equal everywhere, eigenvalues within 1e-12 of the largest, the salient flag and the
keypoint mask equal on every point the restatement does not exclude as fragile, under its 1 % cap; equal support sets give
equal bits; the descriptors at chosen rows equal the rows of the full call bit for bit."""

import os
import subprocess
import sys

import numpy as np
import pytest

import point_cloud_registration_amd as pcr

import fpfh_cases as fc
import iss_cases as ic
from conftest import REPO
from test_gpu_parity import capi, ctx, orc  # noqa: F401

pytestmark = pytest.mark.gpu

# the two sides differ in the order of at most a few hundred float64 terms and in the eigen-solver: a few ulp of l1 each
EIG_TOL = 1e-12


@pytest.fixture(scope="module")
def targets(capi, ctx):
    """named cloud -> point target with the cloud's normals: built once, shared and left unchanged."""
    return {name: capi.Target.points(ctx, fc.cloud(name)[0], fc.cloud(name)[1]) for name in fc.CLOUDS}


def one_pattern_per_set(values, set_id):
    """Every group of points with one support set has one bit pattern in every column of ``values``."""
    if len(set_id) == 0:
        return True
    bits = np.ascontiguousarray(values, np.float64).reshape(len(set_id), -1).view(np.uint64)
    order = np.argsort(set_id, kind="stable")
    same = set_id[order][1:] == set_id[order][:-1]
    return bool(np.all(bits[order][1:][same] == bits[order][:-1][same]))


def assert_seam(got, ref, name):
    eig, sal, k = got
    assert eig.dtype == sal.dtype == np.float64 and k.dtype == np.int64 and eig.shape == (len(k), 3) and sal.shape == k.shape
    assert np.array_equal(k, ref["k"])
    l1 = ref["eig"][:, 0] if len(k) else np.zeros(0)
    err = np.abs(eig - ref["eig"]).max(axis=1) if len(k) else np.zeros(0)
    pos = l1 > 0
    ratio = float(np.max(err[pos] / l1[pos])) if pos.any() else 0.0
    print(f"{name}: largest |eig - ref| / l1 = {ratio:.3g}, salient {int(np.sum(sal > 0))} of {len(k)}, excluded {int(ref['excluded'].sum())}")
    assert np.all(err <= EIG_TOL * l1)
    assert np.all(eig[:, 0] >= eig[:, 1]) and np.all(eig[:, 1] >= eig[:, 2])
    ok = ~ref["excluded"]
    assert np.array_equal((sal > 0)[ok], ref["salient"][ok])
    assert np.array_equal(sal[sal > 0], eig[sal > 0, 2]) and np.all(sal >= 0)
    assert one_pattern_per_set(eig, ref["set_id"]) and one_pattern_per_set(sal, ref["set_id"])


def assert_mask(mask, ref):
    assert mask.dtype == bool and mask.shape == ref["keypoint"].shape
    ok = ~ref["excluded"]
    assert np.array_equal(mask[ok], ref["keypoint"][ok])


# ---- the named clouds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "second"])
def test_seam_equals_the_restatement(orc, targets, name):
    ref = ic.cloud_ref(orc, name, 0)
    ic.assert_cap(ref, name)
    assert_seam(targets[name].iss_saliency(ic.PARAMS[name][0][0]), ref, name)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", ["main", "second"])
def test_keypoints_equal_the_restatement(orc, targets, name, which):
    ref = ic.cloud_ref(orc, name, which)
    ic.assert_cap(ref, name)
    assert int(ref["keypoint"].sum()) == ic.EXPECTED[(name, which)]
    rs, rn = ic.PARAMS[name][which]
    mask, sal = targets[name].iss_keypoints(rs, rn, want_saliency=True)
    assert_mask(mask, ref)
    assert np.array_equal(sal, targets[name].iss_saliency(rs)[1])         # (the cell-sorted pass: the same bits as the seam)
    assert np.array_equal(mask, targets[name].iss_keypoints(rs, rn))
    print(f"{name} at ({rs}, {rn}): {int(mask.sum())} keypoints, the restatement {int(ref['keypoint'].sum())}, ties {int(ref['tie'].sum())}")
    rows, sal2 = pcr.iss_keypoints(fc.cloud(name)[0], rs, rn, return_saliency=True)
    assert rows.dtype == np.int64 and np.array_equal(rows, np.flatnonzero(mask)) and np.array_equal(sal2, sal)
    assert np.array_equal(pcr.iss_keypoints(fc.cloud(name)[0], rs, rn), rows)


def test_default_radii_come_from_the_resolution(capi, ctx, targets):
    pts = fc.cloud("main")[0]
    res = 2.0 * float(np.mean(targets["main"].knn_mean_distance(2), dtype=np.float64))
    rs, rn = float(np.float32(6.0 * res)), float(np.float32(4.0 * res))
    assert np.array_equal(pcr.iss_keypoints(pts), np.flatnonzero(targets["main"].iss_keypoints(rs, rn)))
    assert np.array_equal(pcr.iss_keypoints(pts, non_max_radius=0.445), np.flatnonzero(targets["main"].iss_keypoints(rs, 0.445)))


# ---- equal support sets ---------------------------------------------------------------------------------------------------
def tight_cluster():
    """Two isolated pairs around one tight cluster of 12 points (rows 2 .. 13): at radius 1 the 12 share one support set."""
    rng = np.random.default_rng(51)
    c = rng.uniform(-0.05, 0.05, (12, 3))
    return np.vstack([[[30, 0, 0], [30.01, 0, 0]], c, [[0, -40, 0], [0, -40, 0.01]]]).astype(np.float32)


def test_same_support_set_same_bits(capi, orc, ctx):
    pts = tight_cluster()
    t = capi.Target.points(ctx, pts)
    eig, sal, k = t.iss_saliency(1.0)
    assert k.tolist() == [2, 2] + [12] * 12 + [2, 2]
    assert len(set(sal[2:14].view(np.uint64).tolist())) == 1 and sal[2] > 0
    assert len({tuple(row) for row in eig[2:14].view(np.uint64).tolist()}) == 1
    assert not sal[[0, 1, 14, 15]].any()                                 # k < min_neighbors
    mask = t.iss_keypoints(1.0, 1.0)
    assert np.flatnonzero(mask).tolist() == [2]                          # the smallest original index of the cluster
    assert_mask(mask, ic.iss_ref(orc, pts, 1.0, 1.0))
    # the same cluster with its rows reversed: again the smallest original index, now another point
    back = np.ascontiguousarray(pts[::-1])
    assert np.flatnonzero(capi.Target.points(ctx, back).iss_keypoints(1.0, 1.0)).tolist() == [2]


# ---- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300])
def test_sizes_around_one_block(capi, orc, ctx, n):
    pts = ic.cluster(n)
    ref = ic.iss_ref(orc, pts, 0.4, 0.3)
    t = capi.Target.points(ctx, pts)
    assert_seam(t.iss_saliency(0.4), ref, f"n={n}")
    mask = t.iss_keypoints(0.4, 0.3)
    assert_mask(mask, ref)
    assert np.sum(ref["excluded"]) <= n // 100
    rows = pcr.iss_keypoints(pts, 0.4, 0.3)
    assert rows.dtype == np.int64 and np.array_equal(rows, np.flatnonzero(mask))
    if n >= 63:
        assert mask.sum() >= 1


def test_radius_zero(targets):
    eig, sal, k = targets["main"].iss_saliency(0.0, min_neighbors=1)
    assert np.all(k == 1) and not eig.any() and not sal.any()            # l1 == 0: never salient
    assert not targets["main"].iss_keypoints(0.0, 0.0, min_neighbors=1).any()
    assert not targets["main"].iss_keypoints(0.0, 0.445, min_neighbors=1).any()


def test_degenerate_sets(capi, orc, ctx):
    same = np.tile(np.float32([[0.25, -1.5, 3.0]]), (20, 1))
    t = capi.Target.points(ctx, same)
    eig, sal, k = t.iss_saliency(0.5)
    assert np.all(k == 20) and not eig.any() and not sal.any() and not t.iss_keypoints(0.5, 0.5).any()
    line = (np.arange(20)[:, None] * np.array([[1, 2, 3]])).astype(np.float32)
    ref = ic.iss_ref(orc, line, 12.0, 8.0)
    t = capi.Target.points(ctx, line)
    eig, sal, k = t.iss_saliency(12.0)
    assert np.array_equal(k, ref["k"]) and k.max() >= 5
    assert np.all((sal == 0) | ref["excluded"])
    assert not np.any(t.iss_keypoints(12.0, 8.0) & ~ref["excluded"])
    P = ic.cluster(100, seed=23)
    both = np.vstack([P, P])
    rows = pcr.iss_keypoints(both, 0.4, 0.3)
    assert len(rows) >= 1 and np.all(rows < len(P))                      # of a point and its duplicate, the first
    ref = ic.iss_ref(orc, both, 0.4, 0.3)
    assert_mask(capi.Target.points(ctx, both).iss_keypoints(0.4, 0.3), ref)


def test_permutation(capi, orc, ctx, targets):
    pts = fc.cloud("main")[0]
    rs, rn = ic.PARAMS["main"][0]
    ref = ic.cloud_ref(orc, "main", 0)
    _, _, k = targets["main"].iss_saliency(rs)
    mask = targets["main"].iss_keypoints(rs, rn)
    perm = np.random.default_rng(31).permutation(len(pts))
    tp = capi.Target.points(ctx, pts[perm])
    assert np.array_equal(tp.iss_saliency(rs)[2], k[perm])
    free = ~(ref["excluded"] | ref["tie"])[perm]
    assert np.array_equal(tp.iss_keypoints(rs, rn)[free], mask[perm][free])
    assert free.sum() > 0.9 * len(pts)


# ---- repeatability and non-interference -----------------------------------------------------------------------------------
def test_non_interference(capi, ctx, targets):
    """KDTree.query_radius, PlaneICP and the full FPFH call on the same context return the same bits before and after the
    keypoint and rows calls, and those return the same bits twice."""
    pts, nrm, r = fc.cloud("second")
    rs, rn = ic.PARAMS["second"][0]
    tree = pcr.KDTree(pts)
    picp = pcr.PlaneICP(max_dist=1.0, k=10)
    picp.set_target(pts)
    scan = fc.cloud("main")[0]
    T = np.eye(4); T[:3, 3] = [0.01, -0.02, 0.015]
    before = tree.query_radius(scan, 0.3) + tuple(picp.calc_H_g_e2(T, scan)) + (targets["second"].fpfh(r),)
    rows, sal = pcr.iss_keypoints(pts, rs, rn, return_saliency=True)
    F = pcr.compute_fpfh_rows(pts, rows, nrm, radius=r)
    after = tree.query_radius(scan, 0.3) + tuple(picp.calc_H_g_e2(T, scan)) + (targets["second"].fpfh(r),)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert len(before[0]) > 0 and np.any(before[3] != 0)
    rows2, sal2 = pcr.iss_keypoints(pts, rs, rn, return_saliency=True)
    assert np.array_equal(rows, rows2) and np.array_equal(sal.view(np.uint64), sal2.view(np.uint64))
    assert np.array_equal(F, pcr.compute_fpfh_rows(pts, rows, nrm, radius=r)) and np.array_equal(F, before[-1][rows])


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join({repo!r}, "tests"))
sys.path.insert(0, {repo!r})
from point_cloud_registration_amd import _capi
import fpfh_cases as fc
pts, nrm, r = fc.cloud("main")
t = _capi.Target.points(_capi.get_context(0), pts, nrm)
eig, sal, k = t.iss_saliency({rs!r})
mask = t.iss_keypoints({rs!r}, {rn!r})
rows = np.flatnonzero(mask).astype(np.int64)
np.savez({path!r}, eig=eig, sal=sal, k=k, mask=mask, F=t.fpfh(r), Frows=t.fpfh(r, rows=rows), heavy=np.array(t.index_info()["heavy"]))
"""


def test_heavy_cell_form_of_the_index(orc, tmp_path):
    """PCR_HEAVY is read once per process, so a fresh one builds the heavy-cell form of the index: another order of the
    records, the same contract."""
    rs, rn = ic.PARAMS["main"][0]
    path = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, rs=rs, rn=rn, path=path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PCR_HEAVY="1"), cwd=REPO)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = np.load(path)
    assert bool(got["heavy"])
    ref = ic.cloud_ref(orc, "main", 0)
    assert_seam((got["eig"], got["sal"], got["k"]), ref, "main, heavy cells")
    assert_mask(got["mask"], ref)
    assert np.array_equal(got["Frows"], got["F"][np.flatnonzero(got["mask"])])


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library(capi, ctx, targets):
    L = capi.lib()
    n = 2048
    h = targets["main"].handle
    eig, sal, k, mask = np.full((n, 3), 7.0), np.full(n, 7.0), np.full(n, 7, np.int64), np.full(n, 7, np.uint8)

    def both(handle, rs=0.5, rn=0.5, g21=0.975, g32=0.975, mn=5):
        a = L.pcr_target_iss_saliency(handle, rs, g21, g32, mn, eig, sal, k)
        b = L.pcr_target_iss_keypoints(handle, rs, rn, g21, g32, mn, mask, sal.ctypes.data)
        return a, b
    vox = capi.Target.voxels(ctx, np.random.default_rng(3).uniform(-2, 2, (5000, 3)).astype(np.float32), 1.0)
    assert both(vox.handle) == (capi.PCR_ERR_INVALID, capi.PCR_ERR_INVALID)
    for r in (-1.0, np.nan, np.inf):
        assert both(h, rs=r) == (capi.PCR_ERR_INVALID, capi.PCR_ERR_INVALID)
        assert L.pcr_target_iss_keypoints(h, 0.5, r, 0.975, 0.975, 5, mask, sal.ctypes.data) == capi.PCR_ERR_INVALID
    for g in (0.0, -0.5, np.nan, np.inf):
        assert both(h, g21=g) == (capi.PCR_ERR_INVALID, capi.PCR_ERR_INVALID)
        assert both(h, g32=g) == (capi.PCR_ERR_INVALID, capi.PCR_ERR_INVALID)
    for mn in (0, -3):
        assert both(h, mn=mn) == (capi.PCR_ERR_INVALID, capi.PCR_ERR_INVALID)
    assert np.all(eig == 7) and np.all(sal == 7) and np.all(k == 7) and np.all(mask == 7)
    with pytest.raises(ValueError, match="point target"):
        vox.iss_keypoints(0.5, 0.5)
    empty = capi.Target.points(ctx, np.zeros((0, 3), np.float32))
    assert both(empty.handle) == (capi.PCR_OK, capi.PCR_OK)
    # descriptors at rows: ascending, inside [0, n), and pcr_target_fpfh's own refusals
    F, kk = np.full((4, 33), 7, np.float32), np.full(4, 7, np.int64)
    for rows in ([3, 3, 4, 5], [0, 5, 2, 9], [0, 1, 2, n], [-1, 0, 1, 2]):
        assert L.pcr_target_fpfh_rows(h, 0.5, np.array(rows, np.int64), 4, F, kk.ctypes.data) == capi.PCR_ERR_INVALID
    good = np.arange(4, dtype=np.int64)
    for r in (-1.0, np.nan, np.inf):
        assert L.pcr_target_fpfh_rows(h, r, good, 4, F, None) == capi.PCR_ERR_INVALID
    assert L.pcr_target_fpfh_rows(vox.handle, 0.5, good, 4, F, None) == capi.PCR_ERR_INVALID
    bare = capi.Target.points(ctx, fc.cloud("main")[0])
    assert L.pcr_target_fpfh_rows(bare.handle, 0.5, good, 4, F, None) == capi.PCR_ERR_NO_TARGET
    assert L.pcr_target_fpfh_rows(empty.handle, 0.5, good[:1], 1, F, None) == capi.PCR_ERR_INVALID
    assert np.all(F == 7) and np.all(kk == 7)
    with pytest.raises(ValueError, match="ascending"):
        targets["main"].fpfh(0.5, rows=[4, 2])
    assert bare.iss_keypoints(0.668, 0.445).sum() == ic.EXPECTED[("main", 0)]          # (no normals needed)


# ---- FPFH at chosen rows --------------------------------------------------------------------------------------------------
def test_fpfh_rows_equal_the_full_call(targets):
    pts, nrm, r = fc.cloud("main")
    n = len(pts)
    t = targets["main"]
    F, k = t.fpfh(r, want_k=True)
    keys = np.flatnonzero(t.iss_keypoints(*ic.PARAMS["main"][0]))
    random65 = np.sort(np.random.default_rng(61).choice(n, 65, replace=False))
    for R in (keys, np.arange(n), [0], [n - 1], [], random65):
        R = np.asarray(R, np.int64)
        G, gk = t.fpfh(r, want_k=True, rows=R)
        assert G.dtype == np.float32 and G.shape == (len(R), 33) and gk.dtype == np.int64
        assert np.array_equal(G, F[R]) and np.array_equal(gk, k[R])
        assert np.array_equal(t.fpfh(r, rows=R), G)
    assert len(keys) == ic.EXPECTED[("main", 0)] and F[keys].any()
    shuffled = np.random.default_rng(62).permutation(random65)
    assert np.any(np.diff(shuffled) < 0)
    assert np.array_equal(pcr.compute_fpfh_rows(pts, shuffled, nrm, radius=r), F[shuffled])
    assert np.array_equal(pcr.compute_fpfh_rows(pts, [], nrm, radius=r), np.zeros((0, 33), np.float32))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_global_registration_through_keypoints():
    pa, na_, r = fc.cloud("main")
    pb, nb_, _ = fc.cloud("main_moved")
    rs, rn = ic.PARAMS["main"][0]
    args = dict(salient_radius=rs, non_max_radius=rn)
    ka, kb = pcr.iss_keypoints(pa, **args), pcr.iss_keypoints(pb, **args)
    share = len(np.intersect1d(ka, kb)) / len(ka)
    print(f"keypoints {len(ka)} and {len(kb)}, reappearing after the motion: a share of {share:.4f}")
    assert share >= 0.5
    max_dist = 0.1
    T, info = pcr.register_global(pa, pb, r, max_dist, normals=(na_, nb_), keypoints="iss", keypoint_args=args, n_hypotheses=20_000,
                                  return_info=True)
    assert info["hypothesis"] >= 0 and T.shape == (4, 4) and not np.array_equal(T, np.eye(4))
    moved = np.linalg.norm(pa.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - pb.astype(np.float64), axis=1)
    print(f"matches {len(info['inliers'])}, inliers {info['count']}, within max_dist {np.mean(moved <= max_dist):.4f}, largest {moved.max():.3g}")
    assert np.mean(moved <= max_dist) >= 0.95
    # the explicit pair runs the same path
    T2 = pcr.register_global(pa, pb, r, max_dist, normals=(na_, nb_), keypoints=(ka, kb), n_hypotheses=20_000)
    assert np.array_equal(T2, T)
    # fewer than three keypoints on a side: ransac_pose's no-match result
    T3, info3 = pcr.register_global(pa, pb, r, max_dist, normals=(na_, nb_), keypoints=(ka[:2], kb), n_hypotheses=1000, return_info=True)
    assert np.array_equal(T3, np.eye(4)) and info3["hypothesis"] == -1 and info3["count"] == 0
