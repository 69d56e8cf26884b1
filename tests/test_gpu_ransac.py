"""RANSAC pose hypotheses and pose scoring on the GPU (csrc/ransac.hip) against the NumPy restatement of
tests/ransac_cases.py: samples, poses (NaNs in the same places), counts, masks and the winner bit for bit."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import ransac_cases as rc
from test_gpu_parity import capi, ctx, orc, _pose_close  # noqa: F401

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = _capi.RANSAC_TILE
H_ALL = 4097
MD, SIM, EDGE = 0.05, 0.8, 0.3


def assert_same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    assert np.array_equal(nan_a, nan_b)                                           # NaNs in the same places
    assert np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


def assert_ransac(got, ref, n_hyp=None):
    """got of _capi.ransac_poses(want_all=True) against the restatement (its first n_hyp hypotheses)."""
    n = len(ref["counts"]) if n_hyp is None else n_hyp
    assert np.array_equal(got["samples"], ref["samples"][:n])
    assert_same_bits(got["poses"], ref["poses"][:n])
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], ref["counts"][:n])
    counts = ref["counts"][:n]
    n_valid = int((counts >= 0).sum())
    best = int(np.argmax(counts)) if n_valid else -1
    assert got["n_valid"] == n_valid and got["best"] == best
    if best >= 0:
        assert got["count"] == counts[best]
        assert_same_bits(got["pose"], ref["poses"][best])
    else:
        assert got["count"] == 0 and got["pose"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


@pytest.fixture(scope="module")
def refs():
    """(m, seed) -> (src, dst, the restatement over H_ALL hypotheses): computed once per key, shared and left unchanged."""
    cache = {}

    def get(m, seed):
        if (m, seed) not in cache:
            src, dst = rc.random_pairs(m, seed=100 + m, inlier_share=1.0 if m < 10 else 0.5)
            cache[(m, seed)] = (src, dst, rc.ransac(src, dst, H_ALL, seed, MD, SIM, EDGE))
        return cache[(m, seed)]
    return get


# ---- per-hypothesis bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 4, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_hypotheses_equal_the_restatement(ctx, refs, m):
    src, dst, ref = refs(m, 0)
    got = _capi.ransac_poses(ctx, src, dst, H_ALL, 0, MD, SIM, EDGE, want_all=True)
    assert_ransac(got, ref)
    if m >= 63:
        assert ref["n_valid"] > 0 and ref["count"] >= 3
    # without the per-hypothesis arrays: the same winner
    lean = _capi.ransac_poses(ctx, src, dst, H_ALL, 0, MD, SIM, EDGE)
    assert (lean["best"], lean["count"], lean["n_valid"]) == (got["best"], got["count"], got["n_valid"])
    assert_same_bits(lean["pose"], got["pose"])


@pytest.mark.parametrize("n_hyp", [1, 2, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("m", [65, 2 * TILE + 1])
def test_hypothesis_counts(ctx, refs, m, n_hyp):
    src, dst, ref = refs(m, 0)
    assert_ransac(_capi.ransac_poses(ctx, src, dst, n_hyp, 0, MD, SIM, EDGE, want_all=True), ref, n_hyp)


@pytest.mark.parametrize("seed", [1, (1 << 63) + 5])
@pytest.mark.parametrize("m", [5, 1000])
def test_seeds(ctx, refs, m, seed):
    src, dst, ref = refs(m, seed)
    assert_ransac(_capi.ransac_poses(ctx, src, dst, H_ALL, seed, MD, SIM, EDGE, want_all=True), ref)
    assert not np.array_equal(ref["samples"], refs(m, 0)[2]["samples"])


# ---- pcr_pose_score ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def score_case():
    """5000 correspondences and 257 poses: hypotheses of the restatement (some invalid: NaN), the planted motion, identity."""
    src, dst = rc.random_pairs(5000, seed=9)
    poses = rc.ransac(src, dst, 257, 3, MD, 0.5, 0.0)["poses"].copy()
    from point_cloud_registration_amd.math_tools import expSO3
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = expSO3(np.array([0.2, -0.1, 0.7])), [1.0, -2.0, 0.5]
    poses[0], poses[1], poses[2] = rc.pose12(T), rc.pose12(np.eye(4)), np.nan
    poses[70, 4] = np.nan                                                          # one NaN entry is enough
    return src, dst, poses


@pytest.mark.parametrize("m", [1, 2, 65, 5000])
@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 257])
def test_pose_score_equals_the_restatement(ctx, score_case, b, m):
    src, dst, poses = score_case
    src, dst, poses = src[:m], dst[:m], poses[:b]
    counts, masks = rc.score(src, dst, poses, 0.2)
    got_c, got_m = _capi.pose_score(ctx, src, dst, poses, 0.2, want_mask=True)
    assert got_c.dtype == np.int32 and got_m.dtype == np.bool_ and got_m.shape == (b, m)
    assert np.array_equal(got_c, counts) and np.array_equal(got_m, masks)
    assert np.array_equal(_capi.pose_score(ctx, src, dst, poses, 0.2), counts)     # (without the mask: the same counts)
    if m == 5000:
        assert counts[0] > 2000                                                    # the planted motion
        assert _capi.pose_score_splits(m, b) > 1                                   # few poses, many rows: the split-M path
    else:
        assert _capi.pose_score_splits(m, b) == 1
    if b > 2:
        assert counts[2] == 0 and not masks[2].any()                               # a NaN pose scores 0
    if b > 70:
        assert counts[70] == 0


def test_pose_score_many_poses_take_the_unsplit_path(ctx, score_case):
    """Enough poses to fill the chip on their own: the rows are not split, every lane walks several tiles."""
    src, dst, poses = score_case
    m, b = 2 * TILE + 1, 600_000
    assert _capi.pose_score_splits(m, b) == 1
    counts = rc.score(src[:m], dst[:m], poses, 0.2)[0]
    reps = -(-b // len(poses))
    many = np.tile(poses, (reps, 1))[:b]
    got = _capi.pose_score(ctx, src[:m], dst[:m], many, 0.2)
    assert np.array_equal(got, np.tile(counts, reps)[:b])


def test_score_poses_interface(score_case):
    src, dst, poses = score_case
    m = 65
    ia = np.arange(m)[::-1].copy()
    ib = np.arange(m)
    Ts = np.stack([rc.T_of(p) for p in poses[:3]])
    counts, masks = rc.score(src[ia], dst[ib], poses[:3], 0.2)
    c, k = pcr.score_poses(src, dst, ia, ib, Ts, 0.2, return_mask=True)
    assert np.array_equal(c, counts) and np.array_equal(k, masks)
    assert np.array_equal(pcr.score_poses(src, dst, ia, ib, Ts, 0.2), counts)
    c1, k1 = pcr.score_poses(src, dst, ia, ib, Ts[0], 0.2, return_mask=True)
    assert isinstance(c1, int) and c1 == counts[0] and np.array_equal(k1, masks[0])


# ---- the threshold ----------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive(ctx):
    rng = np.random.default_rng(2)
    q = 2.0 ** -10
    md = np.float32(5 * 2.0 ** -4)
    up = np.nextafter(md, np.float32(1))
    n = 40
    src = (rng.integers(-2048, 2048, (n, 3)) * q).astype(np.float32)
    src[:, 0] = 0                                       # (0 + the next float32 above max_dist is exact)
    off = np.zeros((n, 3), np.float32)
    off[0:5, 0] = md; off[5:10, 1] = md; off[10:15, 2] = -md
    off[15:20] = [3 * 2.0 ** -4, 4 * 2.0 ** -4, 0]       # 9 + 16 = 25: |offset| = max_dist exactly
    off[20:25, 0] = up
    off[25:30, 0] = -up
    off[30:35] = 0
    off[35:40] = [q, 0, 0]
    dst = src + off
    assert np.array_equal(dst.astype(np.float64), src.astype(np.float64) + off.astype(np.float64))
    I = rc.pose12(np.eye(4))[None]
    want = np.r_[np.ones(20, bool), np.zeros(10, bool), np.ones(10, bool)]
    c, k = _capi.pose_score(ctx, src, dst, I, float(md), want_mask=True)
    assert np.array_equal(k[0], want) and c[0] == 30
    assert np.array_equal(rc.score(src, dst, I, md)[1][0], want)
    c, k = _capi.pose_score(ctx, src, dst, I, 0.0, want_mask=True)                 # only coincident rows
    assert np.array_equal(k[0], np.r_[np.zeros(30, bool), np.ones(5, bool), np.zeros(5, bool)]) and c[0] == 5


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx):
    rng = np.random.default_rng(4)
    P, Q = rng.uniform(-3, 3, (200, 3)).astype(np.float32), rng.uniform(-3, 3, (200, 3)).astype(np.float32)
    identity = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    # the same correspondence row repeated
    got = _capi.ransac_poses(ctx, np.tile(P[:1], (50, 1)), np.tile(Q[:1], (50, 1)), 300, 0, 1.0, 0.0, 0.0, want_all=True)
    assert got["n_valid"] == 0 and got["best"] == -1 and got["count"] == 0 and got["pose"].tolist() == identity
    assert np.all(got["counts"] == -1) and np.all(np.isnan(got["poses"])) and got["samples"].min() >= 0
    # collinear triples
    L = np.outer(np.arange(50), [1, 2, 3]).astype(np.float32)
    got = _capi.ransac_poses(ctx, L, L + np.float32(1), 300, 0, 1.0, 0.0, 0.0, want_all=True)
    assert_ransac(got, rc.ransac(L, L + np.float32(1), 300, 0, 1.0, 0.0, 0.0))
    assert got["n_valid"] == 0 and got["best"] == -1
    # M = 0, 1, 2
    for m in (0, 1, 2):
        got = _capi.ransac_poses(ctx, P[:m], Q[:m], 10, 0, 1.0, 0.9, 0.0, want_all=True)
        assert got["best"] == -1 and got["count"] == 0 and got["n_valid"] == 0 and got["pose"].tolist() == identity
        assert np.all(got["counts"] == -1)
    # all outliers, nothing valid: unrelated points never have equal edge lengths
    got = _capi.ransac_poses(ctx, P, Q, 2000, 0, 1.0, 1.0, 0.0, want_all=True)
    ref = rc.ransac(P, Q, 2000, 0, 1.0, 1.0, 0.0)
    assert_ransac(got, ref)
    assert got["best"] == -1 and got["n_valid"] == 0 and got["pose"].tolist() == identity
    T, info = pcr.ransac_pose(P, Q, np.arange(200), np.arange(200), 1.0, n_hypotheses=2000, edge_similarity=1.0, return_info=True)
    assert np.array_equal(T, np.eye(4)) and info["hypothesis"] == -1 and info["count"] == 0 and not info["inliers"].any()
    # edge_similarity = 1 on a noisy copy
    src, dst = rc.random_pairs(300, seed=12, inlier_share=1.0, noise=1e-3)
    got = _capi.ransac_poses(ctx, src, dst, 2000, 0, 0.05, 1.0, 0.0, want_all=True)
    assert_ransac(got, rc.ransac(src, dst, 2000, 0, 0.05, 1.0, 0.0))
    # and a min_edge that cuts some of the triples
    got = _capi.ransac_poses(ctx, src, dst, 2000, 0, 0.05, 0.9, 4.0, want_all=True)
    ref = rc.ransac(src, dst, 2000, 0, 0.05, 0.9, 4.0)
    assert_ransac(got, ref)
    assert 0 < ref["n_valid"] < 2000


def test_refusals_leave_the_context_usable(ctx, score_case):
    src, dst, poses = score_case
    L = _capi.lib()
    bad = src[:10].copy()
    bad[3, 1] = np.nan
    count = np.zeros(2, np.int32)
    best, bc, nv, pose = _capi.C.c_int64(), _capi.C.c_int32(), _capi.C.c_int64(), np.zeros(12, np.float32)
    assert L.pcr_pose_score(ctx.handle, bad, dst[:10], 10, poses[:2], 2, 0.1, count, None) == _capi.PCR_ERR_INVALID
    assert L.pcr_pose_score(ctx.handle, src[:10], dst[:10], 10, poses[:2], 2, -0.1, count, None) == _capi.PCR_ERR_INVALID
    assert L.pcr_pose_score(ctx.handle, src[:10], dst[:10], (1 << 24) + 1, poses[:2], 2, 0.1, count, None) == _capi.PCR_ERR_INVALID
    refs = (_capi.C.byref(best), pose, _capi.C.byref(bc), _capi.C.byref(nv), None, None, None)
    for args in ((10, 10, 0, float("nan"), 0.9, 0.0), (10, 10, 0, 0.1, 1.5, 0.0), (10, 10, 0, 0.1, -0.1, 0.0), (10, 10, 0, 0.1, 0.9, -1.0),
                 (10, 10, 0, 0.1, 0.9, float("inf")), (10, -1, 0, 0.1, 0.9, 0.0), (10, (1 << 26) + 1, 0, 0.1, 0.9, 0.0),
                 ((1 << 24) + 1, 10, 0, 0.1, 0.9, 0.0)):
        assert L.pcr_ransac_poses(ctx.handle, src[:10], dst[:10], *args, *refs) == _capi.PCR_ERR_INVALID, args
    assert L.pcr_ransac_poses(ctx.handle, src[:10], bad, 10, 10, 0, 0.1, 0.9, 0.0, *refs) == _capi.PCR_ERR_INVALID
    # m == 0, b == 0, n_hyp == 0: PCR_OK
    count[:] = 7
    assert L.pcr_pose_score(ctx.handle, src[:0], dst[:0], 0, poses[:2], 2, 0.1, count, None) == 0 and count.tolist() == [0, 0]
    assert L.pcr_pose_score(ctx.handle, src[:10], dst[:10], 10, poses[:0], 0, 0.1, count, None) == 0
    assert L.pcr_ransac_poses(ctx.handle, src[:10], dst[:10], 10, 0, 0, 0.1, 0.9, 0.0, *refs) == 0 and best.value == -1 and bc.value == 0
    # the context still works
    assert np.array_equal(_capi.pose_score(ctx, src[:65], dst[:65], poses[:3], 0.2), rc.score(src[:65], dst[:65], poses[:3], 0.2)[0])


# ---- ties -------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_hypothesis(ctx):
    src, dst = rc.ties_case()
    TIES = rc.TIES
    k = {key: TIES[key] for key in ("n_hyp", "seed", "max_dist", "edge_similarity", "min_edge")}
    ref = rc.ransac(src, dst, **k)
    full = np.flatnonzero(ref["counts"] == TIES["m"])
    assert len(full) > 100 and ref["best"] == full[0] == np.flatnonzero(ref["counts"] >= 0)[0] > 0
    got = _capi.ransac_poses(ctx, src, dst, k["n_hyp"], k["seed"], k["max_dist"], k["edge_similarity"], k["min_edge"], want_all=True)
    assert_ransac(got, ref)
    assert got["best"] == full[0] and got["count"] == TIES["m"]
    # the same winner with 64 hypotheses per chunk (read once per process: a child)
    code = ("import sys, json, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests');"
            "from point_cloud_registration_amd import _capi; import ransac_cases as t;"
            "src, dst = t.ties_case(); k = t.TIES;"
            "g = _capi.ransac_poses(_capi.get_context(0), src, dst, k['n_hyp'], k['seed'], k['max_dist'], k['edge_similarity'], k['min_edge'], want_all=True);"
            "print(json.dumps(dict(best=g['best'], count=g['count'], n_valid=g['n_valid'], pose=g['pose'].view(np.uint32).tolist(),"
            " counts=g['counts'].tolist(), samples=g['samples'].ravel().tolist())))")
    r = subprocess.run([sys.executable, "-c", code, REPO], env=dict(os.environ, PCR_RANSAC_CHUNK="64"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert (child["best"], child["count"], child["n_valid"]) == (got["best"], got["count"], got["n_valid"])
    assert child["pose"] == got["pose"].view(np.uint32).tolist()
    assert child["counts"] == got["counts"].tolist() and child["samples"] == got["samples"].ravel().tolist()


# ---- recovery ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hyp", [1024, 4096])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recovers_the_planted_pose(ctx, n_hyp, seed):
    c, p = rc.recovery_case(), rc.RECOVERY
    src, dst = c["src"], c["dst"]
    rows = np.arange(len(src))
    T, info = pcr.ransac_pose(src, dst, rows, rows, p["max_dist"], n_hypotheses=n_hyp, seed=seed, edge_similarity=p["edge_similarity"],
                              min_edge=p["min_edge"], return_info=True)
    Tr, ref = rc.ransac_pose(src, dst, p["max_dist"], n_hyp, seed, p["edge_similarity"], p["min_edge"])
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert np.array_equal(T, Tr) and np.array_equal(info["inliers"], ref["inliers"]) and info["count"] == ref["count"]
    assert info["hypothesis"] == ref["hypothesis"] and info["n_valid"] == ref["n_valid"] and info["rmse"] == ref["rmse"]
    assert info["fitness"] == ref["count"] / p["m"]
    assert info["pose"].dtype == np.float32 and np.array_equal(info["pose"], ref["pose"])
    assert np.abs(T - rc.T_of(info["pose"])).max() < 1e-7 and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-15
    again, mask = pcr.score_poses(src, dst, rows, rows, rc.T_of(info["pose"]), p["max_dist"], return_mask=True)
    assert again == info["count"] and np.array_equal(mask, info["inliers"])               # what info describes is the pose as scored
    assert np.array_equal(info["inliers"], c["planted"])
    cloud, Tt = c["cloud"], c["T_true"]
    moved = np.linalg.norm((cloud @ T[:3, :3].T + T[:3, 3]) - (cloud @ Tt[:3, :3].T + Tt[:3, 3]), axis=1)
    print(f"H {n_hyp} seed {seed}: best h {info['hypothesis']}, count {info['count']}, rmse {info['rmse']:.4g}, largest displacement {moved.max():.4g}")
    assert moved.max() < p["max_dist"]
    assert np.array_equal(pcr.ransac_pose(src, dst, rows, rows, p["max_dist"], n_hypotheses=n_hyp, seed=seed, edge_similarity=p["edge_similarity"],
                                          min_edge=p["min_edge"]), T)


# ---- end to end -------------------------------------------------------------------------------------------------------------
E2E = dict(n=4096, radius=6.7, max_dist=0.3, n_hypotheses=20_000, min_edge=5.0)


def e2e_case():
    from point_cloud_registration_amd.math_tools import expSO3
    from point_cloud_registration_amd.synthetic import street, street_normals
    target = street(E2E["n"], seed=3)
    nt = street_normals(target)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = expSO3(np.array([0.3, -0.5, 1.2])), [4.0, -7.0, 1.5]
    Ti = np.linalg.inv(T)                                                          # scan -> target is T
    scan = np.ascontiguousarray(target.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], dtype=np.float32)
    ns = np.ascontiguousarray(nt.astype(np.float64) @ Ti[:3, :3].T, dtype=np.float32)
    return target, nt, scan, ns, T


def test_register_global_gives_plane_icp_its_start():
    target, nt, scan, ns, T_true = e2e_case()
    T, info = pcr.register_global(scan, target, E2E["radius"], E2E["max_dist"], normals=(ns, nt), n_hypotheses=E2E["n_hypotheses"],
                                  min_edge=E2E["min_edge"], return_info=True)
    print(f"register_global: {len(info['inliers'])} matches, {info['count']} inliers, rmse {info['rmse']:.3g}, hypothesis {info['hypothesis']}, "
          f"|dt| {np.linalg.norm(T[:3, 3] - T_true[:3, 3]):.3g}")
    picp = pcr.PlaneICP(max_dist=1.0, k=10)
    picp.set_target(target)
    assert _pose_close(picp.align(scan, init_T=T), T_true)
    assert not _pose_close(picp.align(scan, init_T=np.eye(4)), T_true)             # the same align from identity does not get there


# ---- determinism and neighbours ---------------------------------------------------------------------------------------------
def test_two_calls_same_bits_and_neighbours_untouched(ctx, refs, score_case):
    src, dst, _ = refs(1000, 0)
    rng = np.random.default_rng(21)
    A, B = rng.uniform(0, 50, (300, 33)).astype(np.float32), rng.uniform(0, 50, (400, 33)).astype(np.float32)
    target, _, scan, _, _ = e2e_case()
    picp = pcr.PlaneICP(max_dist=1.0, k=10)
    picp.set_target(target)
    T0 = np.eye(4)
    before = (_capi.feature_match(ctx, A, B), picp.calc_H_g_e2(T0, target[:1000]))
    a = _capi.ransac_poses(ctx, src, dst, H_ALL, 0, MD, SIM, EDGE, want_all=True)
    b = _capi.ransac_poses(ctx, src, dst, H_ALL, 0, MD, SIM, EDGE, want_all=True)
    for key in ("samples", "counts"):
        assert np.array_equal(a[key], b[key])
    assert_same_bits(a["poses"], b["poses"])
    assert_same_bits(a["pose"], b["pose"])
    assert (a["best"], a["count"], a["n_valid"]) == (b["best"], b["count"], b["n_valid"])
    s, d, poses = score_case
    c1, m1 = _capi.pose_score(ctx, s, d, poses, 0.2, want_mask=True)
    c2, m2 = _capi.pose_score(ctx, s, d, poses, 0.2, want_mask=True)
    assert np.array_equal(c1, c2) and np.array_equal(m1, m2)
    after = (_capi.feature_match(ctx, A, B), picp.calc_H_g_e2(T0, target[:1000]))
    for x, y in zip(before[0], after[0]):
        assert np.array_equal(x, y)
    for x, y in zip(before[1], after[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
