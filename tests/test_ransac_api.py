"""RANSAC pose hypotheses and pose scoring: the interface, its refusals, the host-side fit, and the restatement of
tests/ransac_cases.py against known answers and against the planted pose of the recovery case.  Needs no GPU."""

import inspect

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import ransac_cases as rc


@pytest.fixture()
def no_gpu(monkeypatch):
    """Any attempt to reach the library or a context fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", refuse)
    monkeypatch.setattr(_capi, "get_context", refuse)


def test_names_are_exported():
    for name in ("score_poses", "fit_rigid", "ransac_pose", "register_global"):
        assert name in pcr.__all__ and callable(getattr(pcr, name))
    p = inspect.signature(pcr.ransac_pose).parameters
    assert list(p)[:11] == ["source", "target", "ia", "ib", "max_dist", "n_hypotheses", "seed", "edge_similarity", "min_edge", "refine_rounds",
                            "return_info"]
    assert (p["n_hypotheses"].default, p["seed"].default, p["edge_similarity"].default, p["min_edge"].default, p["refine_rounds"].default,
            p["return_info"].default) == (100_000, 0, 0.9, 0.0, 5, False)
    p = inspect.signature(pcr.score_poses).parameters
    assert list(p)[:7] == ["source", "target", "ia", "ib", "Ts", "max_dist", "return_mask"] and p["return_mask"].default is False
    p = inspect.signature(pcr.register_global).parameters
    assert list(p)[:7] == ["source", "target", "feature_radius", "max_dist", "normals", "mutual", "ratio"]
    assert p["mutual"].default is True and p["ratio"].default is None
    assert callable(_capi.pose_score) and callable(_capi.ransac_poses)


def test_prototypes():
    assert len(_capi.PROTOTYPES["pcr_pose_score"][1]) == 9
    assert len(_capi.PROTOTYPES["pcr_ransac_poses"][1]) == 16
    assert "pcr_pose_score_splits" in _capi.PROTOTYPES
    with open(_capi.os.path.join(_capi.os.path.dirname(_capi.os.path.dirname(_capi.__file__)), "include", "pcr.h")) as f:
        header = f.read()
    for name in ("pcr_pose_score", "pcr_ransac_poses", "pcr_pose_score_splits"):
        assert f"{name}(" in header
    assert f"#define PCR_RANSAC_TILE {_capi.RANSAC_TILE}\n" in header


def test_bad_arguments_are_refused_before_the_gpu(no_gpu):
    rng = np.random.default_rng(0)
    P, Q = rng.uniform(-1, 1, (8, 3)).astype(np.float32), rng.uniform(-1, 1, (9, 3)).astype(np.float32)
    ia, ib = np.arange(8), np.arange(8)
    I = np.eye(4)
    for bad in (-1e-30, -1.0, np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError, match="max_dist"):
            pcr.ransac_pose(P, Q, ia, ib, bad)
        with pytest.raises(ValueError, match="max_dist"):
            pcr.score_poses(P, Q, ia, ib, I, bad)
        with pytest.raises(ValueError, match="min_edge"):
            pcr.ransac_pose(P, Q, ia, ib, 0.1, min_edge=bad)
    for bad in (-1e-6, 1.0001, np.nan, np.inf):
        with pytest.raises(ValueError, match="edge_similarity"):
            pcr.ransac_pose(P, Q, ia, ib, 0.1, edge_similarity=bad)
    for bad in (-1, (1 << 26) + 1):
        with pytest.raises(ValueError, match="n_hypotheses"):
            pcr.ransac_pose(P, Q, ia, ib, 0.1, n_hypotheses=bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            pcr.ransac_pose(P, Q, ia, ib, 0.1, seed=bad)
    for bad in (np.nan, np.inf, -np.inf):
        p = P.copy(); p[3, 1] = bad
        q = Q.copy(); q[5, 2] = bad
        for fn in (lambda a, b: pcr.ransac_pose(a, b, ia, ib, 0.1), lambda a, b: pcr.score_poses(a, b, ia, ib, I, 0.1)):
            with pytest.raises(ValueError, match="finite"):
                fn(p, Q)
            with pytest.raises(ValueError, match="finite"):
                fn(P, q)
    with pytest.raises(ValueError, match="finite"):
        pcr.ransac_pose(P.astype(np.float64) * 1e39, Q, ia, ib, 0.1)
    # more than 2^24 correspondences (a broadcast view: no memory behind it)
    big = np.broadcast_to(np.zeros((1, 3), np.float32), ((1 << 24) + 1, 3))
    with pytest.raises(ValueError, match="2\\^24"):
        _capi.check_pairs(big, big)
    with pytest.raises(ValueError, match="2\\^26"):
        _capi.pose_score(None, P, P, np.broadcast_to(np.zeros((1, 12), np.float32), ((1 << 26) + 1, 12)), 0.1)
    for shape in ((8,), (8, 2), (2, 4, 3)):
        with pytest.raises(ValueError, match="shape"):
            pcr.ransac_pose(np.zeros(shape), Q, ia, ib, 0.1)
    with pytest.raises(ValueError, match="one length"):
        pcr.ransac_pose(P, Q, ia, ib[:7], 0.1)
    with pytest.raises(ValueError, match="outside"):
        pcr.ransac_pose(P, Q, ia + 1, ib, 0.1)
    with pytest.raises(ValueError, match="outside"):
        pcr.score_poses(P, Q, ia, ib - 1, I, 0.1)
    with pytest.raises(ValueError, match="integer"):
        pcr.ransac_pose(P, Q, ia.astype(float), ib, 0.1)
    for T in (np.zeros((3, 4)), np.zeros((2, 3, 3)), np.zeros(16)):
        with pytest.raises(ValueError, match="Ts"):
            pcr.score_poses(P, Q, ia, ib, T, 0.1)
    with pytest.raises(ValueError, match="refine_rounds"):
        pcr.ransac_pose(P, Q, ia, ib, 0.1, refine_rounds=-1)


def test_empty_inputs_need_no_gpu(no_gpu):
    rng = np.random.default_rng(1)
    P, Q = rng.uniform(-1, 1, (8, 3)).astype(np.float32), rng.uniform(-1, 1, (8, 3)).astype(np.float32)
    none = np.zeros(0, np.int64)
    for m in (0, 1, 2):
        T, info = pcr.ransac_pose(P, Q, np.arange(m), np.arange(m), 0.5, n_hypotheses=100, return_info=True)
        assert np.array_equal(T, np.eye(4)) and info["hypothesis"] == -1 and info["count"] == 0 and info["n_valid"] == 0
        assert info["inliers"].shape == (m,) and not info["inliers"].any() and info["fitness"] == 0
    T, info = pcr.ransac_pose(P, Q, np.arange(8), np.arange(8), 0.5, n_hypotheses=0, return_info=True)
    assert np.array_equal(T, np.eye(4)) and info["hypothesis"] == -1 and info["count"] == 0
    counts, masks = pcr.score_poses(P, Q, none, none, np.tile(np.eye(4), (3, 1, 1)), 0.5, return_mask=True)
    assert counts.tolist() == [0, 0, 0] and counts.dtype == np.int32 and masks.shape == (3, 0) and masks.dtype == np.bool_
    counts = pcr.score_poses(P, Q, np.arange(8), np.arange(8), np.zeros((0, 4, 4)), 0.5)
    assert counts.shape == (0,)
    r = _capi.ransac_poses(None, P[:2], Q[:2], 5, 0, 0.5, 0.9, 0.0, want_all=True)
    assert np.all(r["samples"] == -1) and np.all(np.isnan(r["poses"])) and np.all(r["counts"] == -1) and r["best"] == -1


def test_mix_known_answers():
    assert rc.mix(0) == 0xE220A8397B1DCDAF and rc.mix(1) == 0x910A2DEC89025CC1


@pytest.mark.parametrize("m", [3, 4, 5, 1000])
def test_samples_are_distinct_and_in_range(m):
    seen = set()
    for seed in (0, 1, (1 << 63) + 5):
        S = rc.samples(seed, 600, m)
        assert S.shape == (600, 3) and S.dtype == np.int32 and S.min() >= 0 and S.max() < m
        assert np.all(S[:, 0] != S[:, 1]) and np.all(S[:, 1] != S[:, 2]) and np.all(S[:, 0] != S[:, 2])
        seen |= {tuple(s) for s in S.tolist()}
    if m <= 5:
        assert len(seen) == m * (m - 1) * (m - 2)            # every ordered triple of distinct rows turns up
    if m == 1000:
        assert not np.array_equal(rc.samples(0, 50, m), rc.samples(1, 50, m))
    assert np.all(rc.samples(0, 7, 2) == -1)


def test_fit_rigid_recovers_an_exact_rigid_motion():
    rng = np.random.default_rng(5)
    P = rng.uniform(-10, 10, (50, 3))
    T = pcr.makeT(pcr.expSO3(np.array([0.4, -1.1, 2.0])), np.array([3.0, -8.0, 0.25]))
    Q = P @ T[:3, :3].T + T[:3, 3]
    G = pcr.fit_rigid(P, Q)
    assert G.shape == (4, 4) and G.dtype == np.float64 and np.array_equal(G[3], [0, 0, 0, 1])
    assert np.abs(G - T).max() < 1e-12 and abs(np.linalg.det(G[:3, :3]) - 1) < 1e-12
    assert np.array_equal(G, rc.kabsch(P, Q))
    # a mirrored set: the determinant correction keeps a rotation
    M = pcr.fit_rigid(P, P * [1, 1, -1])
    assert abs(np.linalg.det(M[:3, :3]) - 1) < 1e-12
    # three points are enough
    assert np.abs(pcr.fit_rigid(P[:3], Q[:3]) - T).max() < 1e-9
    with pytest.raises(ValueError, match="shape"):
        pcr.fit_rigid(P[:2], Q[:2])


def test_triad_fit_of_congruent_triangles_is_their_motion():
    rng = np.random.default_rng(6)
    P = rng.uniform(-4, 4, (30, 3)).astype(np.float32)
    T = pcr.makeT(pcr.expSO3(np.array([0.0, 0.0, np.pi / 2])), np.array([1.0, 2.0, 3.0]))
    Q = (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    r = rc.ransac(P, Q, 64, 0, 1e-3, 0.9, 0.0)
    assert r["n_valid"] == 64 and r["count"] == 30
    assert np.abs(rc.T_of(r["pose"]) - T).max() < 1e-4
    # collinear and repeated rows make no hypothesis
    L = np.outer(np.arange(10), [1, 2, 3]).astype(np.float32)
    assert rc.ransac(L, L, 64, 0, 1.0, 0.9, 0.0)["n_valid"] == 0
    assert rc.ransac(np.tile(P[:1], (10, 1)), np.tile(Q[:1], (10, 1)), 64, 0, 1.0, 0.9, 0.0)["best"] == -1


def test_refine_pose_is_the_restatements_refinement():
    """The module's host refinement over the restatement's scoring = the restatement's ransac_pose, bit for bit."""
    from point_cloud_registration_amd import global_registration as gr
    c = rc.recovery_case()
    src, dst = c["src"], c["dst"]
    p = rc.RECOVERY
    r = rc.ransac(src, dst, 1024, 0, p["max_dist"], p["edge_similarity"], p["min_edge"])

    def score(T):
        cnt, mask = rc.score(src, dst, rc.pose12(T)[None], p["max_dist"])
        return int(cnt[0]), mask[0]
    T, count, mask, rmse = gr.refine_pose(score, src, dst, rc.T_of(r["pose"]), 5)
    Tr, info = rc.ransac_pose(src, dst, p["max_dist"], 1024, 0, p["edge_similarity"], p["min_edge"])
    assert np.array_equal(rc.pose12(T), info["pose"]) and np.abs(T - Tr).max() < 1e-7
    assert count == info["count"] and np.array_equal(mask, info["inliers"]) and rmse == info["rmse"]


@pytest.mark.parametrize("n_hyp", [1024, 4096])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_recovers_the_planted_pose(n_hyp, seed):
    c = rc.recovery_case()
    p = rc.RECOVERY
    assert c["planted"].sum() == p["inliers"] and len(c["src"]) == p["m"]
    T, info = rc.ransac_pose(c["src"], c["dst"], p["max_dist"], n_hyp, seed, p["edge_similarity"], p["min_edge"])
    raw = rc.ransac(c["src"], c["dst"], n_hyp, seed, p["max_dist"], p["edge_similarity"], p["min_edge"])
    cloud, Tt = c["cloud"], c["T_true"]
    true = cloud @ Tt[:3, :3].T + Tt[:3, 3]
    def worst(Tc):
        return float(np.linalg.norm(cloud @ Tc[:3, :3].T + Tc[:3, 3] - true, axis=1).max())
    print(f"H {n_hyp} seed {seed}: best h {info['hypothesis']}, n_valid {info['n_valid']}, raw count {raw['count']}, refined count {info['count']}, "
          f"rmse {info['rmse']:.4g}, largest displacement raw {worst(rc.T_of(raw['pose'])):.4g}, refined {worst(T):.4g}")
    assert np.array_equal(info["inliers"], c["planted"])
    assert worst(T) < p["max_dist"]
