"""FPFH descriptors and feature matching: the interface, its refusals, the host-side selection rule, and the yardsticks of
tests/fpfh_cases.py against themselves.  Needs no GPU."""

import inspect

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import fpfh_cases as fc

NEW_ENTRY_POINTS = ("pcr_target_spfh", "pcr_target_fpfh", "pcr_feature_match")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture()
def no_gpu(monkeypatch):
    """Any attempt to reach the library or a context fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", refuse)
    monkeypatch.setattr(_capi, "get_context", refuse)


def test_names_are_exported():
    for name in ("compute_fpfh", "match_features", "select_matches"):
        assert name in pcr.__all__ and callable(getattr(pcr, name))
    p = inspect.signature(pcr.compute_fpfh).parameters
    assert list(p) == ["points", "normals", "radius", "k_normals", "device"] and p["normals"].default is None and p["k_normals"].default == 15
    p = inspect.signature(pcr.match_features).parameters
    assert list(p)[2:] == ["mutual", "ratio", "device"] and p["mutual"].default is True and p["ratio"].default is None
    for name in ("spfh", "fpfh"):
        assert callable(getattr(_capi.Target, name))
    assert callable(_capi.feature_match)


def test_prototypes_and_abi_version():
    for name in NEW_ENTRY_POINTS:
        assert name in _capi.PROTOTYPES, name
    assert len(_capi.PROTOTYPES["pcr_target_spfh"][1]) == 4 and len(_capi.PROTOTYPES["pcr_target_fpfh"][1]) == 4
    assert len(_capi.PROTOTYPES["pcr_feature_match"][1]) == 9
    assert _capi.ABI_VERSION == 5


def test_bad_arguments_are_refused_before_the_gpu(no_gpu):
    pts = np.random.default_rng(0).uniform(-1, 1, (8, 3)).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (8, 1))
    for r in (-1e-30, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            pcr.compute_fpfh(pts, nrm, radius=r)
        target = _capi.Target.__new__(_capi.Target)
        with pytest.raises(ValueError, match="radius"):
            target.spfh(r)
        with pytest.raises(ValueError, match="radius"):
            target.fpfh(r)
    with pytest.raises(ValueError, match="radius"):
        pcr.compute_fpfh(pts, nrm)
    for bad in (np.nan, np.inf, -np.inf):
        p = pts.copy(); p[3, 1] = bad
        with pytest.raises(ValueError, match="points must be finite"):
            pcr.compute_fpfh(p, nrm, radius=0.5)
        m = nrm.copy(); m[5, 2] = bad
        with pytest.raises(ValueError, match="normals must be finite"):
            pcr.compute_fpfh(pts, m, radius=0.5)
    with pytest.raises(ValueError, match="finite as float32"):
        pcr.compute_fpfh(pts.astype(np.float64) * 1e39, nrm, radius=0.5)
    for shape in ((8,), (8, 2), (2, 4, 3)):
        with pytest.raises(ValueError, match="shape"):
            pcr.compute_fpfh(np.zeros(shape), radius=0.5)
        with pytest.raises(ValueError, match="shape"):
            pcr.compute_fpfh(pts, np.zeros(shape), radius=0.5)
    with pytest.raises(ValueError, match="shape"):
        pcr.compute_fpfh(pts, nrm[:7], radius=0.5)
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            pcr.compute_fpfh(pts, radius=0.5, k_normals=k)
    f = np.zeros((5, 33), np.float32)
    for a, b in ((f, np.zeros((5, 32), np.float32)), (np.zeros(33, np.float32), f), (f, np.zeros((2, 5, 33), np.float32))):
        with pytest.raises(ValueError, match="shapes"):
            pcr.match_features(a, b)
    for d in (0, 65):
        with pytest.raises(ValueError, match="1 to 64 columns"):
            pcr.match_features(np.zeros((5, d), np.float32), np.zeros((4, d), np.float32))
    for ratio in (-0.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="ratio"):
            pcr.match_features(f, f, ratio=ratio)


def test_empty_inputs_need_no_gpu(no_gpu):
    out = pcr.compute_fpfh(np.zeros((0, 3)), radius=0.5)
    assert out.shape == (0, 33) and out.dtype == np.float32
    for a, b in ((np.zeros((0, 33), np.float32), np.zeros((4, 33), np.float32)), (np.zeros((4, 33), np.float32), np.zeros((0, 33), np.float32))):
        ia, ib, d = pcr.match_features(a, b)
        assert ia.shape == ib.shape == d.shape == (0,) and ia.dtype == ib.dtype == np.int64 and d.dtype == np.float32


def test_select_matches():
    #             A0 -> B2 (and back), A1 -> B0 (B0 prefers A3), A2 -> B1 (back), A3 -> B0 (back), A4 -> nothing
    idx_ab = np.array([2, 0, 1, 0, -1], np.int64)
    idx_ba = np.array([3, 2, 0], np.int64)
    d1 = np.array([4.0, 1.0, 9.0, 0.25, np.inf], np.float32)
    d2 = np.array([16.0, 1.0, 9.5, np.inf, np.inf], np.float32)
    ia, ib, d = pcr.select_matches(idx_ab, d1, d2, idx_ba, mutual=True)
    assert ia.dtype == ib.dtype == np.int64 and d.dtype == np.float32
    assert ia.tolist() == [0, 2, 3] and ib.tolist() == [2, 1, 0] and d.tolist() == [4.0, 9.0, 0.25]
    ia, ib, d = pcr.select_matches(idx_ab, d1, d2, mutual=False)
    assert ia.tolist() == [0, 1, 2, 3] and ib.tolist() == [2, 0, 1, 0]
    # the ratio: d1 <= ratio^2 d2.  Row 0 sits exactly AT the bound for ratio 0.5 (4 = 0.25 * 16), row 3 has no second
    for ratio, want in ((0.5, [0, 3]), (0.49, [3]), (0.51, [0, 3]), (1.0, [0, 1, 2, 3]), (0.98, [0, 2, 3]), (0.0, [])):
        assert pcr.select_matches(idx_ab, d1, d2, mutual=False, ratio=ratio)[0].tolist() == want, ratio
    assert pcr.select_matches(idx_ab, d1, d2, idx_ba, mutual=True, ratio=0.5)[0].tolist() == [0, 3]
    # the comparison is made in float64: in float32 both sides below round to the same number
    a, b = np.float32(1.0), np.float32(1.0 + 2.0 ** -23)
    r = float(np.sqrt(np.float64(a) / np.float64(b)))
    one = np.zeros(1, np.int64)
    assert len(pcr.select_matches(one, [a], [b], mutual=False, ratio=r * (1 + 1e-12))[0]) == 1
    assert len(pcr.select_matches(one, [a], [b], mutual=False, ratio=r * (1 - 1e-9))[0]) == 0
    with pytest.raises(ValueError, match="idx_ba"):
        pcr.select_matches(idx_ab, d1, d2, mutual=True)
    with pytest.raises(ValueError, match="one length"):
        pcr.select_matches(idx_ab, d1[:3], d2)


def test_pair_feature_by_hand():
    """p = (0,0,0), q = (0,0,1), s = (1,0,0), all normals (0,0,1)."""
    P = np.float32([[0, 0, 0], [0, 0, 1], [1, 0, 0]])
    N = np.tile(np.float32([0, 0, 1]), (3, 1))
    I, J = np.array([0, 0, 1, 1, 2, 2]), np.array([1, 2, 0, 2, 0, 1])
    pf = fc.pair_features(P, N, I, J)
    # (p, q): d parallel to n1 -> alpha = theta = 0 (bins 5), phi = 1 (bin 10); (q, p): the same with d = -z: phi = -1 (bin 0)
    assert pf["bins"][0].tolist() == [5, 10, 5] and pf["bins"][2].tolist() == [5, 0, 5]
    # (p, s): d = x, a1 = a2 = 0: no swap, phi = 0, v = x cross z = -y, alpha = v . n2 = 0, theta = atan2(0, 1) = 0
    assert pf["bins"][1].tolist() == [5, 5, 5] and pf["bins"][4].tolist() == [5, 5, 5]
    # (q, s): d = (1, 0, -1), a1 = a2 = -1: no swap, phi = -1 / sqrt 2 -> floor(5.5 (1 - 0.7071)) = 1
    assert pf["bins"][3].tolist() == [5, 1, 5] and pf["bins"][5].tolist() == [5, 9, 5]
    assert pf["vnorm"][0] == 0
    # equal normals make every pair an exact role tie; it counts as fragile where the other assignment (d = -d) changes phi's bin
    assert np.all(pf["tie"] == 0) and pf["fragile"].tolist() == [True, False, True, True, False, True]


def test_matching_yardstick():
    rng = np.random.default_rng(11)
    A, B = rng.uniform(0, 4, (40, 33)).astype(np.float32), rng.uniform(0, 4, (50, 33)).astype(np.float32)
    B[7] = B[3]                              # duplicate rows: the lower index wins, the second distance equals the first
    B[20] = A[5]                             # a copy: d2 = 0
    B[30] = np.nan
    A[9] = B[3]
    idx, d1, d2 = fc.match_ref(A, B)
    assert idx[9] == 3 and d1[9] == 0 and d2[9] == 0 and idx[5] == 20 and d1[5] == 0 and d2[5] > 0
    assert not np.any(idx == 30) and idx.dtype == np.int64 and d1.dtype == d2.dtype == np.float32
    # row by row, a plain loop in float32
    for i in (0, 5, 9, 17):
        row = []
        for j in range(len(B)):
            s = np.float32(0)
            for c in range(33):
                t = np.float32(A[i, c] - B[j, c])
                s = np.float32(s + np.float32(t * t))
            row.append(s)
        row = np.array(row)
        order = [j for j in np.lexsort((np.arange(len(B)), row)) if not np.isnan(row[j])]
        assert idx[i] == order[0] and d1[i] == row[order[0]] and d2[i] == row[order[1]]
    i1, f1, s1 = fc.match_ref(A, B[:1])
    assert np.all(i1 == 0) and np.all(np.isinf(s1)) and np.all(np.isfinite(f1))
    i2, f2, s2 = fc.match_ref(A, B[30:31])
    assert np.all(i2 == -1) and np.all(np.isinf(f2)) and np.all(np.isinf(s2))


@pytest.mark.parametrize("name", fc.CLOUDS)
def test_fragile_cap_holds(orc, name):
    ref = fc.cloud_ref(orc, name)
    share = fc.assert_cap(ref, name)
    k, pf = ref["k"], ref["pairs"]
    print(f"{name}: {len(ref['I'])} pairs, neighbours mean {k.mean():.2f} ({k.min()} to {k.max()}), closest bin edge {pf['edge'].min():.3g}, "
          f"closest role tie {pf['tie'].min():.3g}, smallest |v| {pf['vnorm'].min():.3g}, fragile pairs {int(pf['fragile'].sum())}, excluded {share:.4f}")
    assert np.array_equal(ref["counts"].reshape(-1, 3, 11).sum(axis=2), np.repeat(k[:, None], 3, axis=1))
    sums = ref["fpfh"].reshape(-1, 3, 11).sum(axis=2)
    assert np.all(np.abs(sums[k > 0] - 200.0) <= 1e-10) and np.all(sums[k == 0] == 0)
    if name == "main":
        assert 19 <= k.mean() <= 23 and k.min() >= 1
    if name == "second":
        assert 18 <= k.mean() <= 22


def test_restatement_agrees_with_itself_under_a_rigid_motion(orc):
    """The main cloud and its copy under a 2 rad yaw, a 0.4 rad roll and the translation (3, -2, 0.5): the restatement's
    matches are the identity for every point."""
    a, b = fc.cloud_ref(orc, "main"), fc.cloud_ref(orc, "main_moved")
    Fa, Fb = a["fpfh"].astype(np.float32), b["fpfh"].astype(np.float32)
    idx_ab, d1, d2 = fc.match_ref(Fa, Fb)
    idx_ba = fc.match_ref(Fb, Fa)[0]
    n = len(Fa)
    print(f"identity share {np.mean(idx_ab == np.arange(n)):.4f}, largest descriptor difference {np.abs(a['fpfh'] - b['fpfh']).max():.3g}")
    assert np.array_equal(idx_ab, np.arange(n)) and np.array_equal(idx_ba, np.arange(n))
    ia, ib, _ = pcr.select_matches(idx_ab, d1, d2, idx_ba, mutual=True)
    assert np.array_equal(ia, np.arange(n)) and np.array_equal(ib, ia)
    assert np.abs(a["fpfh"] - b["fpfh"]).max() < 1e-3
