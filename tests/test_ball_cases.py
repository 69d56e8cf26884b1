"""The yardstick of tests/ball_cases.py against itself: needs no GPU.  The hybrid set is the prefix of the radius segment, equal
sets give equal bits, the case radii do what their comment says, and at most 1 % of every case is fragile -- the cap the GPU
test (tests/test_gpu_ball.py) inherits."""

import numpy as np
import pytest

import ball_cases as bc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("name", list(bc.CASES))
def test_hybrid_set_is_the_prefix_of_the_radius_segment(orc, name):
    pts = bc.cloud(name)
    for r in bc.CASES[name][1]:
        segs = bc.segments(orc, pts, r, key=name)
        whole = bc.case_ref(orc, name, r, 0)
        assert np.array_equal(whole["count"], [len(s) for s in segs])
        for p, s in enumerate(segs):
            assert np.array_equal(whole["lists"][p], np.sort(s))
            if np.isfinite(pts[p]).all():
                d2 = np.sum((pts[s].astype(np.float64) - pts[p].astype(np.float64)) ** 2, axis=1)
                assert len(s) >= 1 and p in s and np.all(np.diff(d2) >= -1e-6 * max(float(r), 1e-6) ** 2)      # (itself, nearest first)
            else:
                assert len(s) == 0
        for m in bc.MAX_NN[1:]:
            ref = bc.case_ref(orc, name, r, m)
            assert np.array_equal(ref["count"], np.minimum(whole["count"], m))
            for p, s in enumerate(segs):
                assert np.array_equal(ref["lists"][p], s[:m])


@pytest.mark.parametrize("name", list(bc.CASES))
def test_equal_sets_give_equal_moments(orc, name):
    for r in bc.CASES[name][1]:
        for m in (0, 3, 17):
            ref = bc.case_ref(orc, name, r, m)
            sid = ref["set_id"]
            if len(sid) == 0:
                continue
            order = np.argsort(sid, kind="stable")
            same = sid[order][1:] == sid[order][:-1]
            for key in ("mean", "cov", "normal"):
                bits = np.ascontiguousarray(ref[key]).view(np.uint64)[order]
                assert np.all(bits[1:][same] == bits[:-1][same]), (name, r, m, key)
    # the radius that holds the whole cloud: one set
    r = bc.CASES[name][1][-1]
    if name not in ("nan", "single", "empty"):
        assert len(set(bc.case_ref(orc, name, r, 0)["set_id"].tolist())) == 1


@pytest.mark.parametrize("name", ["grid", "planes", "sphere", "lidar", "duplicates"])
def test_radii_do_what_they_say(orc, name):
    n = len(bc.cloud(name))
    r0, r1, r2, r3 = bc.CASES[name][1]
    pairs = bc.PAIRS if name == "duplicates" else 0
    for r in (r0, r1):
        c = bc.case_ref(orc, name, r, 0)["count"]
        assert int(np.sum(c == 2)) == 2 * pairs and int(np.sum(c == 1)) == n - 2 * pairs
    c = bc.case_ref(orc, name, r2, 0)["count"]
    print(f"{name}: n = {n}, typical radius {r2}: median count {np.median(c):.0f}, range {c.min()} .. {c.max()}")
    assert 10 <= np.median(c) <= 60
    assert np.all(bc.case_ref(orc, name, r3, 0)["count"] == n)
    assert n % 64 != 0 or name == "grid"


def test_degenerate_clouds(orc):
    ref = bc.case_ref(orc, "nan", 0.5, 0)
    assert ref["count"][17] == 0 and not ref["mean"][17].any() and not ref["cov"][17].any() and not ref["normal"][17].any()
    assert all(17 not in l for l in ref["lists"]) and np.all(np.delete(ref["count"], 17) >= 1)
    for m in bc.MAX_NN:
        one = bc.case_ref(orc, "single", 1.0, m)
        assert one["count"].tolist() == [1] and np.array_equal(one["mean"], bc.cloud("single").astype(np.float64))
        assert not one["cov"].any() and not one["normal"].any()
        none = bc.case_ref(orc, "empty", 1.0, m)
        assert none["count"].shape == (0,) and none["mean"].shape == (0, 3) and none["cov"].shape == (0, 6)
    cov, ok = bc.cov_finish(bc.case_ref(orc, "single", 1.0, 0), bc.COV_PLANE, 1e-3)
    assert ok.all() and np.array_equal(cov, [[1.0 - (1.0 - 1e-3), 0, 0, 1, 0, 1]])


@pytest.mark.parametrize("name,r,max_nn", bc.all_cases())
def test_fragile_share_is_under_the_cap(orc, name, r, max_nn):
    ref = bc.case_ref(orc, name, r, max_nn)
    share = bc.assert_cap(ref, f"{name} r={r} max_nn={max_nn}")
    # a normal is a unit vector or exactly zero, and zero exactly where count < 3
    nn = np.linalg.norm(ref["normal"], axis=1)
    assert np.all((ref["count"] >= 3) == (nn > 0)) and np.allclose(nn[nn > 0], 1.0, atol=1e-12)
    # the covariance is that of the members about their mean, whatever the anchor
    for p in range(0, len(ref["count"]), 97):
        l = ref["lists"][p]
        if len(l):
            q = bc.cloud(name)[l].astype(np.float64)
            direct = np.cov(q.T, bias=True).reshape(3, 3) if len(l) > 1 else np.zeros((3, 3))
            assert np.all(np.abs(bc.full3(ref["cov"][p]) - direct) <= 1e-9 * max(1.0, float(np.abs(q).max()) ** 2))
            assert np.all(np.abs(ref["mean"][p] - q.mean(axis=0)) <= 1e-12 * max(1.0, float(np.abs(q).max())))
    if share:
        print(f"{name} r={r} max_nn={max_nn}: fragile share {share:.4f}")
