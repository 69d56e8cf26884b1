"""The list sets of a point target: near (0.1 cell, built with the target), mid (0.25) and far (0.35; not on heavy targets), the
deeper two built once the target has served a dozen search + reduce passes and read by the passes whose scan moved by at least
0.12 / 0.4 cell and less than 1.5 cell since the pass before (pcr_internal.h: PCR_HALO2_FRAC / PCR_HALO3_FRAC / PCR_HALO2_MOVE /
PCR_HALO3_MOVE / PCR_HALO_OUT_MOVE; pass.hip: enqueue_search; kernels.hip: k_gn_update; pass_device.h: select_lists).
PCR_LIST_SET = 0 / 1 / 2 is the developer switch that makes every plain full search read one set.

Every case of tests/list_set_cases.py runs in this process with the switch unset and set to 0, 1 and 2, and in child processes
under PCR_DEEP_LISTS=0 (a library that only ever has the first set) and PCR_XORDER=0.  Whatever set a pass read, its matches must
be brute force in NumPy by the library's own float32 formula, index for index, and every sum, pose, trace and batch result must be
equal bit for bit across the runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import list_set_cases as lc
from conftest import REPO

pytestmark = pytest.mark.gpu

FORCED = ("0", "1", "2")


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


def _child(tmp_path_factory, tag, **switches):
    out = str(tmp_path_factory.mktemp("list_sets") / (tag + ".npz"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), **switches)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "list_set_cases.py"), out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(capi, tmp_path_factory):
    """{"auto" | "0" | "1" | "2" | "first_only" | "old_order": results of every case}"""
    assert not any(os.environ.get(k) for k in ("PCR_LIST_SET", "PCR_HALO", "PCR_DEEP_LISTS", "PCR_DEEP_LISTS_MB")) \
        and os.environ.get("PCR_XORDER", "1") != "0", "this suite sets the switches itself"
    ctx = capi.get_context(0)
    res = {"auto": lc.run_all(capi, ctx)}
    for k in FORCED:
        with pytest.MonkeyPatch.context() as mp:           # (read at every pass)
            mp.setenv("PCR_LIST_SET", k)
            res[k] = lc.run_all(capi, ctx)
    res["first_only"] = _child(tmp_path_factory, "first_only", PCR_DEEP_LISTS="0")
    res["old_order"] = _child(tmp_path_factory, "old_order", PCR_XORDER="0")
    return res


@pytest.fixture(scope="module")
def expected():
    """brute force, once: {name: [(distance, index) per shift]}"""
    return {name: [lc.brute(pts, lc._moved(lc.shift_pose(dx), q), lc.GATE) for dx in lc.SHIFTS] for name, pts, q in lc.hand_cases()}


def test_cases_are_what_they_claim(expected):
    """CPU only: the edge cases sit where they say, the ties are ties, the steps straddle the three thresholds"""
    by = {n: (p, q) for n, p, q in lc.hand_cases()}
    for k, halo in enumerate(lc.HALOS):
        edge = np.float32(np.float32(5.5) + np.float32(0.5) + np.float32(halo))
        xs = [by[f"edge_set{k}_{t}"][0][2, 0] for t in ("below", "at", "above")]
        assert xs[1] == edge and xs[0] == np.nextafter(edge, np.float32(0)) and xs[2] == np.nextafter(edge, np.float32(9))
        for t in ("below", "at", "above"):
            assert expected[f"edge_set{k}_{t}"][0][1][0] == 2             # the point on the edge, not the decoy
    d2 = rc_d2(*by["tie_ab"])
    assert d2[0, 2] == d2[0, 3] == np.float32(0.5625) and expected["tie_ab"][0][1][0] == 2 and expected["tie_ba"][0][1][0] == 2
    for name, x in (("empty_cell_mid", 6.2), ("empty_cell_far", 6.3)):
        pts, q = by[name]
        assert not (np.floor(pts) == np.floor(q[0])).all(1).any() and expected[name][0][1][0] == 2
    steps = np.abs(np.diff(lc.SHIFTS))
    assert (steps[:6] < [0.12, 0.4, 0.4, 1.5, 1.5, 9]).all() and (steps[:6] >= [0, 0.12, 0.12, 0.4, 0.4, 1.5]).all() and steps[6] > 1.5


def rc_d2(pts, q):
    import rows_once_cases as rc
    return rc.d2_all(pts, q)


def test_sets_exist_as_designed(runs):
    """near with the target, mid and far after a dozen passes; a fresh target and the child that opts out have the first only"""
    for form in ("auto",) + FORCED + ("old_order",):
        got = runs[form]
        for name in ("street", "heavy"):
            per_cell = got[name + "/sets_per_cell"]
            want = lc.HALOS[:2] + (0.0,) if name == "heavy" else lc.HALOS       # (a heavy target has no far set)
            assert np.allclose(per_cell, want, atol=1e-6), (form, name, per_cell)
            rec = got[name + "/sets"][:, 1]
            assert 0 < rec[0] < rec[1] and (rec[2] == 0 if name == "heavy" else rec[1] < rec[2]), (form, name, rec)
            assert (got[name + "/fresh_sets"][1:] == 0).all() and got[name + "/fresh_sets"][0, 1] == rec[0]
        assert bool(got["heavy/heavy"]) and not bool(got["street/heavy"])
        assert tuple(got["grid_6x6x4/dims"]) == (6, 6, 4) and tuple(got["min_grid/dims"])[1:] == (2, 2)
        assert (got["grid_6x6x4/sets"][:, 1] > 0).all()
    assert (runs["first_only"]["street/sets"][1:] == 0).all() and runs["first_only"]["street/sets"][0, 1] > 0


@pytest.mark.parametrize("form", ("auto",) + FORCED + ("first_only", "old_order"))
def test_hand_placed_matches_are_brute_force(runs, expected, form):
    got = runs[form]
    for name, pts, q in lc.hand_cases():
        pos = got[name + "/pos"]
        assert np.array_equal(np.sort(pos), np.arange(pts.shape[0])), (form, name)          # the probe found every point itself
        for k, (d, i) in enumerate(expected[name]):
            assert np.array_equal(got[name + "/idx"][k], i), (form, name, k, got[name + "/idx"][k], i)
            # split and fused pass count brute force's matches and sum the same squared distances (float32 residuals summed in
            # float64: 1e-6 relative covers the float32 rounding of a residual, 6e-8 each)
            e2 = float((d[i >= 0].astype(np.float64) ** 2).sum())
            for path in ("sums", "fused"):
                s = got[f"{name}/{path}"][k]
                assert s[28] == (i >= 0).sum() and np.isclose(s[27], e2, rtol=1e-6, atol=1e-12), (form, name, path, k)


@pytest.mark.parametrize("form", FORCED + ("first_only",))
def test_every_result_is_equal_across_sets(runs, form):
    """matches, the 29 sums of the split and the fused path, both loops' poses and traces, align_batch: bit for bit"""
    skip = ("/sets", "/sets_per_cell", "/fresh_sets")
    keys = sorted(k for k in runs["auto"] if not k.endswith(skip))
    assert keys == sorted(k for k in runs[form] if not k.endswith(skip))
    for k in keys:
        assert runs["auto"][k].shape == runs[form][k].shape and np.array_equal(runs["auto"][k], runs[form][k]), (form, k)


def test_old_order_target_agrees(runs):
    """a target built under PCR_XORDER=0 (other positions inside a cell, so other cell-sorted indices): same sums and poses"""
    keys = sorted(k for k in runs["auto"] if not k.endswith(("/pos", "_matches", "/sets", "/sets_per_cell", "/fresh_sets")))
    for k in keys:
        assert np.array_equal(runs["auto"][k], runs["old_order"][k]), k


def test_warmed_target_equals_fresh(runs):
    for form in ("auto",) + FORCED:
        for name in ("street", "heavy"):
            got = runs[form]
            assert np.array_equal(got[name + "/warm_sums"], got[name + "/fresh_sums"]), (form, name)
            assert np.array_equal(got[name + "/warm_matches"], got[name + "/fresh_matches"]), (form, name)
            assert (got[name + "/warm_matches"] >= 0).sum() > 5000
            assert np.array_equal(got[name + "/both"][:, 0, :], got[name + "/both"][:, 1, :])          # split == fused
