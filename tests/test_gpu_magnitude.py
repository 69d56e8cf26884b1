"""The point search far from the origin and across long grids: every case of tests/magnitude_cases.py (slack / h from 0 to 9.7,
grids of 2^14 (x) and 2^13 (y, z) cells along one axis with points and queries within three float32 steps of cell faces,
and ties whose smaller index lies two cells away) against brute force by the
library's own float32 formula, index for index and distance bit for bit -- nn_query bounded and unbounded, knn_query at k = 7
and 20, radius_count, and the matches and counts of the split and the fused pass at sixteen poses in two scan frames, on a target
warmed by fourteen passes so that it has its mid and far list sets.  The passes run with PCR_LIST_SET unset and forced to 0, 1
and 2, and in child processes under PCR_HEAVY=1, PCR_XORDER=0 and PCR_EDGE_SEED=0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import magnitude_cases as mc
from conftest import REPO, rel_H

pytestmark = pytest.mark.gpu

FORCED = ("0", "1", "2")
CHILDREN = {"heavy": {"PCR_HEAVY": "1"}, "old_order": {"PCR_XORDER": "0"}, "no_seed": {"PCR_EDGE_SEED": "0"}}
CASES = mc.cases()
CHILD_SECONDS = 240                                    # a child takes ~15 s


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _start_child(tmp_path_factory, tag, **switches):
    out = str(tmp_path_factory.mktemp("magnitude") / (tag + ".npz"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), **switches)
    return out, subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "magnitude_cases.py"), out], env=env,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.fixture(scope="module")
def runs(capi, tmp_path_factory):
    """{"auto" | "0" | "1" | "2" | "heavy" | "old_order" | "no_seed": results of every case}"""
    switches = ("PCR_LIST_SET", "PCR_HALO", "PCR_DEEP_LISTS", "PCR_DEEP_LISTS_MB", "PCR_HEAVY", "PCR_GRID_CELL")
    assert not any(os.environ.get(k) for k in switches) and os.environ.get("PCR_XORDER", "1") != "0" \
        and os.environ.get("PCR_EDGE_SEED", "1") != "0", "this suite sets the switches itself"
    ctx = capi.get_context(0)
    children = {tag: _start_child(tmp_path_factory, tag, **env) for tag, env in CHILDREN.items()}      # (beside this process)
    res = {"auto": mc.run_all(capi, ctx)}
    for k in FORCED:
        with pytest.MonkeyPatch.context() as mp:           # (read at every pass)
            mp.setenv("PCR_LIST_SET", k)
            res[k] = mc.run_all(capi, ctx, queries=False)
    try:
        for tag, (out, proc) in children.items():
            text = proc.communicate(timeout=CHILD_SECONDS)[0]
            assert proc.returncode == 0, (tag, text)
            res[tag] = dict(np.load(out))
    finally:
        for _, proc in children.values():                  # (a child that is still there: none is left behind)
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    return res


@pytest.fixture(scope="module")
def expected(orc):
    """brute force, once: per case the whole table of sorted distances and indices of the queries, and per frame and pose the
    nearest neighbour of the scan as the float32 transform moves it and the oracle's sums"""
    out = {}
    for c in CASES:
        pts, q = mc._f32(c.pts), mc._f32(c.q)
        e = {"rows": orc.knn_brute(pts, q, pts.shape[0]), "self": orc.nn_brute(pts, pts)[1]}
        o_pts = orc.TargetPoints(pts)
        for frame in mc.FRAMES:
            scan, idx, sums = c.scan(frame), [], []
            for P in c.poses(frame):
                d, i = orc.nn_brute(pts, orc.transform(P, scan))
                idx.append(np.where(d < np.float32(c.gate), i, -1))
                sums.append(orc.calc_H_g_e2(orc.ICP, o_pts, P, scan, c.gate, with_count=True))
            e[frame] = (np.stack(idx), sums)
            if c.loops_in(frame):                          # the oracle's own loop from the first pose
                trace = []
                T = orc.align(orc.ICP, o_pts, scan, c.poses(frame)[0], mc.LOOP_ITERS, 1e-3, c.gate, trace=trace)
                margin = min(abs(np.linalg.norm(orc.solve6(H, g)) - 1e-3) for _, H, g, _ in trace)
                e[frame + "/loop"] = (T, len(trace), margin)
        out[c.name] = e
    return out


ALL_FORMS = ("auto",) + FORCED + tuple(CHILDREN)
PROCESSES = ("auto",) + tuple(CHILDREN)                 # the queries read no deeper list set: once per process


def test_forms_are_what_the_switches_ask_for(runs):
    """the search form of every run, as index_info() reports it: (heavy, x-ordered)"""
    for form in ALL_FORMS:
        forms = {tuple(runs[form][c.name + "/form"]) for c in CASES}
        print(f"{form}: (heavy, x-ordered) = {sorted(forms)}")
        assert forms == {{"heavy": (1, 0), "old_order": (0, 0)}.get(form, (0, 1))}, (form, forms)
        for c in CASES:
            assert tuple(runs[form][c.name + "/dims"]) == mc.dims_of(c.pts, c.h), (form, c.name)
            assert float(runs[form][c.name + "/cell"]) == c.h, (form, c.name)


def test_all_three_sets_exist_in_every_regime(runs):
    """near with the target, mid and far after fourteen passes, each with its margin of 0.1 / 0.25 / 0.35 cell (the slack is
    added where a list is built, not to the margin a set reports); a heavy target has no far set (pcr_build_deep_lists)"""
    for form in ALL_FORMS:
        for c in CASES:
            sets = runs[form][c.name + "/sets"]
            want = mc.HALOS[:2] + (0.0,) if form == "heavy" else mc.HALOS
            assert np.allclose(sets[:, 0] / c.h, want, atol=1e-6), (form, c.name, sets)
            rec = sets[:, 1]
            assert mc.N_POINTS <= rec[0] <= rec[1] and (rec[2] == 0 if form == "heavy" else rec[1] <= rec[2]), (form, c.name, rec)


@pytest.mark.parametrize("form", PROCESSES)
def test_queries_are_brute_force(runs, expected, form):
    """nn_query with and without the gate, knn_query at k = 7 and 20, radius_count at 0.7 cell"""
    got = runs[form]
    for c in CASES:
        d, i = expected[c.name]["rows"]
        n = c.name
        assert np.array_equal(got[n + "/nn_i_inf"], i[:, 0]) and np.array_equal(got[n + "/nn_d_inf"], d[:, 0]), (form, n)
        hit = d[:, 0] < np.float32(c.gate)
        assert np.array_equal(got[n + "/nn_i"], np.where(hit, i[:, 0], -1)), (form, n)
        assert np.array_equal(got[n + "/nn_d"], np.where(hit, d[:, 0], np.float32(np.inf))), (form, n)
        for k in mc.KS:
            assert np.array_equal(got[f"{n}/knn{k}_i"], i[:, :k]) and np.array_equal(got[f"{n}/knn{k}_d"], d[:, :k]), (form, n, k)
        assert np.array_equal(got[n + "/radius"], (d <= np.float32(mc.RADIUS_CELLS * c.h)).sum(1)), (form, n)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_pass_matches_and_counts_are_brute_force(runs, expected, form):
    """the split pass' matches as original indices at every pose of both frames; its count, the fused pass' count and the
    counts of both on a scan in the device's own order"""
    got = runs[form]
    for c in CASES:
        pos = got[c.name + "/pos"]
        # the probe: every point finds itself, or the first of the points at float32 distance zero from it -- its twins, and on
        # long_x the three points a denormal step apart around x = 0, whose squared distance underflows
        first = expected[c.name]["self"]
        assert (pos >= 0).all() and np.array_equal(pos, pos[first]), (form, c.name)
        assert np.unique(pos).shape[0] == np.unique(first).shape[0], (form, c.name)
        for frame in mc.FRAMES:
            idx, _ = expected[c.name][frame]
            key = f"{c.name}/{frame}"
            bad = np.argwhere(got[key + "/idx"] != idx)
            assert bad.shape[0] == 0, (form, key, bad.shape[0], bad[:5].tolist())
            count = (idx >= 0).sum(1)
            for path in ("sums", "fused", "reuse"):
                assert np.array_equal(got[f"{key}/{path}"][:, 28], count), (form, key, path)
            assert np.array_equal(got[key + "/sorted"][:, :, 28], np.stack([count[::5]] * 2)), (form, key)
            assert count.min() > 150


@pytest.mark.parametrize("form", ("auto", "heavy"))
def test_sums_against_the_oracle(runs, expected, form):
    """the tolerance of test_fuzz_against_oracle: 1e-9 of max |H|, equal count"""
    from point_cloud_registration_amd import _capi
    worst = 0.0
    for c in CASES:
        for frame in mc.FRAMES:
            sums = runs[form][f"{c.name}/{frame}/sums"]
            for k, (Ho, go, e2o, cnto) in enumerate(expected[c.name][frame][1]):
                H, g, e2, cnt = _capi.unpack29(sums[k])
                assert cnt == cnto, (form, c.name, frame, k)
                rel = rel_H(H, Ho)
                worst = max(worst, rel)
                assert rel < 1e-9, (form, c.name, frame, k, rel)
                assert np.max(np.abs(g - go)) <= 1e-9 * max(np.max(np.abs(H)), np.max(np.abs(go))), (form, c.name, frame, k)
                assert abs(e2 - e2o) <= 1e-9 * abs(e2o), (form, c.name, frame, k, e2, e2o)
    print(f"{form}: worst max|dH| / max|H| = {worst:.3g}")


def test_split_equals_fused_and_reuse_changes_nothing(runs):
    for form in ("auto",) + FORCED:
        got = runs[form]
        for c in CASES:
            for frame in mc.FRAMES:
                key = f"{c.name}/{frame}"
                assert np.array_equal(got[key + "/sums"], got[key + "/fused"]), (form, key)
                assert np.array_equal(got[key + "/sums"], got[key + "/reuse"]), (form, key)
                assert np.array_equal(got[key + "/sorted"][0], got[key + "/sorted"][1]), (form, key)


@pytest.mark.parametrize("form", FORCED + ("no_seed",))
def test_every_result_is_equal_across_sets_and_without_the_seed(runs, form):
    """whatever set a pass reads, and with or without the seed of queries outside the box: matches, sums, both loops' poses
    and traces, align_batch -- bit for bit"""
    keys = sorted(runs[form])
    assert keys == sorted(k for k in runs["auto"] if form == "no_seed" or not ("/nn_" in k or "/knn" in k or k.endswith("/radius")))
    for k in keys:
        assert runs["auto"][k].shape == runs[form][k].shape and np.array_equal(runs["auto"][k], runs[form][k], equal_nan=True), (form, k)


def test_old_order_and_heavy_targets_agree(runs):
    """other positions inside a cell, so other cell-sorted indices: the same matches as original indices (above), the same sums,
    poses and traces bit for bit under PCR_XORDER=0, as tests/test_gpu_list_sets.py demands; the heavy form within the
    tolerance of the fuzz test"""
    skip = ("/pos", "/sets", "/form")
    keys = sorted(k for k in runs["auto"] if not k.endswith(skip))
    for k in keys:
        assert np.array_equal(runs["auto"][k], runs["old_order"][k], equal_nan=True), k
    for k in keys:
        a, b = runs["auto"][k], runs["heavy"][k]
        if k.endswith(("/idx", "/radius")) or "/nn_" in k or "/knn" in k:
            assert np.array_equal(a, b), k
        elif k.endswith(("/sums", "/fused", "/reuse", "/sorted")):
            a, b = a.reshape(-1, 29), b.reshape(-1, 29)
            assert np.array_equal(a[:, 28], b[:, 28]), k
            hmax, gmax = np.abs(a[:, :21]).max(1), np.abs(a[:, 21:27]).max(1)            # per component, as against the oracle
            assert (np.abs(a[:, :21] - b[:, :21]).max(1) <= 1e-9 * hmax).all(), k
            assert (np.abs(a[:, 21:27] - b[:, 21:27]).max(1) <= 1e-9 * np.maximum(hmax, gmax)).all(), k
            assert (np.abs(a[:, 27] - b[:, 27]) <= 1e-9 * np.abs(a[:, 27])).all(), k


@pytest.mark.parametrize("form", ("auto", "heavy"))
def test_loops_ran_and_follow_the_oracle(runs, expected, form):
    """every loop that the cases run (magnitude_cases.Case.loops_in) holds a pose and a trace -- no error is caught anywhere, a
    singular system would have ended the run -- the host-driven and the device-resident loop take the oracle's number of
    iterations and end within 1e-6 (1 + |t|) of the oracle's pose (eight float32 steps of a transformed coordinate: a rounding of
    one transformed point that falls the other way moves a residual, and so the pose, by one such step at most); every item of
    align_batch ends with status 0"""
    got, seen = runs[form], 0
    for c in CASES:
        for frame in mc.FRAMES:
            key = f"{c.name}/{frame}"
            if not c.loops_in(frame):
                assert not any(k.startswith(key + "/") and k.endswith(("/device", "/host", "/batch")) for k in got)
                continue
            To, ito, margin = expected[c.name][frame + "/loop"]
            scale = 1.0 + np.abs(To[:3, 3]).max()
            for loop in ("device", "host"):
                r = got[f"{key}/{loop}"]
                it = int(r[16])
                assert r.shape == (17 + 45 * it,) and np.isfinite(r).all() and 1 <= it <= mc.LOOP_ITERS, (form, key, loop, r.shape)
                err = np.abs(r[:16].reshape(4, 4) - To).max() / scale
                print(f"{form} {key} {loop}: {it} iterations (oracle {ito}), pose off the oracle's by {err:.2e}")
                if margin > 1e-6:                          # (a step that lands ON the tolerance may fall either way: as
                    assert it == ito and err <= 1e-6, (form, key, loop, it, ito, err)      # test_fuzz_align_against_oracle_loop)
                seen += 1
            b = got[key + "/batch"]
            assert b.shape == (2 * 16 + 4,) and np.isfinite(b).all() and (b[32:34] >= 1).all() and (b[34:] == 0).all(), (form, key, b[32:])
    assert seen == 2 * (len(CASES) + 2 + 3)                # the sensor frame of every case, the map frame near the origin
