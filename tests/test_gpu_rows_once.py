"""The row-once traversal of the plain float32 point search on x-ordered targets (nn_device.h: nn_rows_x; PCR_ROWS_ONCE=0 is
the compile-time switch back to the ring loop).

Every case of tests/rows_once_cases.py goes through nn_query (gated at 2 m and at 6.5 m, and ungated), through the split pass
and through the fused pass, on targets with the shallow extended lists (this process), with lists of a whole cell (PCR_HALO=1:
nn_ring0 returns kstart = 2) and, in a child process, without lists (PCR_HALO=0).  The matches must be brute force in NumPy by
the library's own float32 formula -- original index and float32 distance bit for bit, ties to the smaller original index.  The
street target is also run by a child process that builds it under PCR_XORDER=0: that child runs the untouched ring loop, and the
29 sums of both paths and align_batch must be equal bit for bit.

Two things the cases could not be built as first described: the grid gives every axis at least two cells, so the target "of a
single row of cells" is a single row of OCCUPIED cells in a 15 x 2 x 2 box; and the hand-placed box is 13 x 8 x 6 cells, so that a
point 5 cells away in x and rows 3 cells away in y and z fit around one query."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rows_once_cases as rc
from conftest import REPO

pytestmark = pytest.mark.gpu

FORMS = ("shallow", "deep", "nolists")


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


def _child(tmp_path_factory, tag, what, **switches):
    out = str(tmp_path_factory.mktemp("rows_once") / (tag + ".npz"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), **switches)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "rows_once_cases.py"), out, what], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def hand(capi, tmp_path_factory):
    """{form: results of every hand-placed case}"""
    assert all(os.environ.get(k, "1") != "0" for k in ("PCR_XORDER", "PCR_EDGE_SEED")) and not os.environ.get("PCR_HALO"), "this suite sets the switches itself"
    ctx = capi.get_context(0)
    res = {"shallow": rc.run_hand(capi, ctx)}
    with pytest.MonkeyPatch.context() as mp:           # (read when a target is built)
        mp.setenv("PCR_HALO", "1.0")
        res["deep"] = rc.run_hand(capi, ctx)
    res["nolists"] = _child(tmp_path_factory, "nolists", "hand", PCR_HALO="0")
    return res


@pytest.fixture(scope="module")
def sets():
    """[(name, points, queries, tie)] of every hand-placed target, the filled box included"""
    return rc.hand_cases() + [("fill", rc.fill_target(), rc.fill_queries()[1], False)]


@pytest.fixture(scope="module")
def expected(sets):
    """brute force, once: {name: {gate or inf: (distance, index)}}"""
    return {name: {**{g: rc.brute(pts, q, g) for g in rc.GATES}, np.inf: rc.brute(pts, q)} for name, pts, q, _ in sets}


def test_cases_are_what_they_claim(sets, expected):
    """CPU only: no tie but the deliberate ones, the cells the cases are drawn on, and that the cases reach where the two
    traversals differ"""
    byname = {name: (pts, q) for name, pts, q, _ in sets}
    for name, pts, q, tie in sets:
        uniq, d2 = rc.unique_nearest(pts, q)
        assert uniq != tie, name
        if tie:
            assert d2[0, 0] == d2[0, 1] == np.float32(6.25) and (pts.shape[0] < 3 or d2[0, 2] > d2[0, 1])
    cell = lambda p: tuple(np.floor(np.asarray(p, np.float32)).astype(int))
    for d, sgn in ((1, 1), (3, -1), (5, 1)):
        pts, q = byname[f"own_row_{d}"]
        assert cell(pts[2]) == (5 + sgn * d, 3, 2) and cell(q[0]) == (5, 3, 2)
        for tag in ("", "_z"):
            pts, q = byname[f"own_row_{d}_adjacent_farther{tag}"]
            assert expected[f"own_row_{d}_adjacent_farther{tag}"][np.inf][1][0] == 2
            c3 = cell(pts[3])
            assert max(abs(c3[1] - 3), abs(c3[2] - 2)) == 1
    for m in (1, 2, 3):
        for tag in (f"row_dy+{m}", f"row_dy-{m}", f"row_dz+{m}", f"row_dz-{m}", f"row_dy{m}_dz{m}"):
            pts, q = byname[tag]
            cp, cq = cell(pts[2]), cell(q[0])
            assert max(abs(cp[1] - cq[1]), abs(cp[2] - cq[2])) == m and abs(cp[0] - cq[0]) > m, tag
            assert expected[tag][6.5][1][0] == 2, tag
    for gap in (2, 3):
        for m in range(gap):
            for side in ("left", "right", "both"):
                pts, q = byname[f"gap{gap}_m{m}_{side}"]
                for p in pts[2:]:
                    cp = cell(p)
                    assert abs(cp[0] - 5) == gap and max(abs(cp[1] - 3), abs(cp[2] - 2)) == m
    e = expected
    assert e["gate_exact"][2.0][1][0] == -1 and e["gate_exact"][np.inf][0][0] == np.float32(2.0) and e["gate_ulp_inside"][2.0][1][0] == 2
    assert e["tie_own_row_first"][np.inf][1][0] == 2 and e["tie_neighbour_row_first"][np.inf][1][0] == 2
    assert e["list_certified"][2.0][1][0] == 2 and e["list_not_certified"][2.0][1][0] == 3 and e["list_halo_copy"][2.0][1][0] == 3
    names, q = rc.fill_queries()
    assert (e["fill"][6.5][1][[n.endswith("_7.0") for n in names]] == -1).all() and (e["fill"][2.0][1] >= 0).sum() > 40
    assert np.array_equal(byname["fill"][0].min(0), np.zeros(3, np.float32))


@pytest.mark.parametrize("form", FORMS)
def test_hand_placed_cases(hand, sets, expected, form):
    got = hand[form]
    for name, pts, q, tie in sets:
        assert bool(got[name + "/x_ordered"]) and float(got[name + "/cell"]) == 1.0, name
        halo = float(got[name + "/halo"])
        assert {"shallow": 0.0 < halo < 0.5, "deep": halo >= 1.0, "nolists": halo == 0.0}[form], (name, halo)
        for gate in rc.GATES + (np.inf,):
            tag = "inf" if gate == np.inf else str(gate)
            d, i = expected[name][gate]
            assert np.array_equal(got[f"{name}/nn_i_{tag}"], i), (form, name, tag, got[f"{name}/nn_i_{tag}"], i)
            assert np.array_equal(got[f"{name}/nn_d_{tag}"], d), (form, name, tag)
            if gate == np.inf:
                continue
            # the passes: the split and the fused path count brute force's matches and sum the same squared distances; both
            # accumulate float32 residuals in float64, so 1e-6 relative covers the float32 rounding of a residual (6e-8 each)
            s = got[f"{name}/sums_{tag}"]
            assert s[0, 28] == s[1, 28] == (i >= 0).sum(), (form, name, tag, s[:, 28])
            e2 = float((d[i >= 0].astype(np.float64) ** 2).sum())
            assert np.allclose(s[:, 27], e2, rtol=1e-6, atol=1e-12), (form, name, tag, s[:, 27], e2)
    if form != "shallow":                              # the sums themselves: the same on every form, bit for bit
        for k in sorted(k for k in got if "/sums_" in k):
            assert np.array_equal(got[k], hand["shallow"][k]), (form, k)


def test_hand_placed_box(hand):
    got = hand["shallow"]
    assert tuple(got["own_row_1/dims"]) == (13, 8, 6) and tuple(got["fill/dims"]) == (9, 6, 4)
    assert tuple(got["single_row/dims"])[1:] == (2, 2) and tuple(got["one_point/dims"]) == (2, 2, 2)


@pytest.fixture(scope="module")
def street(capi):
    return rc.run_street(capi, capi.get_context(0))


@pytest.fixture(scope="module")
def street_rings(tmp_path_factory):
    return _child(tmp_path_factory, "rings", "street", PCR_XORDER="0")


def test_street_target_matches_brute_force(street):
    target, normals, scan = rc.street_case()
    assert bool(street["street/x_ordered"]) and street["street/poses"].shape[0] == 5
    # brute force by the C oracle (the same float32 formula and tie rule as rows_once_cases.brute -- tests/test_gpu_edge_seed.py
    # compares the two -- at a tenth of the time), then the strict gate
    from oracle import oracle
    for k in range(5):
        d, i = oracle.nn_brute(target, rc._moved(street["street/poses"][k], scan))
        miss = ~(d < np.float32(2.0))
        d, i = np.where(miss, np.float32(np.inf), d), np.where(miss, -1, i)
        assert (i >= 0).sum() > 500
        assert np.array_equal(street[f"street/nn_i{k}"], i) and np.array_equal(street[f"street/nn_d{k}"], d), k
    assert np.array_equal(street["street/sums"][:, 0, :], street["street/sums"][:, 1, :])          # split == fused


def test_street_target_against_the_ring_loop(street, street_rings):
    assert not bool(street_rings["street/x_ordered"])
    keys = sorted(k for k in street if k != "street/x_ordered")
    assert keys == sorted(k for k in street_rings if k != "street/x_ordered")
    for k in keys:
        assert street[k].shape == street_rings[k].shape and np.array_equal(street[k], street_rings[k]), k
