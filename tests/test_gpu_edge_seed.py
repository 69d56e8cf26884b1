"""The seed of a query outside the target's grid box (nn_device.h: nn_ring0; GeomSwitches::edge_seed, PCR_EDGE_SEED=0 is the
developer off switch).

Every case of tests/edge_seed_cases.py is searched with the seed (this process) and without it (a child process with
PCR_EDGE_SEED=0), and both again on targets in the old order inside a cell (PCR_XORDER=0: the plain range scan): the matches
must be brute force in NumPy by the library's own float32 formula -- original index and float32 distance bit for bit -- and
the matches, the 29 sums, poses and iteration counts with and without the seed must be equal bit for bit.  The seed is a
real target point tested like any candidate, so nothing may move."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_seed_cases as ec
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def mine(capi):
    assert os.environ.get("PCR_EDGE_SEED", "1") != "0" and os.environ.get("PCR_XORDER", "1") != "0", "this suite compares the defaults with the switches"
    return ec.run_all(capi, capi.get_context(0))


def _child(tmp_path_factory, tag, **switches):
    """the same cases in a child process under the given switches (they are read once per process)"""
    out = str(tmp_path_factory.mktemp("edge_seed") / (tag + ".npz"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), **switches)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "edge_seed_cases.py"), out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def unseeded(tmp_path_factory):
    return _child(tmp_path_factory, "off", PCR_EDGE_SEED="0")


@pytest.fixture(scope="module")
def old_order(tmp_path_factory):
    return _child(tmp_path_factory, "old", PCR_XORDER="0")


@pytest.fixture(scope="module")
def old_order_unseeded(tmp_path_factory):
    return _child(tmp_path_factory, "old_off", PCR_XORDER="0", PCR_EDGE_SEED="0")


SKIP = ("/x_ordered", "/heavy", "/cell", "/dims")


def _same(a, b, name):
    keys = sorted(k for k in a if k.startswith(name + "/") and not k.endswith(SKIP))
    assert keys and sorted(k for k in b if k.startswith(name + "/") and not k.endswith(SKIP)) == keys
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def hand():
    """target, names, queries and the brute-force answers with and without the gate -- computed once"""
    pts = ec.hand_target()
    names, q = ec.hand_queries()
    return pts, names, q, ec.brute(pts, q, ec.MAX_DIST), ec.brute(pts, q)


def test_numpy_brute_force_is_the_oracles(hand):
    """the float32 fma of the NumPy brute force is emulated: the C oracle's d2f gives the same distances and indices"""
    from oracle import oracle
    pts, names, q, gated, (d, i) = hand
    do, io = oracle.nn_brute(pts, q)
    assert np.array_equal(d, do) and np.array_equal(i, io)


def test_hand_placed_box_is_what_the_cases_assume(mine, hand):
    pts, names, q, gated, free = hand
    assert float(mine["hand/cell"]) == 1.0 and tuple(mine["hand/dims"]) == (6, 6, 4)
    assert np.array_equal(pts.min(0), np.zeros(3, np.float32))
    assert ec.outside(pts.min(0), 1.0, (6, 6, 4), q).all()                  # every query exercises the branch
    cq = np.clip(ec.cell_of(pts.min(0), 1.0, q), 0, [5, 5, 3])
    cp = ec.cell_of(pts.min(0), 1.0, pts)
    held = np.array([(cp == c).all(1).sum() for c in cq])
    k = {n: names.index(n) for n in ec.SPECIAL}
    assert held[k["empty_cell_seed"]] == 0 and (held == 0).sum() > 50 and (held > 0).sum() > 20
    # the seed (the one point of the clamped cell) is the nearest point / lies beyond the gate while another point matches
    for n, seed in (("seed_is_nearest", 5), ("seed_beyond_gate", 6)):
        assert held[k[n]] == 1 and (cp[seed] == cq[k[n]]).all()
    assert gated[1][k["seed_is_nearest"]] == 5
    assert np.linalg.norm(pts[6].astype(np.float64) - q[k["seed_beyond_gate"]]) > ec.MAX_DIST and gated[1][k["seed_beyond_gate"]] == 7
    # faces, edges and corners at 0.3, 1 and 3 cells
    for kind, count in (("face", 6), ("edge", 12), ("corner", 8)):
        assert len({n.split("_")[0] for n in names if n.startswith(kind)}) == count
        assert all(sum(n.startswith(kind) and f"_{d}_" in n for n in names) == 3 * count for d in (0.3, 1.0, 3.0))


def test_hand_placed_queries_outside_the_box(mine, unseeded, hand):
    """outside each face, edge and corner at 0.3, 1 and 3 cells; at, just inside and beyond the gate; an empty clamped cell
    with a seed; two equidistant points; the seed as the nearest point and the seed beyond the gate"""
    pts, names, q, (dg, ig), (df, i_f) = hand
    assert np.array_equal(mine["hand/nn_i"], ig), [names[k] for k in np.flatnonzero(mine["hand/nn_i"] != ig)[:8]]
    assert np.array_equal(mine["hand/nn_d"], dg)
    assert np.array_equal(mine["hand/nn_i_inf"], i_f) and np.array_equal(mine["hand/nn_d_inf"], df)
    k = {n: names.index(n) for n in ec.SPECIAL}
    assert ig[k["gate_inside"]] == 0 and ig[k["gate_exact"]] == -1 and ig[k["gate_beyond"]] == -1
    assert np.isinf(mine["hand/nn_d"][k["gate_exact"]]) and mine["hand/nn_d_inf"][k["gate_exact"]] == np.float32(2.0)
    assert mine["hand/nn_i"][k["equidistant"]] == 3                        # (3 and 4 are equally far: the smaller index)
    assert (ig >= 0).sum() > 30 and (ig < 0).sum() > 100                   # matches and queries beyond the gate, both
    _same(mine, unseeded, "hand")
    # search + reduce (batches of 4) and the fused kernel (batches of 8) count the same matches
    assert mine["hand/sums"][0, 28] == mine["hand/sums"][1, 28] >= (ig >= 0).sum() - 1      # (gate_inside is 1e-4 from the gate)


def test_cells_beyond_the_gap_cap_have_no_seed(mine, unseeded):
    """between two clusters 40 cells apart a clamped cell is farther than 15 cells from any point: no seed, no match, and
    the queries beside the clusters still find theirs"""
    pts, q = ec.far_target(), ec.far_queries()
    assert tuple(mine["far/dims"]) == (42, 3, 3) and ec.outside(pts.min(0), 1.0, (42, 3, 3), q).all()
    d, i = ec.brute(pts, q, ec.MAX_DIST)
    assert np.array_equal(mine["far/nn_i"], i) and np.array_equal(mine["far/nn_d"], d)
    assert list(i[:3]) == [-1, -1, -1] and i[3] >= 0 and i[4] >= 0
    d, i = ec.brute(pts, q)
    assert np.array_equal(mine["far/nn_i_inf"], i) and np.array_equal(mine["far/nn_d_inf"], d)
    _same(mine, unseeded, "far")


def test_street_target_along_its_trajectory(mine, unseeded):
    """20 k-point street target, 2 k-point scan at the five poses of its own Gauss-Newton trajectory, ICP and PlaneICP: the
    matches of nn_query, the 29 sums of the split path and of the fused small-scan kernel, and align_batch with two items"""
    target, normals, scan = ec.street_case()
    assert bool(mine["street/x_ordered"]) and not bool(mine["street/heavy"])
    assert mine["street/poses"].shape[0] == 5 and mine["street/sums"].shape == (10, 2, 29)
    # a tenth of the scan at least starts outside the box: the test cannot pass without the branch
    q0 = ec._moved(mine["street/poses"][0], scan)
    share = ec.outside(target.min(0), float(mine["street/cell"]), mine["street/dims"], q0).mean()
    print(f"outside the box at the start pose: {share:.3f}")
    assert share >= 0.10
    d, i = ec.brute(target, q0, ec.MAX_DIST)
    assert np.array_equal(mine["street/nn_i0"], i) and np.array_equal(mine["street/nn_d0"], d)
    assert np.array_equal(mine["street/sums"][:, 0, :], mine["street/sums"][:, 1, :])          # split == fused
    _same(mine, unseeded, "street")


def test_heavy_target_and_old_order(mine, unseeded, old_order, old_order_unseeded):
    """a LiDAR sweep (heavy cells: the boxes path) and every case again on targets built under PCR_XORDER=0 (the plain
    range scan): with the seed, without it and in either order, the same results"""
    assert bool(mine["heavy/heavy"]) and not bool(mine["heavy/x_ordered"])
    _same(mine, unseeded, "heavy")
    assert not bool(old_order["street/x_ordered"]) and not bool(old_order_unseeded["street/x_ordered"])
    for name in ("hand", "far", "street", "heavy"):
        _same(old_order, old_order_unseeded, name)
        _same(mine, old_order, name)
