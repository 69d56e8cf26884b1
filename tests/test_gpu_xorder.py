"""The x order inside a cell (Geom::xq) and the range scan that uses it (nn_device.h: nn_scan_range_x).

Every case of tests/xorder_cases.py is searched on targets in x order (this process) and on targets in the old order (a child
process with PCR_XORDER=0): the matches must be the oracle's brute force -- original index and float32 distance bit for bit --
and the 29 sums, poses and iteration counts of the two orders must be equal bit for bit.  The search may only skip records that
provably cannot beat the current best, so nothing may move."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xorder_cases as xc
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def mine(capi):
    assert os.environ.get("PCR_XORDER", "1") != "0", "this suite compares the default order with PCR_XORDER=0"
    return xc.run_all(capi, capi.get_context(0))


@pytest.fixture(scope="module")
def old_order(tmp_path_factory):
    """the same cases on targets built under PCR_XORDER=0, in a child process (the switch is read when a target is built)"""
    out = str(tmp_path_factory.mktemp("xorder") / "old.npz")
    env = dict(os.environ, PCR_XORDER="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "xorder_cases.py"), out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


def _same_as_old(mine, old, name):
    keys = sorted(k for k in mine if k.startswith(name + "/") and not k.endswith(("/x_ordered", "/halo2_records")))
    assert keys and sorted(k for k in old if k.startswith(name + "/") and not k.endswith(("/x_ordered", "/halo2_records"))) == keys
    for k in keys:
        assert mine[k].shape == old[k].shape and np.array_equal(mine[k], old[k]), k


HAND = sorted(xc.hand_cases())


@pytest.mark.parametrize("name", HAND)
def test_hand_placed_case(name, mine, old_order, orc):
    """rows of 1 .. 17 points (batch edges of B = 4 and 8), skewed rows, a wall of equal x with duplicates, points closer in x
    than the quantum, equidistant points on opposite sides, the first and the last record, ring-0 lists"""
    pts, q = xc.hand_cases()[name]
    assert bool(mine[name + "/x_ordered"]) and not bool(old_order[name + "/x_ordered"])
    d, i = orc.nn_brute(pts, q)
    assert np.array_equal(mine[name + "/nn_i"], i), np.flatnonzero(mine[name + "/nn_i"] != i)[:8]
    assert np.array_equal(mine[name + "/nn_d"], d)
    _same_as_old(mine, old_order, name)
    # search + reduce (batches of 4) and the fused kernel (batches of 8) add the same matches in the same order
    assert mine[name + "/sums"][0, 28] == mine[name + "/sums"][1, 28]


def test_equidistant_points_keep_the_smaller_index(mine):
    """(1 - 0.25, y) and (1 + 0.25, y) are exactly 0.25 from (1, y): stored left-right in one pair and right-left in the other,
    the smaller original index wins whichever side the scan reaches first"""
    pts, q = xc.hand_cases()["equidistant"]
    i = mine["equidistant/nn_i"]
    for k in (0, 1):
        tied = np.flatnonzero((np.abs(pts[:, 0] - 1.0) == 0.25) & (pts[:, 1] == q[k, 1]))
        assert tied.size == 2 and i[k] == tied.min()
        assert mine["equidistant/nn_d"][k] == np.float32(0.25)


def test_both_list_sets_are_scanned_in_x_order(mine, old_order):
    """the deeper list set exists after a dozen search + reduce passes; a scan without history reads it, its second pass the
    first set: the sums of both are those of the old order and of each other"""
    for name in ("lists", "street"):
        assert int(mine[name + "/halo2_records"]) > 0 and int(old_order[name + "/halo2_records"]) == int(mine[name + "/halo2_records"])
        assert np.array_equal(mine[name + "/sums_deep"], old_order[name + "/sums_deep"])
    assert np.array_equal(mine["lists/sums_deep"][0], mine["lists/sums_deep"][1])
    assert np.array_equal(mine["lists/sums_deep"][0], mine["lists/sums"][0])


def test_street_target_at_the_bench_poses(mine, old_order, orc):
    """20 k-point street target, 2 k-point scan at the poses of its own Gauss-Newton trajectory: search + reduce, the fused
    kernel, nn_query and align (host and device loops)"""
    target, normals, scan = xc.street_case()
    assert bool(mine["street/x_ordered"]) and not bool(mine["street/heavy"]) and not bool(old_order["street/x_ordered"])
    assert mine["street/poses"].shape[0] == 5
    for k in range(5):
        d, i = orc.nn_brute(target, mine[f"street/nn_q{k}"])
        assert np.array_equal(mine[f"street/nn_i{k}"], i), k
        assert np.array_equal(mine[f"street/nn_d{k}"], d), k
    _same_as_old(mine, old_order, "street")


def test_heavy_target_keeps_its_order(mine, old_order, orc):
    """a LiDAR sweep has heavy cells: Morton order and leaf / group boxes, no x order, and nothing moves"""
    target, normals, scan = xc.heavy_case()
    assert bool(mine["heavy/heavy"]) and not bool(mine["heavy/x_ordered"])
    d, i = orc.nn_brute(target, mine["heavy/nn_q0"])
    assert np.array_equal(mine["heavy/nn_i0"], i) and np.array_equal(mine["heavy/nn_d0"], d)
    _same_as_old(mine, old_order, "heavy")
