"""The wave fold of the 32 block partials (pass_device.h: wave_fold32 -- lane swaps and DPP moves instead of LDS shuffles)
returns the bits it returned before: every case of tests/fold_cases.py against tests/golden/g17_fold_bits.npz, which
tools/make_golden_fold_bits.py recorded with the library of the commit in front of that change (the __shfl_xor fold).

`==` on all 29 values of every case: the four kinds through the split and the fused path on scans of 1 ... 20 000 points, a
scan without a match, one with a NaN point (NaN sums, if any, in the same places), one linearize_batch and one GICP pass (the
match-list reduce of match_pass.h folds with the same function)."""
import numpy as np
import pytest

import fold_cases as fc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def golden():
    return load_golden("g17_fold_bits.npz")


@pytest.fixture(scope="module")
def mine(capi):
    return fc.run_all(capi, capi.get_context(0))


def test_the_fixture_holds_every_case(capi, golden, mine):
    assert sorted(golden) == sorted(mine)
    names = [f"{k}/{s}" for k, _ in fc.kinds(capi) for s in list(map(str, fc.SIZES)) + ["far", "nan"]]
    assert set(names) | {"batch/plane", "gicp/2049"} == set(golden)
    # the cases are not empty: the point kinds match nearly every point, the voxel kinds a good part; the far scan nothing
    for k, _ in fc.kinds(capi):
        counts = [golden[f"{k}/{n}"][:, 28] for n in fc.SIZES]
        print(k, [tuple(c) for c in counts])
        assert (counts[-1] > (18_000 if k in ("icp", "plane") else 2_000)).all()
        assert all((c <= n).all() for c, n in zip(counts, fc.SIZES))
        assert not golden[f"{k}/far"].any()


@pytest.mark.parametrize("kind", ["icp", "plane", "vplane", "ndt"])
def test_linearize_bits(kind, golden, mine):
    for s in list(map(str, fc.SIZES)) + ["far"]:
        name = f"{kind}/{s}"
        assert mine[name].shape == (2, 29)
        assert np.array_equal(mine[name], golden[name]), name             # split and fused, all 29 values


@pytest.mark.parametrize("kind", ["icp", "plane", "vplane", "ndt"])
def test_nan_point_bits(kind, golden, mine):
    name = f"{kind}/nan"
    assert fc.same_bits(mine[name], golden[name]), name


def test_batch_and_gicp_bits(golden, mine):
    assert np.array_equal(mine["batch/plane"], golden["batch/plane"])
    assert mine["batch/plane"].shape[-1] == 29 and (mine["batch/plane"][:, 28] > 0).all()
    assert np.array_equal(mine["gicp/2049"], golden["gicp/2049"]) and mine["gicp/2049"][28] > 1000
