"""The direct VGICP unit behind the host scaffold of the match-list passes (csrc/match_pass.h: DirectUnit<NB>, the one place
that launches a fold) returns the bits it returned as a driver of its own, and so do the four units whose launches moved with
it: every case of tests/direct_bits_cases.py against tests/golden/g18_direct_bits.npz, which tools/make_golden_direct_bits.py
recorded on an MI355X with the library of the commit in front of that change.

`==` on every value: the 29 sums of pcr_vgicp_direct_linearize (two kinds of voxel covariances, 1 / 7 / 27 voxels, gates 0.8 and
2.0, scans of 0 ... 2000 points, plain and under Cauchy(1) and Tukey(1)), the residuals of a 257-point scan, T, the iteration
count and every trace row of a five-iteration align, the target with no kept voxel, and one plain, one robust and two
adaptive passes (sums and stats) of GICP, VGICP, SymmetricICP and ColoredICP.  The bits depend on the device through the grid of
the reduce (choose_blocks), as those of g17_fold_bits.npz do."""
import numpy as np
import pytest

import direct_bits_cases as db
from conftest import load_golden
from test_gpu_direct import PAIRS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def golden():
    return load_golden("g18_direct_bits.npz")


@pytest.fixture(scope="module")
def mine(capi, g2):
    return db.run_all(capi, capi.get_context(0), g2)


def test_the_fixture_holds_every_case(golden, mine):
    assert sorted(golden) == sorted(mine)
    names = {f"linearize/{c}/{nb}/{g}" for c in db.COVS for nb in db.NEIGHBORS for g in db.GATES}
    names |= {f"residuals/plane/{nb}" for nb in db.NEIGHBORS} | {f"align/plane/{nb}/{k}" for nb in db.NEIGHBORS for k in ("plain", "cauchy")}
    names |= {f"empty/{what}/{nb}" for what in ("linearize", "residuals") for nb in db.NEIGHBORS}
    names |= {f"unit/{u}/{what}" for u in db.UNITS for what in ("linearize", "robust", "adaptive/trim", "adaptive/huber")}
    assert names == set(golden)
    # the cases are not empty: the whole scan keeps the pairs tests/test_gpu_direct.py pins, under every kernel, and every scan
    # with points keeps some
    full, first = db.PREFIXES.index(2000), db.PREFIXES.index(0) + 1
    for c in db.COVS:
        for nb in db.NEIGHBORS:
            for g in db.GATES:
                lin = golden[f"linearize/{c}/{nb}/{g}"]
                assert lin.shape == (len(db.PREFIXES), len(db.KERNELS), 29)
                assert (lin[full, :, 28] == PAIRS[g][nb]).all()
                assert (lin[first:, :, 28] > 0).all() and not lin[0].any()
    for nb in db.NEIGHBORS:
        res = golden[f"residuals/plane/{nb}"]
        assert res.shape == (db.RESIDUALS_AT, nb) and np.isfinite(res).sum() == golden[f"linearize/plane/{nb}/{db.RESIDUALS_GATE}"][-2, 0, 28]
        for k in ("plain", "cauchy"):
            al = golden[f"align/plane/{nb}/{k}"]
            assert al[16] == db.ALIGN_ITERATIONS and al.shape == (17 + 45 * db.ALIGN_ITERATIONS,)
            assert (al[17:].reshape(-1, 45)[:, 44] > 0).all()
        assert not golden[f"empty/linearize/{nb}"].any() and np.isposinf(golden[f"empty/residuals/{nb}"]).all()
    for u in db.UNITS:
        for what in ("linearize", "robust", "adaptive/trim", "adaptive/huber"):
            assert golden[f"unit/{u}/{what}"][28] > 1000, (u, what)


@pytest.mark.parametrize("nb", db.NEIGHBORS)
@pytest.mark.parametrize("cov", db.COVS)
def test_linearize_bits(golden, mine, cov, nb):
    for g in db.GATES:
        name = f"linearize/{cov}/{nb}/{g}"
        assert np.array_equal(mine[name], golden[name]), name


@pytest.mark.parametrize("nb", db.NEIGHBORS)
def test_residuals_align_and_empty_target_bits(golden, mine, nb):
    for name in (f"residuals/plane/{nb}", f"align/plane/{nb}/plain", f"align/plane/{nb}/cauchy", f"empty/linearize/{nb}", f"empty/residuals/{nb}"):
        assert np.array_equal(mine[name], golden[name]), name


@pytest.mark.parametrize("unit", db.UNITS)
def test_match_unit_bits(golden, mine, unit):
    for what in ("linearize", "robust", "adaptive/trim", "adaptive/huber"):
        name = f"unit/{unit}/{what}"
        assert mine[name].shape == (33 if "adaptive" in what else 29,)
        assert np.array_equal(mine[name], golden[name]), name
