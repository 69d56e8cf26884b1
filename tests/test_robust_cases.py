"""The robust kernels without a GPU: the weight table of include/pcr.h as math_tools.robust_weight states it, the constructors'
refusals, and the end-to-end case of tests/robust_cases.py through the restated Gauss-Newton loop."""

import numpy as np
import pytest

import robust_cases as rc

C = 0.75
C2 = C * C
BELOW, ABOVE = np.nextafter(C2, 0.0), np.nextafter(C2, np.inf)


def rw(kind, s, scale=C):
    from point_cloud_registration_amd import robust_weight
    return robust_weight(kind, s, scale)


def test_exported():
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd import math_tools
    assert "robust_weight" in pcr.__all__ and pcr.robust_weight is math_tools.robust_weight


def test_weight_table_pinned():
    """s = 0, just below, at and just above c2, and 1e300: the values of the table, written out."""
    s = np.array([0.0, BELOW, C2, ABOVE, 1e300])
    assert np.array_equal(rw("huber", s), [1.0, 1.0, 1.0, C / np.sqrt(ABOVE), C / 1e150])
    assert np.array_equal(rw("cauchy", s), [1.0, 1.0 / (1.0 + BELOW / C2), 0.5, 1.0 / (1.0 + ABOVE / C2), 1.0 / (1.0 + 1e300 / C2)])
    assert np.array_equal(rw("tukey", s), [1.0, (1.0 - BELOW / C2) ** 2, 0.0, 0.0, 0.0])
    assert np.array_equal(rw("gm", s), [1.0, (C2 / (C2 + BELOW)) ** 2, 0.25, (C2 / (C2 + ABOVE)) ** 2, (C2 / (C2 + 1e300)) ** 2])
    for kind in rc.KINDS:
        w = rw(kind, s)
        assert w.dtype == np.float64 and np.all((0.0 <= w) & (w <= 1.0)) and w[-1] < 1e-100
        assert np.array_equal(w, rc.weight(kind, s, C))                      # the restatement the GPU tests use
        assert rw(kind, np.inf) == 0.0 and float(rw(kind, 0.3)) == float(rw(kind, np.array([0.3]))[0])
    assert np.array_equal(rw(None, np.array([0.0, 1e300, np.inf])), [1.0, 1.0, 0.0])


@pytest.mark.parametrize("kind", rc.KINDS)
def test_continuous_at_c2(kind):
    """One ulp of s on either side of c2 moves no weight by more than a few ulps of 1: no jump where the branch is."""
    w = rw(kind, np.array([BELOW, C2, ABOVE]))
    assert np.all(np.abs(np.diff(w)) <= 4 * 2.0 ** -52), w
    assert np.all(np.diff(w) <= 0.0)                                         # and no kernel rises


def test_scale_and_kind_refusals():
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e200, 1e-200):
        with pytest.raises(ValueError):
            rw("huber", 1.0, bad)
    with pytest.raises(ValueError):
        rw("welsch", 1.0)


def test_constructors_refuse_before_any_device_call():
    """ValueError from the constructor itself: no target, no context, no GPU needed."""
    import point_cloud_registration_amd as pcr
    for cls in (pcr.GICP, pcr.VGICP, pcr.SymmetricICP, pcr.ColoredICP):
        with pytest.raises(ValueError, match="robust must be"):
            cls(robust="welsch")
        with pytest.raises(ValueError, match="robust must be"):
            cls(robust=1)
        for bad in (0.0, -0.5, float("nan"), float("inf"), 1e200):
            with pytest.raises(ValueError, match="robust_scale"):
                cls(robust="tukey", robust_scale=bad)
        reg = cls(robust="gm", robust_scale=0.25)
        assert (reg.robust, reg.robust_scale) == ("gm", 0.25)
        plain = cls()
        assert plain.robust is None and plain._robust is None
        # the stubs stay
        for call in (reg.linearize, reg.coreset, reg.align_batch, reg.calc_H_g_e2_batch):
            with pytest.raises(NotImplementedError):
                call()


@pytest.fixture(scope="module")
def case():
    return rc.e2e_case()


def test_case_as_described(case):
    assert case["scan"].shape == (1024, 3) and case["target"].shape == (4096, 3)
    assert 0.29 < case["moved"].mean() < 0.31
    assert 0.2 < np.linalg.norm(rc.E2E_SHIFT) < 0.4 < rc.E2E_MAX_DIST
    assert np.linalg.norm(case["T_true"] - np.eye(4)) < 0.1
    assert len(case["means"]) > 100


def test_huge_scale_is_weight_one(case):
    """scale = 1e150: c2 = 1e300 is finite and every s of the cases is far below it -- all four kernels return exactly 1."""
    for family in ("symm", "color", "gicp", "vgicp"):
        plain = rc.e2e_terms(family, case, np.eye(4), None, 1.0)
        s = plain[:, 27]
        assert np.any(s > 0)
        for kind in rc.KINDS:
            assert np.all(rw(kind, s, 1e150) == 1.0), (family, kind)
            assert np.array_equal(rc.e2e_terms(family, case, np.eye(4), kind, 1e150), plain)


@pytest.mark.parametrize("family", ["symm", "color", "gicp", "vgicp"])
def test_end_to_end(case, family):
    """The restated loop on the case: the kernel brings the translation at least a factor 2 closer to the truth (a condition on
    the chosen input), and the errors are the ones robust_cases.E2E_ERRORS records for the GPU tests."""
    Tp, ip = rc.gn_loop(family, case, None, 1.0)
    Tr, ir = rc.gn_loop(family, case, rc.E2E_KIND, rc.E2E_SCALE[family])
    ep, er = rc.t_err(Tp, case), rc.t_err(Tr, case)
    print(f"{family}: plain |dt| {ep:.4e} after {ip} iterations, {rc.E2E_KIND} |dt| {er:.4e} after {ir}")
    assert ip < 30 and ir < 30
    assert er <= ep / 2.0
    rec_p, rec_r = rc.E2E_ERRORS[family]
    assert abs(ep - rec_p) <= 1e-3 * rec_p and abs(er - rec_r) <= 1e-3 * rec_r
