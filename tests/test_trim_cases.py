"""The adaptive pass without a GPU: math_tools.trim_threshold against known answers, the restatement of tests/trim_cases.py,
the refusals that happen before any device call, and the end-to-end case through the restated adaptive loop."""

import numpy as np
import pytest

import robust_cases as rc
import trim_cases as tc


def tt(s, ratio):
    from point_cloud_registration_amd import trim_threshold
    return trim_threshold(s, ratio)


def test_exported():
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd import math_tools
    assert "trim_threshold" in pcr.__all__ and pcr.trim_threshold is math_tools.trim_threshold


def test_trim_threshold_known_answers():
    s = np.array([5.0, 1.0, np.inf, 3.0, 2.0, 4.0, np.inf])                 # m = 5
    assert tt(s, 1.0) == (5.0, 5)
    assert tt(s, 0.6) == (3.0, 3)
    assert tt(s, 0.59) == (2.0, 2)                                          # floor(2.95)
    assert tt(s, 0.2) == (1.0, 1) and tt(s, 0.01) == (1.0, 1)               # max(1, .)
    assert tt(s.reshape(7, 1), 0.6) == (3.0, 3)
    # ties at tau: the threshold is the tied value, and s <= tau keeps all of them -- more than k
    s = np.array([2.0, 1.0, 2.0, 2.0, 7.0, 2.0])
    tau, k = tt(s, 0.5)
    assert (tau, k) == (2.0, 3) and np.sum(s <= tau) == 5
    # zeros, a denormal, NaN as outside
    s = np.array([0.0, 5e-324, np.nan, 0.0, np.inf])
    assert tt(s, 1.0) == (5e-324, 3) and tt(s, 0.5) == (0.0, 1)
    # nothing
    assert tt(np.array([np.inf, np.inf]), 0.5) == (np.inf, 0) and tt(np.array([]), 1.0) == (np.inf, 0)
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            tt(s, bad)


def test_restatement_agrees_with_trim_threshold():
    rng = np.random.default_rng(5)
    s = rng.lognormal(0.0, 3.0, 1000)
    s[rng.random(1000) < 0.2] = np.inf
    for q in (1e-4, 0.25, 0.5, 0.6, 0.999, 1.0):
        tau, k, m, n_le = tc.threshold(s, q)
        assert (tau, k) == tt(s, q) and m == np.sum(np.isfinite(s)) and n_le == k      # (distinct values: no ties)
        assert k == tc.rank(q, m) == max(1, int(q * m))


def test_key_and_trim_mask():
    """ColoredICP: kappa = s_G + s_C, one decision for both rows; ties at tau are all kept."""
    s = np.array([[1.0, 2.0], [0.5, 0.25], [np.inf, np.inf], [3.0, 0.0], [0.25, 0.5], [4.0, 4.0]])
    assert np.array_equal(tc.key(s), [3.0, 0.75, np.inf, 3.0, 0.75, 8.0])
    w, stats, m = tc.weights("trim", s, 0.8)                               # m = 5, k = 4: tau = 3, both 3s in
    assert m == 5 and np.array_equal(stats, [3.0, 0.0, 4.0, 4.0])
    assert np.array_equal(w, [[1, 1], [1, 1], [0, 0], [1, 1], [1, 1], [0, 0]])
    w, stats, m = tc.weights("trim", s, 0.2)                               # k = 1: tau = 0.75, tied: kept 2 > k
    assert np.array_equal(stats, [0.75, 0.0, 2.0, 1.0]) and w.sum() == 4
    w, stats, m = tc.weights("trim", np.full((3, 2), np.inf), 0.5)
    assert m == 0 and not w.any() and np.array_equal(stats, [np.inf, 0.0, 0.0, 0.0])


def test_scale_from_tau_and_the_limit():
    s = np.array([0.04, 0.01, 0.09, np.inf, 0.16])
    for kind in rc.KINDS:
        w, stats, m = tc.weights(kind, s, 0.5, 3.0)                        # m = 4, k = 2: tau = 0.04
        c = 3.0 * np.sqrt(0.04)
        assert m == 4 and np.array_equal(stats, [0.04, c, 2.0, 2.0])
        assert np.array_equal(w[:, 0], rc.weight(kind, s, c)) and w[3, 0] == 0.0
        # tau = 0 (more than half of the keys are exactly 0): c2 is not > 0, the limit for c -> 0
        z = np.array([0.0, 0.0, 0.3, 0.0, np.inf, 1e-300])
        w, stats, m = tc.weights(kind, z, 0.5, 3.0)
        assert np.array_equal(stats, [0.0, 0.0, 3.0, 2.0])
        assert np.array_equal(w[:, 0], [1.0, 1.0, 0.0, 1.0, 0.0, 0.0]) and np.all(np.isfinite(w))
        # underflow: tau > 0 but c * c == 0
        u = np.array([1e-320, 2e-320, 1.0])
        w, stats, m = tc.weights(kind, u, 0.5, 1e-10)
        assert stats[0] == 1e-320 and stats[1] > 0.0 and stats[1] * stats[1] == 0.0 and not w.any()


def test_refusals_before_any_device_call():
    """check_adaptive states the library's rule: ValueError without a context or a GPU."""
    from point_cloud_registration_amd import _capi
    assert _capi.check_adaptive("trim", 0.6) == (5, 0.6, 1.0)
    assert _capi.check_adaptive("trim", 1.0, float("nan")) == (5, 1.0, pytest.approx(float("nan"), nan_ok=True))     # (not read)
    assert _capi.check_adaptive("tukey", 0.5, 3.0) == (3, 0.5, 3.0)
    for kind, q, f in (("welsch", 0.5, 1.0), (None, 0.5, 1.0), (5, 0.5, 1.0), ("trim", 0.0, 1.0), ("trim", -0.5, 1.0), ("trim", 1.5, 1.0),
                       ("trim", float("nan"), 1.0), ("huber", 0.5, 0.0), ("huber", 0.5, -1.0), ("gm", 0.5, float("inf")),
                       ("cauchy", 0.5, float("nan")), ("tukey", 0.0, 3.0)):
        with pytest.raises(ValueError):
            _capi.check_adaptive(kind, q, f)
    assert _capi.ROBUST_TRIM == 5 and _capi.ADAPTIVE_KINDS == tc.KIND_ID


@pytest.fixture(scope="module")
def case():
    return rc.e2e_case()


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_ratio_one_is_the_plain_pass(case, family):
    """A trim at ratio 1 keeps every correspondence: the restated plain terms, and so the recorded plain error."""
    plain = rc.e2e_terms(family, case, np.eye(4), None, 1.0)
    got, stats = tc.e2e_pass(family, case, np.eye(4), "trim", 1.0)
    assert np.array_equal(got, plain) and stats[2] == stats[3] > 0
    T, it = tc.gn_loop(family, case, "trim", 1.0)
    e = rc.t_err(T, case)
    print(f"{family}: trim at 1.0 |dt| {e:.4e} after {it} iterations (recorded plain {rc.E2E_ERRORS[family][0]:.4e})")
    assert abs(e - rc.E2E_ERRORS[family][0]) <= 1e-3 * rc.E2E_ERRORS[family][0]


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_end_to_end(case, family):
    """The restated adaptive loop on the case: both schemes end closer to the truth than the hand-tuned Cauchy scale did, and the
    errors are the ones trim_cases.ADAPTIVE_ERRORS records for the GPU tests."""
    for (kind, q, factor), rec in zip((tc.E2E_TRIM, tc.E2E_TUKEY), tc.ADAPTIVE_ERRORS[family]):
        T, it = tc.gn_loop(family, case, kind, q, factor)
        e = rc.t_err(T, case)
        print(f"{family}: {kind} q {q} factor {factor}: |dt| {e:.4e} after {it} iterations (recorded {rec:.4e})")
        assert it < 30
        assert e < rc.E2E_ERRORS[family][1]
        assert abs(e - rec) <= 1e-3 * rec
