"""Fast global registration without a GPU: the NumPy restatement of tests/fgr_cases.py recovers the truth on the shared cases
(the condition under which the GPU tests against it mean anything), the tuple multiplicities equal a brute-force loop, the
Python layer refuses bad arguments before any device call, and header, bindings and ABI version stand together."""
import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import fgr_cases as fc

PUBLIC = dict(n_tuples=60_000, seed=0)          # the public-call case of tests/test_gpu_fgr.py: case B, seed 0


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_recovers_the_truth(name, seed):
    c, r = fc.case(name, seed), fc.reference(name, seed)
    ang, dt = fc.pose_error(r["T"], c["T_true"])
    w = r["weights"]
    print(f"case {name} seed {seed}: status {r['status']}, {r['iterations']} iterations, mu {r['mu']:.4g}, {ang:.2e} deg, {dt:.4f} m, "
          f"smallest inlier weight {w[c['inlier']].min():.4f}, largest outlier weight {w[~c['inlier']].max():.4f}")
    assert r["status"] == 0 and r["iterations"] == fc.SCHEDULE["max_iter"]
    assert ang <= 0.05 and dt <= 0.1
    assert w[c["inlier"]].min() > 0.99                       # every inlier weight rounds to 1.00


def test_schedule_and_trace():
    r = fc.reference("A", 0)
    mu, mu_min = fc.case("A", 0)["mu0"], fc.MAX_DIST ** 2
    for it in range(fc.SCHEDULE["max_iter"]):
        assert r["trace"][it, 45] == mu
        mu = fc.schedule(mu, it, mu_min, fc.SCHEDULE["division"], fc.SCHEDULE["period"])
    assert r["mu"] == mu
    assert fc.schedule(1.0, 3, 0.9, 1.4, 4) == 0.9 and fc.schedule(1.0, 2, 0.9, 1.4, 4) == 1.0 and fc.schedule(0.9, 3, 0.9, 1.4, 4) == 0.9


def test_exactly_singular_systems():
    """One and two matches leave H rank-deficient; with integer coordinates, q = p and T = I every weight is 1 and the
    elimination is exact, so the pivot is exactly 0: status 2 at the first pass, T untouched.  (Generic coordinates leave a
    pivot of rounding size instead, and the loop runs on.)"""
    pts = np.float32([[1, 2, 3], [4, -1, 2]])
    for m in (1, 2):
        r = fc.fgr_numpy(pts[:m], pts[:m], np.eye(4), 100.0, 0.01, 1.4, 4, 8)
        assert r["status"] == 2 and r["iterations"] == 1 and np.array_equal(r["T"], np.eye(4))


def test_step_is_the_left_update():
    """Exact matches under a large rotation: the loop converges from the identity (the local aligners' right update diverges)."""
    from point_cloud_registration_amd.math_tools import expSO3
    rng = np.random.default_rng(5)
    src = rng.uniform(-20, 20, (50, 3)).astype(np.float32)
    R, t = expSO3(np.array([1.5, -1.0, 0.8])), np.array([3.0, -8.0, 5.0])
    dst = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    r = fc.fgr_numpy(src, dst, np.eye(4), 1e4, 1e-4, 1.4, 4, 40)
    assert np.abs(r["T"][:3, :3] - R).max() < 1e-5 and np.abs(r["T"][:3, 3] - t).max() < 1e-4


@pytest.mark.parametrize("m, n_tuples, scale, min_edge", [(3, 50, 0.9, 0.0), (40, 700, 0.9, 0.0), (40, 700, 0.5, 3.0), (2, 10, 0.9, 0.0)])
def test_multiplicities_equal_a_brute_force_loop(m, n_tuples, scale, min_edge):
    import ransac_cases as rc
    src, dst = rc.random_pairs(m, seed=40 + m, inlier_share=0.7)
    got, want = fc.tuple_mult(src, dst, n_tuples, 3, scale, min_edge), fc.tuple_mult_loop(src, dst, n_tuples, 3, scale, min_edge)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    assert got[0].sum() == 3 * got[1]
    if m == 40:
        assert 0 < got[1] < n_tuples                         # the case has tuples of either kind


def test_public_call_restated():
    """What tests/test_gpu_fgr.py asks of fgr_pose on case B, checked on the restatement first: the pose, the fitness and
    that the refinement leaves no true inlier outside max_dist."""
    c = fc.case("B", PUBLIC["seed"])
    T, info = fc.fgr_pose_numpy(c["src"], c["dst"], fc.MAX_DIST, c["mu0"], PUBLIC["n_tuples"], seed=PUBLIC["seed"])
    ang, dt = fc.pose_error(T, c["T_true"])
    print(f"{info['n_valid']} valid tuples, {np.count_nonzero(info['mult'])} rows kept, {ang:.2e} deg, {dt:.4f} m, fitness {info['fitness']:.4f}, "
          f"true inliers outside max_dist: {int((c['inlier'] & ~info['inliers']).sum())}")
    assert ang <= 0.05 and dt <= 0.1 and info["fitness"] >= 0.19
    assert not (c["inlier"] & ~info["inliers"]).any()


def test_refusals_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_capi, "get_context", no_device)
    c = fc.case("A", 0)
    src, dst = c["src"], c["dst"]
    rows = np.arange(len(src))
    with pytest.raises(ValueError):
        pcr.fgr_pose(src[:, :2], dst, rows, rows, 0.05)
    with pytest.raises(ValueError):
        pcr.fgr_pose(src, dst, rows, rows[:-1], 0.05)
    with pytest.raises(ValueError):
        pcr.fgr_pose(src, dst, rows.astype(np.float64), rows, 0.05)
    for bad in (1.0, 0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            pcr.fgr_pose(src, dst, rows, rows, 0.05, division_factor=bad)
    for kw in (dict(period=0), dict(iterations=-1), dict(mu0=0.0), dict(mu0=np.inf), dict(refine_rounds=-1), dict(init_T=np.eye(3)),
               dict(tuple_scale=1.5), dict(n_tuples=-1), dict(min_edge=-1.0), dict(seed=-1)):
        with pytest.raises(ValueError):
            pcr.fgr_pose(src, dst, rows, rows, 0.05, **kw)
    for md in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            pcr.fgr_pose(src, dst, rows, rows, md)
    with pytest.raises(ValueError):
        pcr.register_global(src, dst, 1.0, 0.05, method="icp")
    with pytest.raises(ValueError):
        pcr.register_global(src, dst, 1.0, 0.05, method=None)
    with pytest.raises(ValueError):
        _capi.fgr_linearize(no_device, src, dst, np.eye(4), 1.0, mult=-np.ones(len(src), np.int32))
    with pytest.raises(ValueError):
        _capi.fgr_linearize(no_device, src, dst, np.eye(4), -1.0)


def test_empty_calls_need_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_capi, "get_context", no_device)
    none = np.zeros((0, 3), np.float32)
    T, info = pcr.fgr_pose(none, none, [], [], 0.05, return_info=True)
    assert np.array_equal(T, np.eye(4)) and info["count"] == 0 and info["fitness"] == 0.0 and info["n_valid"] == 0
    two = np.float32([[0, 0, 0], [1, 0, 0]])
    T, info = pcr.fgr_pose(two, two, [0, 1], [0, 1], 0.05, return_info=True)          # fewer than 3 rows: ransac_pose's no-match result
    assert np.array_equal(T, np.eye(4)) and info["count"] == 0 and not info["inliers"].any()


def test_prototypes_and_abi_version():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcr.h")).read()
    for name in ("pcr_fgr_linearize", "pcr_fgr_pose", "pcr_fgr_tuples", "pcr_fgr_blocks"):
        assert name in _capi.PROTOTYPES and re.search(rf"PCR_API\s+[\w\s\*]+?\b{name}\s*\(", header)
    assert _capi.ABI_VERSION == 5 and re.search(r"#define\s+PCR_ABI_VERSION\s+5\b", header)
    assert len(_capi.PROTOTYPES["pcr_fgr_pose"][1]) == 19 and len(_capi.PROTOTYPES["pcr_fgr_linearize"][1]) == 9
    assert (_capi.FGR_TILE, _capi.FGR_WIDTH, _capi.FGR_TRACE) == tuple(
        int(re.search(rf"#define\s+{k}\s+(\d+)", header).group(1)) for k in ("PCR_FGR_TILE", "PCR_FGR_WIDTH", "PCR_FGR_TRACE"))
