"""Radius and hybrid neighbourhoods: the interface, its defaults and its refusals.  Needs no GPU."""

import inspect

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

NEW_ENTRY_POINTS = {"pcr_target_ball_moments": 6, "pcr_target_estimate_normals_radius": 5, "pcr_scan_estimate_normals_radius": 5,
                    "pcr_target_estimate_covariances_radius": 7, "pcr_scan_estimate_covariances_radius": 7}


@pytest.fixture()
def no_gpu(monkeypatch):
    """Any attempt to reach the library or a context fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", refuse)
    monkeypatch.setattr(_capi, "get_context", refuse)


def test_names_and_defaults():
    assert "ball_moments" in pcr.__all__ and callable(pcr.ball_moments)
    p = inspect.signature(pcr.ball_moments).parameters
    assert list(p) == ["points", "radius", "max_nn"] and p["max_nn"].default is None
    for fn in (pcr.estimate_normals, pcr.estimate_norm_with_tree):
        p = inspect.signature(fn).parameters
        assert list(p)[-5:] == ["k", "compat", "radius", "max_nn", "return_counts"]
        assert (p["k"].default, p["compat"].default, p["radius"].default, p["max_nn"].default, p["return_counts"].default) == \
            (15, True, None, None, False)
    p = inspect.signature(pcr.PlaneICP.__init__).parameters
    assert p["normal_radius"].default is None and p["normal_max_nn"].default is None and p["k"].default == 15
    p = inspect.signature(pcr.registration.MatchPass.__init__).parameters
    assert (p["k"].default, p["radius"].default, p["max_nn"].default) == (10, None, None)
    for name in ("ball_moments", "estimate_normals_radius", "estimate_covariances_radius"):
        assert callable(getattr(_capi.Target, name))
    for name in ("estimate_normals_radius", "estimate_covariances_radius"):
        assert callable(getattr(_capi.Scan, name))


def test_prototypes():
    for name, n_args in NEW_ENTRY_POINTS.items():
        assert name in _capi.PROTOTYPES, name
        assert len(_capi.PROTOTYPES[name][1]) == n_args


def test_check_ball():
    assert _capi.check_ball(0.5, None) == (0.5, 0) and _capi.check_ball(0, 0) == (0.0, 0)
    assert _capi.check_ball(np.float32(1.0), np.int64(64)) == (1.0, 64)
    for r in (-1e-30, -1.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="radius"):
            _capi.check_ball(r, None)
    for m in (-1, 65, 2.5, 1000):
        with pytest.raises(ValueError, match="max_nn"):
            _capi.check_ball(0.5, m)
    with pytest.raises(ValueError, match="max_nn needs a radius"):
        _capi.check_ball(None, 3)


def test_bad_arguments_are_refused_before_the_gpu(no_gpu):
    pts = np.random.default_rng(0).uniform(-1, 1, (8, 3)).astype(np.float32)
    target = _capi.Target.__new__(_capi.Target)
    scan = _capi.Scan.__new__(_capi.Scan)
    bad = [(r, None) for r in (-1.0, np.nan, np.inf)] + [(0.5, -1), (0.5, 65), (None, 3)]
    for r, m in bad:
        with pytest.raises(ValueError):
            pcr.ball_moments(pts, r, m)
        with pytest.raises(ValueError):
            pcr.estimate_normals(pts, radius=r, max_nn=m)
        with pytest.raises(ValueError):
            pcr.estimate_norm_with_tree(pts, None, radius=r, max_nn=m)
        with pytest.raises(ValueError):
            pcr.PlaneICP(normal_radius=r, normal_max_nn=m)
        for cls in (pcr.GICP, pcr.VGICP, pcr.SymmetricICP, pcr.ColoredICP):
            with pytest.raises(ValueError):
                cls(radius=r, max_nn=m)
        for obj in (target, scan):
            with pytest.raises(ValueError):
                obj.estimate_normals_radius(r, m)
            with pytest.raises(ValueError):
                obj.estimate_covariances_radius(r, m)
        with pytest.raises(ValueError):
            target.ball_moments(r, m)
    with pytest.raises(ValueError, match="max_nn needs a radius"):
        pcr.estimate_normals(pts, max_nn=30)
    with pytest.raises(ValueError, match="shape"):
        pcr.ball_moments(np.zeros((4, 2), np.float32), 0.5)


def test_a_ball_runs_on_one_gpu_of_one_process(no_gpu):
    for kw in ({"devices": [0, 1]}, {"comm": object()}):
        with pytest.raises(NotImplementedError, match="does not support"):
            pcr.PlaneICP(normal_radius=0.5, **kw)
        for cls in (pcr.GICP, pcr.VGICP, pcr.SymmetricICP, pcr.ColoredICP):
            with pytest.raises(NotImplementedError, match="does not support"):
                cls(radius=0.5, max_nn=30, **kw)
            with pytest.raises(ValueError):                  # (without a ball: the refusal these classes always gave)
                cls(**kw)


def test_the_aligners_remember_their_neighbourhood(no_gpu):
    a = pcr.GICP(radius=0.5, max_nn=30)
    assert (a.radius, a.max_nn, a.k) == (0.5, 30, 10) and a._neighbourhood() == ("ball", 0.5, 30)
    assert pcr.SymmetricICP(radius=1)._neighbourhood() == ("ball", 1.0, 0)
    b = pcr.GICP(k=12)
    assert (b.radius, b.max_nn) == (None, None) and b._neighbourhood() == ("k", 12)
    assert a._neighbourhood() != pcr.GICP(radius=0.5)._neighbourhood() != b._neighbourhood()
    p = pcr.PlaneICP(normal_radius=0.25, normal_max_nn=16)
    assert p._normal_ball == (0.25, 16) and pcr.PlaneICP()._normal_ball is None


def test_no_gpu_behaviour_of_the_bindings_is_unchanged():
    """Without a GPU the library still loads and every new symbol resolves; nothing new runs at import."""
    import os
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("the library is not built")
    L = _capi.lib()
    for name in NEW_ENTRY_POINTS:
        assert getattr(L, name).argtypes == _capi.PROTOTYPES[name][1]
    if not os.path.exists("/dev/kfd"):
        assert _capi.device_count() == 0
        with pytest.raises((_capi.PcrError, ValueError)):
            pcr.estimate_normals(np.zeros((10, 3), np.float32), radius=1.0)      # no silent CPU path
        with pytest.raises((_capi.PcrError, ValueError)):
            pcr.ball_moments(np.zeros((10, 3), np.float32), 1.0)
