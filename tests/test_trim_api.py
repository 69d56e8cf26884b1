"""The adaptive pass at the public interface, without a GPU: what the constructors of GICP, VGICP, SymmetricICP and ColoredICP
take and refuse, and the nine new names in the header, the library and the binding."""

import os
import re
import subprocess

import pytest

from conftest import REPO

NAMES = ["pcr_order_statistic"] + [f"pcr_{u}_{f}_adaptive" for u in ("gicp", "vgicp", "symm", "color") for f in ("linearize", "align")]


def classes():
    import point_cloud_registration_amd as pcr
    return pcr.GICP, pcr.VGICP, pcr.SymmetricICP, pcr.ColoredICP


def test_constructors():
    for cls in classes():
        plain = cls()
        assert plain.trim is None and plain._adaptive is None and plain._robust is None and plain.last_adaptive is None
        fixed = cls(robust="tukey", robust_scale=0.25)
        assert fixed._adaptive is None and fixed._robust == (3, 0.25)                    # (what it was)
        reg = cls(trim=0.6)
        assert reg.trim == 0.6 and reg._adaptive == (5, 0.6, 1.0) and reg._robust is None and reg.robust is None
        assert cls(trim=1)._adaptive == (5, 1.0, 1.0)
        reg = cls(robust="tukey", robust_scale=("quantile", 0.5, 3))
        assert reg._adaptive == (3, 0.5, 3.0) and reg._robust is None and reg.robust == "tukey" and reg.robust_scale == ("quantile", 0.5, 3)
        assert cls(robust="huber", robust_scale=["quantile", 1.0, 1.5])._adaptive == (1, 1.0, 1.5)


def test_constructors_refuse_before_any_device_call():
    for cls in classes():
        for bad in (0.0, -0.2, 1.01, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="quantile"):
                cls(trim=bad)
        with pytest.raises(ValueError, match="exclude"):
            cls(trim=0.6, robust="huber", robust_scale=0.1)
        with pytest.raises(ValueError, match="exclude"):
            cls(trim=0.6, robust="huber", robust_scale=("quantile", 0.5, 3.0))
        for bad in (("quantile", 0.5), ("quantile", 0.5, 3.0, 1.0), ("median", 0.5, 3.0), (0.5, 3.0, "quantile"), (), ("quantile", None, 3.0),
                    ("quantile", 0.5, "x")):
            with pytest.raises(ValueError, match="robust_scale"):
                cls(robust="cauchy", robust_scale=bad)
        for q, f in ((0.0, 3.0), (1.5, 3.0), (float("nan"), 3.0), (0.5, 0.0), (0.5, -3.0), (0.5, float("inf")), (0.5, float("nan"))):
            with pytest.raises(ValueError):
                cls(robust="cauchy", robust_scale=("quantile", q, f))
        with pytest.raises(ValueError, match="robust_scale"):                          # a quantile of nothing: no kernel
            cls(robust_scale=("quantile", 0.5, 3.0))
        with pytest.raises(ValueError, match="robust must be"):
            cls(robust="trim")                                                          # (a trim is trim=, not a kernel's name)


def test_names_in_header_library_and_binding():
    from point_cloud_registration_amd import _capi
    text = open(os.path.join(REPO, "include", "pcr.h")).read()
    declared = set(re.findall(r"PCR_API\s+[\w\s\*]+?\b(pcr_\w+)\s*\(", text))
    assert len(NAMES) == 9 and set(NAMES) <= declared
    assert re.search(r"#define\s+PCR_ROBUST_TRIM\s+5\b", text) and "pcr_adaptive;" in text
    if not os.path.exists(_capi.LIB_PATH):
        from point_cloud_registration_amd.build import build
        build()
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pcr_\w+)", out))
    assert set(NAMES) <= exported
    assert set(NAMES) <= set(_capi.PROTOTYPES)
    L = _capi.lib()
    for name in NAMES:
        assert getattr(L, name) is not None
    for unit in _capi.MATCH_UNITS:
        assert callable(getattr(_capi, f"{unit}_linearize_adaptive")) and callable(getattr(_capi, f"{unit}_align_adaptive"))
    assert callable(_capi.order_statistic) and callable(_capi.check_adaptive)
    # the struct of the binding has the header's layout: int, double, double
    assert [f[0] for f in _capi.Adaptive._fields_] == ["kind", "quantile", "factor"] and _capi.Adaptive.quantile.offset == 8
