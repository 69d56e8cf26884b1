"""The host-side rule that decides which targets store the records of a cell in ascending x (index_build.hip:
pcr_x_order_rule), and index_info()'s field -- no GPU needed."""
import inspect
import os
import subprocess
import sys

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from point_cloud_registration_amd.build import build
        build()
    return _capi


def test_rule(capi, monkeypatch):
    monkeypatch.delenv("PCR_XORDER", raising=False)
    rule = capi.lib().pcr_x_order_rule
    assert rule(1, 0, 1_060_000, 22) == 1                 # the street cloud: float32 points, no heavy cells
    assert rule(1, 0, 1, 1) == 1
    assert rule(1, 1, 1_060_000, 24) == 0                 # heavy cells keep the Morton order of their leaf / group boxes
    assert rule(0, 0, 1_060_000, 22) == 0                 # centroid grids and the float32 filter index of a voxel target
    assert rule(1, 0, 0, 1) == 0                          # an empty target has nothing to order
    assert rule(1, 0, 100_000_000, 32) == 1               # 32 bits of cell id + 16 bits of x offset fit the 64-bit key
    assert rule(1, 0, 1000, 49) == 0                      # a key that would not


def test_switch_is_read_from_the_environment_of_the_build(capi):
    """PCR_XORDER=0 builds the old order (the A/B switch); anything else, or nothing, the x order"""
    code = ("import sys; sys.path.insert(0, %r); from point_cloud_registration_amd import _capi; "
            "print(_capi.lib().pcr_x_order_rule(1, 0, 1000, 10))" % REPO)
    for value, want in (("0", "0"), ("1", "1"), ("", "1"), (None, "1")):
        env = {k: v for k, v in os.environ.items() if k != "PCR_XORDER"}
        if value is not None:
            env["PCR_XORDER"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.strip() == want, (value, out)


def test_index_info_reports_the_order(capi):
    assert "pcr_target_index_x_order" in capi.PROTOTYPES and "pcr_x_order_rule" in capi.PROTOTYPES
    src = inspect.getsource(capi.Target.index_info)
    assert '"x_ordered"' in src and "pcr_target_index_x_order" in src
