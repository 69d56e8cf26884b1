"""linearize / weighted calc_H_g_e2 / coreset: the interface and its argument checks.  Needs no GPU: everything here is
refused before the library is touched."""

import inspect
import os
import re

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

from conftest import REPO

CLASSES = (pcr.ICP, pcr.PlaneICP, pcr.VPlaneICP, pcr.NDT)
SRC = np.zeros((5, 3), np.float32)


def with_target_flag(cls):
    """An instance that believes its target is set (no device involved: the argument checks come first)."""
    reg = cls()
    reg._is_target_set = True
    return reg


@pytest.mark.parametrize("cls", CLASSES)
def test_methods_exist(cls):
    assert list(inspect.signature(cls.linearize).parameters) == ["self", "cur_T", "source", "return_index"]
    assert list(inspect.signature(cls.calc_H_g_e2).parameters) == ["self", "cur_T", "source", "weights"]
    assert inspect.signature(cls.calc_H_g_e2).parameters["weights"].default is None
    p = inspect.signature(cls.coreset).parameters
    assert list(p) == ["self", "cur_T", "source", "N_target", "k"] and p["N_target"].default == 1024 and p["k"].default == 64


@pytest.mark.parametrize("cls", CLASSES)
def test_unset_target_is_a_value_error(cls):
    reg = cls()
    with pytest.raises(ValueError, match="Target is not set."):
        reg.linearize(np.eye(4), SRC)
    with pytest.raises(ValueError, match="Target is not set."):
        reg.calc_H_g_e2(np.eye(4), SRC, weights=np.ones(5))
    with pytest.raises(ValueError, match="Target is not set."):
        reg.calc_H_g_e2(np.eye(4), SRC)
    with pytest.raises(ValueError, match="Target is not set."):
        reg.coreset(np.eye(4), SRC)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("bad", [np.ones(4), np.ones((5, 1)), [1, 1, np.nan, 1, 1], [1, np.inf, 1, 1, 1], [1, 1, 1, -1e-300, 1]],
                         ids=["short", "2d", "nan", "inf", "negative"])
def test_bad_weights(cls, bad):
    with pytest.raises(ValueError, match="weights"):
        with_target_flag(cls).calc_H_g_e2(np.eye(4), SRC, weights=bad)


@pytest.mark.parametrize("cls", CLASSES)
def test_bad_coreset_sizes(cls):
    reg = with_target_flag(cls)
    with pytest.raises(ValueError, match="N_target"):
        reg.coreset(np.eye(4), SRC, N_target=28)
    with pytest.raises(ValueError, match="k must"):
        reg.coreset(np.eye(4), SRC, k=29)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("how", ["comm", "devices"])
def test_one_gpu_of_one_process_only(cls, how):
    reg = with_target_flag(cls)
    if how == "comm":
        reg._comm = object()
    else:
        reg._group = object()          # (what devices= leaves behind; building a real group needs the GPUs)
    with pytest.raises(ValueError, match="comm= or devices="):
        reg.linearize(np.eye(4), SRC)
    with pytest.raises(ValueError, match="comm= or devices="):
        reg.calc_H_g_e2(np.eye(4), SRC, weights=np.ones(5))
    with pytest.raises(ValueError, match="comm= or devices="):
        reg.coreset(np.eye(4), SRC)


def test_uploaded_scan_without_the_order_is_refused():
    class FakeScan:
        flags = 0
    reg = with_target_flag(pcr.ICP)
    with pytest.raises(ValueError, match="keep_order"):
        reg.linearize(np.eye(4), pcr.registration.UploadedScan(FakeScan(), (5, 3)))


def test_keep_order_flag():
    assert _capi.FLAG_KEEP_ORDER == 32
    header = open(os.path.join(REPO, "include", "pcr.h")).read()
    assert re.search(r"PCR_FLAG_KEEP_ORDER = 32u", header)
    for name in ("pcr_linearize_rows", "pcr_linearize_weighted", "pcr_scan_coreset"):
        assert name in _capi.PROTOTYPES and re.search(rf"PCR_API pcr_status {name}\(", header)
