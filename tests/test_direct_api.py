"""VGICP's direct voxel neighbourhoods without a device: the constructor refuses what the pass does not do, the C ABI carries
the entry points, and the default is the nearest-centroid pass."""

import os
import re

import numpy as np
import pytest

from conftest import REPO

NAMES = ("pcr_target_voxels_lookup", "pcr_target_voxels_set_keys", "pcr_vgicp_direct_linearize", "pcr_vgicp_direct_align",
         "pcr_vgicp_direct_residuals")


def test_default_is_the_nearest_centroid_pass():
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.registration import MatchPass
    v = pcr.VGICP()
    assert v.neighbors is None
    for nb in (1, 7, 27):
        assert pcr.VGICP(neighbors=nb).neighbors == nb
    assert pcr.VGICP(neighbors=7, robust="cauchy", robust_scale=2.0).robust == "cauchy"
    # nothing of the direct pass reaches GICP, whose class keeps the base class's entry points
    assert "_native_linearize" not in vars(pcr.GICP) and pcr.GICP._native_linearize is MatchPass._native_linearize


def test_constructor_refusals():
    import point_cloud_registration_amd as pcr
    for bad in (0, 2, 3, 8, 26, -1, 7.5, "7"):
        with pytest.raises(ValueError, match="neighbors"):
            pcr.VGICP(neighbors=bad)
    with pytest.raises(ValueError, match="neighbors"):
        pcr.VGICP(neighbors=7, trim=0.8)
    with pytest.raises(ValueError, match="neighbors"):
        pcr.VGICP(neighbors=27, robust="huber", robust_scale=("quantile", 0.5, 1.0))
    # ... which the nearest-centroid pass still takes
    assert pcr.VGICP(trim=0.8).trim == 0.8
    assert pcr.VGICP(robust="huber", robust_scale=("quantile", 0.5, 1.0)).neighbors is None
    with pytest.raises(ValueError):
        pcr.VGICP(neighbors=7, devices=[0, 0])
    v = pcr.VGICP(neighbors=7)
    src = np.zeros((4, 3), np.float32)
    for call in (lambda: v.align(src), lambda: v.calc_H_g_e2(np.eye(4), src), lambda: v.residuals(np.eye(4), src)):
        with pytest.raises(ValueError, match="Target is not set."):
            call()
    for call in (lambda: v.linearize(np.eye(4), src), lambda: v.coreset(np.eye(4), src), lambda: v.align_batch([src]),
                 lambda: v.calc_H_g_e2(np.eye(4), src, weights=np.ones(4))):
        with pytest.raises(NotImplementedError, match="VGICP"):
            call()


def test_prototypes_and_header():
    from point_cloud_registration_amd import _capi
    header = open(os.path.join(REPO, "include", "pcr.h")).read()
    for name in NAMES:
        assert name in _capi.PROTOTYPES and re.search(rf"PCR_API pcr_status {name}\(", header), name
    assert len(_capi.PROTOTYPES["pcr_target_voxels_lookup"][1]) == 5
    assert len(_capi.PROTOTYPES["pcr_vgicp_direct_linearize"][1]) == 8
    assert len(_capi.PROTOTYPES["pcr_vgicp_direct_align"][1]) == 12
    assert len(_capi.PROTOTYPES["pcr_vgicp_direct_residuals"][1]) == 7
    assert _capi.NEIGHBORS == (1, 7, 27) and "vgicp_direct" not in _capi.MATCH_UNITS
    for name in ("vgicp_direct_linearize", "vgicp_direct_align", "vgicp_direct_residuals"):
        assert callable(getattr(_capi, name))
    assert callable(_capi.Target.lookup) and callable(_capi.Target.set_voxel_keys)
    # the rule is written down where RANSAC's and FGR's are
    for phrase in ("floor((double)t / voxel_size)", "2^40", "dz outer, dy middle, dx inner", "column 13"):
        assert phrase in header, phrase


def test_voxelgrid_lookup_refuses_other_neighbourhoods():
    from point_cloud_registration_amd.voxel import VoxelGrid
    grid = VoxelGrid(1.0)
    for bad in (0, 3, 26, None):
        with pytest.raises(ValueError, match="neighbors"):
            grid.lookup(np.zeros((2, 3), np.float32), bad)
