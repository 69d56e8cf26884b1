"""Batched alignment (align_batch / calc_H_g_e2_batch, pcr_linearize_batch / pcr_align_batch): everything that needs no GPU --
signatures, the errors raised before any library call, the normalisation of the input forms, the binding's prototypes, and
the compiler's resource report for the batched kernels."""

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
BATCH_SYMBOLS = ("pcr_scan_batch_create", "pcr_scan_batch_size", "pcr_scan_batch_destroy", "pcr_linearize_batch", "pcr_align_batch")


def _classes():
    import point_cloud_registration_amd as pcr
    return (pcr.ICP, pcr.PlaneICP, pcr.VPlaneICP, pcr.NDT)


def test_signatures_and_defaults():
    for cls in _classes():
        sig = inspect.signature(cls.align_batch)
        assert list(sig.parameters) == ["self", "sources", "init_Ts", "return_info"]
        assert sig.parameters["init_Ts"].default is None and sig.parameters["return_info"].default is False
        assert list(inspect.signature(cls.calc_H_g_e2_batch).parameters) == ["self", "cur_Ts", "sources"]


def test_new_entry_points_are_declared_and_bound():
    from point_cloud_registration_amd import _capi
    header = open(os.path.join(REPO, "include", "pcr.h")).read()
    for name in BATCH_SYMBOLS:
        assert re.search(rf"PCR_API\s+pcr_status\s+{name}\s*\(", header), name
        assert name in _capi.PROTOTYPES
    # adding entry points is not a layout change
    assert int(re.search(r"#define PCR_ABI_VERSION (\d+)", header).group(1)) == _capi.ABI_VERSION
    assert len(_capi.PROTOTYPES["pcr_align_batch"][1]) == 14 and len(_capi.PROTOTYPES["pcr_linearize_batch"][1]) == 9


def test_errors_come_before_any_library_call(monkeypatch):
    from point_cloud_registration_amd import _capi

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_capi, "lib", no_library)
    monkeypatch.setattr(_capi, "get_context", lambda *a, **k: no_library())
    src = np.zeros((10, 3), np.float32)
    for cls in _classes():
        m = cls()
        with pytest.raises(ValueError, match="Target is not set."):
            m.align_batch([src])
        with pytest.raises(ValueError, match="Target is not set."):
            m.calc_H_g_e2_batch(np.eye(4), [src])
        m._is_target_set = True                      # (as after set_target; no target handle is reached below)
        for bad in ([np.zeros((10, 2))], [src, np.zeros(3)], [], 5):
            with pytest.raises(ValueError):
                m.align_batch(bad)
        with pytest.raises(ValueError):
            m.align_batch([src, src], np.zeros((3, 4, 4)))            # 3 poses for 2 sources
        with pytest.raises(ValueError):
            m.align_batch([src], np.eye(3))
        with pytest.raises(ValueError):
            m.calc_H_g_e2_batch(np.zeros((2, 4, 4)), [src])
        m._comm = object()
        with pytest.raises(ValueError, match="comm="):
            m.align_batch([src])
        m._comm, m._group = None, object()
        with pytest.raises(ValueError, match="devices="):
            m.calc_H_g_e2_batch(np.eye(4), [src])


def test_normalize_batch_inputs():
    from point_cloud_registration_amd.registration import normalize_batch_inputs
    rng = np.random.default_rng(0)
    a = rng.normal(size=(7, 3))                      # float64 in: cast to float32
    b = rng.normal(size=(4, 3)).astype(np.float32)
    e = np.zeros((0, 3), np.float32)

    # a sequence: one item per entry, identity poses
    arrays, offsets, item_scan, Ts = normalize_batch_inputs([a, b, e])
    assert [x.shape for x in arrays] == [(7, 3), (4, 3), (0, 3)] and all(x.dtype == np.float32 for x in arrays)
    assert np.array_equal(arrays[0], a.astype(np.float32)) and arrays[1] is b
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 7, 11, 11]
    assert item_scan.dtype == np.intc and item_scan.tolist() == [0, 1, 2]
    assert Ts.shape == (3, 4, 4) and Ts.dtype == np.float64 and all(np.array_equal(T, np.eye(4)) for T in Ts)

    # the same array OBJECT several times: listed once; an equal COPY is another scan
    arrays, offsets, item_scan, Ts = normalize_batch_inputs([a, b, a, b.copy(), a])
    assert len(arrays) == 3 and offsets.tolist() == [0, 7, 11, 15] and item_scan.tolist() == [0, 1, 0, 2, 0]

    # one array + B poses: multi-start
    P = np.stack([np.eye(4) * (i + 1) for i in range(5)])
    arrays, offsets, item_scan, Ts = normalize_batch_inputs(b, P)
    assert len(arrays) == 1 and arrays[0] is b and offsets.tolist() == [0, 4] and item_scan.tolist() == [0] * 5
    assert np.array_equal(Ts, P) and Ts.flags.c_contiguous
    # one array, one pose / no pose: a batch of one
    for poses in (None, np.eye(4) * 2):
        arrays, offsets, item_scan, Ts = normalize_batch_inputs(b, poses)
        assert len(arrays) == 1 and item_scan.tolist() == [0] and Ts.shape == (1, 4, 4)
    # a (4, 4) pose is broadcast over a sequence; the result does not alias the caller's array
    T1 = np.eye(4) * 3
    arrays, offsets, item_scan, Ts = normalize_batch_inputs([a, b], T1)
    assert Ts.shape == (2, 4, 4) and np.array_equal(Ts[0], T1) and np.array_equal(Ts[1], T1)
    Ts[0, 0, 0] = -1
    assert T1[0, 0] == 3
    # a (B, N, 3) array is a sequence of B scans
    arrays, offsets, item_scan, Ts = normalize_batch_inputs(np.zeros((3, 6, 3), np.float32))
    assert len(arrays) == 3 and offsets.tolist() == [0, 6, 12, 18] and item_scan.tolist() == [0, 1, 2]

    for bad_sources, bad_poses in (([a, np.zeros((3, 2))], None), ([], None), ([a], np.zeros((2, 4, 4))), (b, np.zeros((4, 3))),
                                   (7, None), ([a, b], np.zeros((2, 2, 4, 4)))):
        with pytest.raises(ValueError):
            normalize_batch_inputs(bad_sources, bad_poses)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_batched_kernels_use_no_more_scratch_than_the_single_ones(tmp_path):
    """The batched kernels are instantiations of their own over the shared device functions (no run-time branch in the
    single-scan kernels); like the fused small-scan kernels they stay below 128 bytes of scratch per lane -- the compiler's own
    resource report, as tests/test_build_hygiene.py reads it for the others."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        f"-I{REPO}/include", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "kernels.hip"), "-o", str(tmp_path / "k.o")], capture_output=True, text=True, check=True)
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    batch = {n: b for n, b in usage.items() if "k_linearize_batch" in n}
    # four kinds; point kinds: lists x boxes, voxel kinds: no filter / filter / filter with lists; each plain and with the step
    assert len(batch) == 28, sorted(batch)
    for kind in range(4):
        for gn in (0, 1):
            assert any(re.match(rf"_Z17k_linearize_batchILi{kind}ELi\dELi{gn}E", n) for n in batch), (kind, gn)
    assert {n: b for n, b in batch.items() if b > 128} == {}
    assert usage.get("_Z12k_batch_initPK9BatchItemi") == 0
