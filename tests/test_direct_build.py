"""The compiler's own resource report for csrc/vgicp_direct.hip: every instantiation of the lookup, the pass, the robust pass
and the residual kernel is there for 1, 7 and 27 voxels, none of them uses scratch memory -- the hit list of a lane lives in LDS,
the accumulators in registers -- and none loses a resident wave against what docs/EXPERIMENTS.md records.

The register bounds are the occupancy steps of a 512-register SIMD lane (waves per SIMD: 8 up to 64 VGPRs, 5 up to 96, 4 up to
128, 3 up to 168, 2 up to 256) at which each kernel was recorded (2026-10-21): pass and robust pass 124 / 178 / 235 VGPRs, residuals
54 / 81 / 119, lookup 36 / 44 / 122.  LDS is exact by construction: 4 bytes per lane and offset, 256 lanes, and the 1 KiB of
block_store_partials in the kernels that fold."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources

# kernel -> NB -> (largest VGPR count that keeps the recorded waves per SIMD, LDS bytes per block)
EXPECT = {
    "k_voxel_lookup": {1: (64, 0), 7: (64, 0), 27: (128, 0)},
    "k_vgicp_direct": {1: (128, 2048), 7: (256, 8192), 27: (256, 28672)},
    "k_vgicp_direct_robust": {1: (128, 2048), 7: (256, 8192), 27: (256, 28672)},
    "k_vgicp_direct_residuals": {1: (64, 1024), 7: (96, 7168), 27: (128, 27648)},
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_direct_kernels_stay_out_of_scratch():
    report = kernel_resources("vgicp_direct.hip")
    assert len(report) >= 14, f"the resource report was not parsed: {sorted(report)}"
    for kernel, by_nb in EXPECT.items():
        for nb, (vgprs, lds) in by_nb.items():
            # (Itanium mangling: <length><name>ILi<NB>EE)
            hits = [n for n in report if f"{len(kernel)}{kernel}ILi{nb}EE" in n]
            assert len(hits) == 1, (kernel, nb, sorted(report))
            u = report[hits[0]]
            print(f"{kernel}<{nb}>: {u['vgprs']} VGPRs (bound {vgprs}), {u['sgprs']} SGPRs, {u['lds']} bytes of LDS, scratch {u['scratch']}")
            assert u["scratch"] == 0, (kernel, nb)
            assert u["vgprs"] <= vgprs, (kernel, nb, u["vgprs"])
            assert u["lds"] == lds, (kernel, nb, u["lds"])
    assert {n: u["scratch"] for n, u in report.items() if u["scratch"] != 0} == {}
