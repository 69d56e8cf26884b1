"""k_fgr_solo, the single-block form of the FGR loop, lost its A/B against the loop of launches (docs/EXPERIMENTS.md) and is in
the developer build only: the shipped library does not carry it, and in a process that loaded libpcr_hip_dev.so (PCR_LIB) it
still returns the bits of the loop of launches (tests/fgr_solo_check.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fgr_cases as fc
from conftest import REPO
from test_gpu_fgr import env, same_bits

pytestmark = pytest.mark.gpu


def test_shipped_library_has_no_single_block_loop():
    from point_cloud_registration_amd import _capi
    if os.environ.get("PCR_LIB"):
        pytest.skip("PCR_LIB selects another build")
    ctx = _capi.get_context(0)
    assert _capi.fgr_solo_max(ctx) == 0
    assert b"k_fgr_solo" not in open(_capi.LIB_PATH, "rb").read()                 # not even as device code in the fat binary
    c = fc.case("A", 0)
    a = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], fc.MAX_DIST ** 2, **fc.SCHEDULE)
    with env(PCR_FGR_SOLO=1):                                                      # asking for it changes nothing
        b = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], fc.MAX_DIST ** 2, **fc.SCHEDULE)
    assert same_bits(a["T"], b["T"]) and same_bits(a["weights"], b["weights"])


def test_single_block_loop_in_the_developer_build():
    from point_cloud_registration_amd import _capi
    assert os.path.exists(_capi.DEV_LIB_PATH), "make dev (csrc/Makefile) builds libpcr_hip_dev.so"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "fgr_solo_check.py")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PCR_LIB=_capi.DEV_LIB_PATH), cwd=REPO)
    assert r.returncode == 0 and "solo ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    print(r.stdout.strip().splitlines()[-1])
