"""Run by tests/test_gpu_fgr_dev.py in a process that loaded the developer build (PCR_LIB): the single-block form of the FGR
loop (k_fgr_solo, PCR_FGR_SOLO=1) against the loop of launches -- the same bits in pose, trace, weights, counters -- and the
library's own report that it was the single block that ran.  Prints one line "solo ok ..." and exits 0."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgr_cases as fc  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402

ctx = _capi.get_context(0)
assert _capi.has_dev_kernels()
solo_max = _capi.fgr_solo_max(ctx)
assert solo_max >= 2000, solo_max                 # 64 KiB of LDS would already hold 2 194 matches


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def both(src, dst, T0, mu0, mu_min, tol=0.0, mult=None, **schedule):
    out = []
    for flag in ("0", "1"):
        os.environ["PCR_FGR_SOLO"] = flag
        os.environ["PCR_FGR_TIMES"] = "1"
        sys.stderr.flush()
        saved = os.dup(2)
        with tempfile.TemporaryFile(mode="w+") as f:          # the library's report goes to stderr
            os.dup2(f.fileno(), 2)
            try:
                r = _capi.fgr_pose(ctx, src, dst, T0, mu0, mu_min, tol=tol, mult=mult, want_trace=True, **schedule)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            f.seek(0)
            r["report"] = f.read()
        out.append(r)
    loop, solo = out
    assert "form device" in loop["report"] and "form solo" in solo["report"], (loop["report"], solo["report"])
    for k in ("T", "trace", "weights"):
        assert np.array_equal(bits(loop[k]), bits(solo[k])), k
    assert (loop["iterations"], loop["status"], loop["mu"]) == (solo["iterations"], solo["status"], solo["mu"])
    return solo


n = 0
for name, seed in (("A", 0), ("B", 0)):           # 2 and 12 tiles, the last one ragged
    c = fc.case(name, seed)
    r = both(c["src"], c["dst"], np.eye(4), c["mu0"], fc.MAX_DIST ** 2, **fc.SCHEDULE)
    assert r["iterations"] == 64 and r["status"] == 0
    n += 1
c = fc.case("A", 1)                                # multiplicities, and the end at the floor
mult = np.random.default_rng(3).integers(0, 4, len(c["src"])).astype(np.int32)
r = both(c["src"], c["dst"], c["T_true"], 4.0, 1.0, tol=1e-9, mult=mult * c["inlier"], division=2.0, period=1, max_iter=40)
assert r["status"] == 1 and 2 < r["iterations"] < 40
pts = np.float32([[1, 2, 3], [4, -1, 2]])          # exactly singular
for m in (1, 2):
    r = both(pts[:m], pts[:m], np.eye(4), 100.0, 0.01, division=1.4, period=4, max_iter=8)
    assert (r["status"], r["iterations"]) == (2, 1) and np.array_equal(r["T"], np.eye(4))
rng = np.random.default_rng(9)                     # a list one match too long runs the launches whatever is asked
big = rng.uniform(-20, 20, (solo_max + 1, 3)).astype(np.float32)
os.environ["PCR_FGR_SOLO"] = "1"
a = _capi.fgr_pose(ctx, big, big[::-1].copy(), np.eye(4), 4800.0, 1.0, 1.4, 4, 4)
os.environ["PCR_FGR_SOLO"] = "0"
b = _capi.fgr_pose(ctx, big, big[::-1].copy(), np.eye(4), 4800.0, 1.0, 1.4, 4, 4)
assert np.array_equal(bits(a["T"]), bits(b["T"])) and a["iterations"] == 4
fit = big[:solo_max]                               # ... and the largest that fits runs the single block
both(fit, fit[::-1].copy(), np.eye(4), 4800.0, 1.0, division=1.4, period=4, max_iter=4)
print(f"solo ok: {n + 4} comparisons bit-equal, solo_max {solo_max}")
