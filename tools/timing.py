"""What the developer probes tools/{radius,fpfh,iss,ransac,compat,ball,direct}_time.py share: HIP events around a call, the library's
PCR_*_TIMES lines collected from stderr meanwhile, medians over the timed calls, and the radius for a wanted mean count.

A PCR_*_TIMES line is a prefix (pcr_radius_times, ..., pcr_direct_times), then words and "name value" fields; a phase is a field whose name ends
in _ms: PHASE (a regex) finds them, phase_ms(text) -> [(name, milliseconds)].  tests/test_gpu_stage_times.py pins that format
(tests/test_gpu_compat.py for pcr_compat_times, tests/test_gpu_direct.py for pcr_direct_times).

Importing this module touches no GPU: the context's stream and the two events are made by the first call_ms."""
import ctypes
import os
import re
import sys
import tempfile

import numpy as np

WARM, REPS = 2, 5
PREFIXES = ("pcr_radius_times", "pcr_fpfh_times", "pcr_iss_times", "pcr_ransac_times", "pcr_compat_times", "pcr_ball_times",
            "pcr_direct_times")
PHASE = re.compile(r"\b([a-z_]+_ms) ([0-9.]+)")

_hip = []


def phase_ms(text):
    """-> [(phase name, milliseconds)] of every phase field in ``text``, in order"""
    return [(name, float(v)) for name, v in PHASE.findall(text)]


def _events():
    if not _hip:
        from point_cloud_registration_amd import _capi
        hip = ctypes.CDLL("libamdhip64.so.7")     # (already in the process: the library's own runtime)
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
        _hip.extend((hip, ctypes.c_void_p(_capi.get_context(0).stream()), e0, e1))
    return _hip


def call_ms(fn):
    """-> (milliseconds by events around the call, what the library wrote to stderr meanwhile)"""
    hip, stream, e0, e1 = _events()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        try:
            assert hip.hipEventRecord(e0, stream) == 0
            fn()
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read()
    t = ctypes.c_float(0)
    assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
    return t.value, text


def timed(fn, phases=(), report=False):
    """Medians over the timed calls after the warm-ups: {"call_ms": ..., phase: ...}; a phase is summed over the lines of one
    call.  ``report``: -> (medians, the last call's lines)."""
    rows, text = [], ""
    for r in range(WARM + REPS):
        ms, text = call_ms(fn)
        row = {"call_ms": ms}
        for p in phases:
            row[p] = sum(v for name, v in phase_ms(text) if name == p)
        if r >= WARM:
            rows.append(row)
    med = {k: float(np.median([row[k] for row in rows])) for k in rows[0]}
    return (med, text.strip()) if report else med


def quiet(fn):
    """fn() with the library's stderr lines swallowed"""
    box = []
    call_ms(lambda: box.append(fn()))
    return box[0]


def radius_for(target, sample, mean):
    """The float32 radius at which ``target.radius_count(sample, r)`` has about the mean wanted: 30 steps of bisection"""
    lo, hi = 0.0, 5.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if quiet(lambda: target.radius_count(sample, mid)).mean() < mean:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))
