#!/usr/bin/env python3
"""Developer probe: what the adaptive pass of GICP, VGICP, SymmetricICP and ColoredICP costs beside the robust pass.
    adaptive_time.py [--scan N] [--target N]

Cloud: street(n) (default 1.06 M points) against a perturbed copy of itself, as tools/robust_time.py.  Per aligner, in one
process and one loop: calc_H_g_e2 with a fixed Tukey scale (pcr_*_linearize_robust), with trim=0.6 and with Tukey at
("quantile", 0.5, 3) (pcr_*_linearize_adaptive).  Every figure is a median over 5 calls after 2 warm-ups by HIP events on the
context's stream around the call (tools/timing.py).  With PCR_ADAPTIVE_TIMES=1 the library brackets the two phases an adaptive
pass has beyond the robust one -- the key kernel, and the selection (16 launches; a trim's drop kernel with them) -- with events
of its own and reports them on stderr; this tool collects those lines: select_ms is the selection kernels alone."""
import argparse
import os
import sys

import numpy as np

os.environ["PCR_ADAPTIVE_TIMES"] = "1"            # (read once, by the first adaptive pass)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from timing import timed  # noqa: E402
import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd.synthetic import perturbed_scan, street, street_normals  # noqa: E402
from robust_time import field  # noqa: E402

PHASES = ("keys_ms", "select_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=1_060_000)
    ap.add_argument("--scan", type=int, default=1_060_000)
    a = ap.parse_args()
    target = street(a.target, seed=0)
    normals = street_normals(target)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]
    scan = perturbed_scan(target, a.scan if a.scan < a.target else None, seed=2)[0]
    I_q, I_p = field(target), field(scan)
    for name, cls in (("gicp", pcr.GICP), ("vgicp", pcr.VGICP), ("symm", pcr.SymmetricICP), ("color", pcr.ColoredICP)):
        kw = {"voxel_size": 1.0} if cls is pcr.VGICP else {}
        extra = {"source_intensity": I_p} if cls is pcr.ColoredICP else {}
        plain = cls(max_dist=2.0, k=10, **kw)
        if cls is pcr.SymmetricICP:
            plain.set_target(target, norm=normals)
        elif cls is pcr.ColoredICP:
            plain.set_target(target, I_q, norm=normals)
        else:
            plain.set_target(target)
        h = plain.upload(scan, keep_order=True)
        plain.calc_H_g_e2(T, h, **extra)                     # (estimates / uploads the scan's payload: once per uploaded scan)
        s = plain.residuals(T, h, **extra)
        s = s.sum(axis=1) if s.ndim == 2 else s
        c = 3.0 * float(np.sqrt(np.median(s[np.isfinite(s)])))
        regs = {"robust": cls(max_dist=2.0, k=10, robust="tukey", robust_scale=c, **kw), "trim": cls(max_dist=2.0, k=10, trim=0.6, **kw),
                "tukey_q": cls(max_dist=2.0, k=10, robust="tukey", robust_scale=("quantile", 0.5, 3.0), **kw)}
        out = []
        for key, reg in regs.items():                        # (the setting is the aligner's; the device target is shared)
            reg._target, reg._is_target_set = plain._target, True
            med = timed(lambda: reg.calc_H_g_e2(T, h, **extra), PHASES if key != "robust" else ())
            out.append(f"{key}: {med['call_ms']:.3f} ms" + "".join(f" {p[:-3]} {med[p] * 1e3:.1f} us" for p in PHASES if p in med))
            if reg.last_adaptive:
                out[-1] += f" (kept {reg.last_adaptive['kept']:.0f} of {reg.last_correspondences}, scale {reg.last_adaptive['scale']:.4g})"
        print(f"{name} scan={len(scan)} target={a.target} fixed c={c:.4g}: " + " | ".join(out), flush=True)
        h.close()
        plain._target.close()


if __name__ == "__main__":
    main()
