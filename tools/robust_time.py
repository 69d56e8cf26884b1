#!/usr/bin/env python3
"""Developer probe: per-pass time of calc_H_g_e2 of GICP, VGICP, SymmetricICP and ColoredICP without and with a robust kernel
(robust=None runs k_*_reduce, any kind runs k_*_robust; the search in front and the fold behind are the same launches), and of
MatchPass.residuals.   robust_time.py [--scan N] [--target N] [--reps R] [--kinds huber cauchy tukey gm]

Every figure is a median over reps after warm-up passes of the same shape: HIP events on the context's stream around the call
(device time of what the call enqueued).  The aligners and kinds alternate inside one loop.  The scale is the median residual
of the scan (residuals()), so both branches of Huber and Tukey are taken.  The reduce kernels alone: run this under
`rocprofv3 --kernel-trace --stats -- python tools/robust_time.py` and read k_*_reduce against k_*_robust."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import perturbed_scan, street, street_normals  # noqa: E402

from gicp_time import timed  # noqa: E402


def field(P):
    P = np.asarray(P, dtype=np.float64)
    return (0.5 + 0.2 * np.sin(2.1 * P[:, 0] + 0.3) + 0.2 * np.cos(1.7 * P[:, 1]) + 0.1 * np.sin(1.3 * P[:, 2])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=1_060_000)
    ap.add_argument("--scan", type=int, default=1_060_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", nargs="*", default=["huber", "cauchy", "tukey", "gm"])
    a = ap.parse_args()
    ctx = _capi.get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    target = street(a.target, seed=0)
    normals = street_normals(target)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]
    scan = perturbed_scan(target, a.scan if a.scan < a.target else None, seed=2)[0]
    I_q, I_p = field(target), field(scan)

    def make(cls):
        reg = cls(max_dist=2.0, k=10, **({"voxel_size": 1.0} if cls is pcr.VGICP else {}))
        if cls is pcr.SymmetricICP:
            reg.set_target(target, norm=normals)
        elif cls is pcr.ColoredICP:
            reg.set_target(target, I_q, norm=normals)
        else:
            reg.set_target(target)
        return reg

    for name, cls in (("gicp", pcr.GICP), ("vgicp", pcr.VGICP), ("symm", pcr.SymmetricICP), ("color", pcr.ColoredICP)):
        extra = {"source_intensity": I_p} if cls is pcr.ColoredICP else {}
        plain = make(cls)
        h = plain.upload(scan, keep_order=True)
        plain.calc_H_g_e2(T, h, **extra)                     # (estimates / uploads the scan's payload: once per uploaded scan)
        s = plain.residuals(T, h, **extra)
        c = float(np.sqrt(np.median(s[np.isfinite(s)])))
        regs = {"none": plain}
        for kind in a.kinds:                                 # (the kernel is the aligner's; the device target is shared)
            kw = {"voxel_size": 1.0} if cls is pcr.VGICP else {}
            regs[kind] = cls(max_dist=2.0, k=10, robust=kind, robust_scale=c, **kw)
            regs[kind]._target, regs[kind]._is_target_set = plain._target, True
            regs[kind].calc_H_g_e2(T, h, **extra)
        res = {k: [] for k in list(regs) + ["residuals"]}
        for r in range(a.warmup + a.reps):
            for k, reg in regs.items():
                e, _ = timed(stream, lambda: reg.calc_H_g_e2(T, h, **extra))
                if r >= a.warmup:
                    res[k].append(e)
            e, _ = timed(stream, lambda: plain.residuals(T, h, **extra))
            if r >= a.warmup:
                res["residuals"].append(e)
        line = " | ".join(f"{k}: {np.median(v):.3f} ms (min {np.min(v):.3f})" for k, v in res.items())
        print(f"{name} scan={len(scan)} target={a.target} c={c:.4g} kept {plain.last_correspondences}: {line}", flush=True)
        h.close()
        plain._target.close()


if __name__ == "__main__":
    main()
