#!/usr/bin/env python3
"""Developer probe: per-pass time of SymmetricICP.calc_H_g_e2 against GICP and PlaneICP under the `split` pipeline, where all
three run a search kernel and then their reduce (PlaneICP: k_reduce_finalize; GICP: k_gicp_reduce + k_gicp_fold; SymmetricICP:
k_symm_reduce + k_symm_fold), and the one-off normal estimation on a scan.   symm_time.py [--scan N ...] [--target N] [--reps R]

Every figure is a median over reps after warm-up passes of the same shape: HIP events on the context's stream around the call
(device time of what the call enqueued) and a host clock around the call, which ends in a stream synchronisation in all three
classes.  The classes alternate inside one loop.  The reduce kernels alone: run this under
`rocprofv3 --kernel-trace --stats -- python tools/symm_time.py` and read k_symm_reduce / k_gicp_reduce / k_reduce_finalize."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import perturbed_scan, street, street_normals  # noqa: E402

from gicp_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=1_060_000)
    ap.add_argument("--scan", type=int, nargs="*", default=[1_060_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = _capi.get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    target = street(a.target, seed=0)
    normals = street_normals(target)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]

    plane, gicp, symm = pcr.PlaneICP(max_dist=2.0), pcr.GICP(max_dist=2.0, k=10), pcr.SymmetricICP(max_dist=2.0, k=10)
    plane.set_target(target, kdree=object(), norm=normals)
    gicp.set_target(target)
    symm.set_target(target, norm=normals)
    with ctx.pipeline(variant=1):
        for n in a.scan:
            scan = perturbed_scan(target, n if n < a.target else None, seed=2)[0]
            hp, hg, hs = plane.upload(scan), gicp.upload(scan), symm.upload(scan)
            gicp.calc_H_g_e2(T, hg)                       # (estimates the scan's covariances: once per uploaded scan)
            ev = []
            for r in range(a.warmup + a.reps):
                e, _ = timed(stream, lambda: hs._scan.estimate_normals(10, want=False))
                if r >= a.warmup:
                    ev.append(e)
            print(f"scan normals n={len(scan)} k=10 (self-index + k_symm_normals): events {np.median(ev):.3f} ms", flush=True)
            symm.calc_H_g_e2(T, hs)
            res = {"plane": ([], []), "gicp": ([], []), "symm": ([], [])}
            for r in range(a.warmup + a.reps):
                for name, reg, h in (("plane", plane, hp), ("gicp", gicp, hg), ("symm", symm, hs)):
                    e, hms = timed(stream, lambda: reg.calc_H_g_e2(T, h))
                    if r >= a.warmup:
                        res[name][0].append(e); res[name][1].append(hms)
            line = " | ".join(f"{name}: events {np.median(v[0]):.3f} ms (min {np.min(v[0]):.3f}), host {np.median(v[1]):.3f} ms"
                              for name, v in res.items())
            print(f"pass scan={len(scan)} target={a.target}: {line} | kept plane {plane.last_correspondences} "
                  f"gicp {gicp.last_correspondences} symm {symm.last_correspondences}", flush=True)
            hp.close(); hg.close(); hs.close()


if __name__ == "__main__":
    main()
