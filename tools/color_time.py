#!/usr/bin/env python3
"""Developer probe: the intensity-gradient estimate of ColoredICP at k = 10 and 20, and the per-pass time of
ColoredICP.calc_H_g_e2 against SymmetricICP and PlaneICP under the `split` pipeline, where all three run a search kernel and then
their reduce (PlaneICP: k_reduce_finalize; SymmetricICP: k_symm_reduce + k_symm_fold; ColoredICP: k_color_reduce + k_color_fold).
    color_time.py [--scan N ...] [--target N] [--reps R]

Every figure is a median over reps after warm-up calls of the same shape: HIP events on the context's stream around the call
(device time of what the call enqueued) and a host clock around the call, which ends in a stream synchronisation everywhere.  The
gradient estimate enqueues ONE kernel, k_color_gradient, so its event time is the kernel's.  The classes alternate inside one
loop.  The reduce kernels alone: run this under `rocprofv3 --kernel-trace --stats -- python tools/color_time.py` and read
k_color_reduce / k_symm_reduce / k_reduce_finalize."""
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
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    return (0.5 + 0.2 * np.sin(2.1 * P[:, 0] + 0.3) + 0.2 * np.cos(1.7 * P[:, 1]) + 0.1 * np.sin(1.3 * P[:, 2])).astype(np.float32)


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
    inten = field(target)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]

    plane, symm, color = pcr.PlaneICP(max_dist=2.0), pcr.SymmetricICP(max_dist=2.0, k=10), pcr.ColoredICP(max_dist=2.0, k=10)
    plane.set_target(target, kdree=object(), norm=normals)
    symm.set_target(target, norm=normals)
    color.set_target(target, inten, norm=normals)
    for k in (10, 20):
        ev = []
        for r in range(a.warmup + a.reps):
            e, _ = timed(stream, lambda: color._target.estimate_color_gradients(k, want=False))
            if r >= a.warmup:
                ev.append(e)
        print(f"k_color_gradient n={a.target} k={k}: events {np.median(ev):.3f} ms (min {np.min(ev):.3f})", flush=True)
    color._target.estimate_color_gradients(10, want=False)
    with ctx.pipeline(variant=1):
        for n in a.scan:
            scan = perturbed_scan(target, n if n < a.target else None, seed=2)[0]
            s_int = field(scan)
            hp, hs, hc = plane.upload(scan), symm.upload(scan), color.upload(scan, keep_order=True)
            symm.calc_H_g_e2(T, hs)                       # (estimates the scan's normals: once per uploaded scan)
            color.calc_H_g_e2(T, hc, s_int)               # (uploads the scan's intensities: once per uploaded scan)
            res = {"plane": ([], []), "symm": ([], []), "color": ([], [])}
            calls = (("plane", lambda: plane.calc_H_g_e2(T, hp)), ("symm", lambda: symm.calc_H_g_e2(T, hs)),
                     ("color", lambda: color._linearize(T, hc._scan)))      # (without hashing the intensity array per call)
            for r in range(a.warmup + a.reps):
                for name, call in calls:
                    e, hms = timed(stream, call)
                    if r >= a.warmup:
                        res[name][0].append(e); res[name][1].append(hms)
            line = " | ".join(f"{name}: events {np.median(v[0]):.3f} ms (min {np.min(v[0]):.3f}), host {np.median(v[1]):.3f} ms"
                              for name, v in res.items())
            print(f"pass scan={len(scan)} target={a.target}: {line} | kept plane {plane.last_correspondences} "
                  f"symm {symm.last_correspondences} color {color.last_correspondences}", flush=True)
            hp.close(); hs.close(); hc.close()


if __name__ == "__main__":
    main()
