#!/usr/bin/env python3
"""Developer probe: per-pass time of GICP.calc_H_g_e2 against ICP.calc_H_g_e2 under the `split` pipeline (the same search
kernel: k_nn_scan; ICP then runs k_reduce_finalize, GICP k_gicp_reduce + k_gicp_fold), and set_target with covariance
estimation.   gicp_time.py [--scan N ...] [--target N] [--reps R]

Every figure is a median over reps after warm-up passes of the same shape, taken twice: HIP events on the context's stream
around the call (device time of what the call enqueued) and a host clock around the call, which ends in a stream
synchronisation in both classes.  ICP and GICP alternate inside one loop."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import point_cloud_registration_amd as pcr  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402
from point_cloud_registration_amd.synthetic import perturbed_scan, street  # noqa: E402


def timed(stream, fn):
    """(event ms, host ms) of one call that ends synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=1_060_000)
    ap.add_argument("--scan", type=int, nargs="*", default=[100_000, 1_060_000])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ctx = _capi.get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    target = street(a.target, seed=0)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]

    for k in (10, 20):
        ev, host = [], []
        for r in range(a.warmup + 8):
            g = pcr.GICP(max_dist=2.0, k=k)
            e, h = timed(stream, lambda: g.set_target(target))
            if r >= a.warmup:
                ev.append(e); host.append(h)
        print(f"set_target n={a.target} k={k} (index + covariance estimation): events {np.median(ev):.3f} ms, host {np.median(host):.3f} ms", flush=True)
    ev, host = [], []
    for r in range(a.warmup + 8):
        i = pcr.ICP(max_dist=2.0)
        e, h = timed(stream, lambda: i.set_target(target))
        if r >= a.warmup:
            ev.append(e); host.append(h)
    print(f"set_target n={a.target} ICP (index only): events {np.median(ev):.3f} ms, host {np.median(host):.3f} ms", flush=True)

    icp, gicp = pcr.ICP(max_dist=2.0), pcr.GICP(max_dist=2.0, k=10)
    icp.set_target(target)
    gicp.set_target(target)
    with ctx.pipeline(variant=1):
        for n in a.scan:
            scan = perturbed_scan(target, n if n < a.target else None, seed=2)[0]
            hi, hg = icp.upload(scan), gicp.upload(scan)
            t0 = time.perf_counter()
            gicp.calc_H_g_e2(T, hg)                       # (estimates the scan's covariances: once per uploaded scan)
            first = (time.perf_counter() - t0) * 1e3
            res = {"icp": ([], []), "gicp": ([], [])}
            for r in range(a.warmup + a.reps):
                for name, reg, h in (("icp", icp, hi), ("gicp", gicp, hg)):
                    e, hms = timed(stream, lambda: reg.calc_H_g_e2(T, h))
                    if r >= a.warmup:
                        res[name][0].append(e); res[name][1].append(hms)
            line = " | ".join(f"{name}: events {np.median(v[0]):.3f} ms (min {np.min(v[0]):.3f}), host {np.median(v[1]):.3f} ms"
                              for name, v in res.items())
            print(f"pass scan={len(scan)} target={a.target}: {line} | first GICP pass incl. scan covariances {first:.2f} ms "
                  f"| kept icp {icp.last_correspondences} gicp {gicp.last_correspondences}", flush=True)
            hi.close(); hg.close()


if __name__ == "__main__":
    main()
