#!/usr/bin/env python3
"""Developer probe: per-pass time of VGICP.calc_H_g_e2 against NDT.calc_H_g_e2 under the `split` pipeline (NDT: k_nn_filter /
k_nn_scan + k_reduce_finalize; VGICP: the float64 centroid search of the rows passes + k_vgicp_reduce + k_vgicp_fold), and
set_target with and without the covariance step.   vgicp_time.py [--scan N ...] [--target N] [--reps R]

The protocol of tools/gicp_time.py: every figure is a median over reps after warm-up passes of the same shape, taken twice:
HIP events on the context's stream around the call (device time of what the call enqueued) and a host clock around the call,
which ends in a stream synchronisation in both classes.  NDT and VGICP alternate inside one loop."""
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
    ap.add_argument("--voxel-size", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ctx = _capi.get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream())
    target = street(a.target, seed=0)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]

    for name, make in (("VGICP plane (voxel build + covariance step)", lambda: pcr.VGICP(voxel_size=a.voxel_size, max_dist=2.0)),
                       ("VGICP raw (voxel build + covariance step)", lambda: pcr.VGICP(voxel_size=a.voxel_size, max_dist=2.0, regularization="raw")),
                       ("NDT (voxel build only)", lambda: pcr.NDT(voxel_size=a.voxel_size, max_dist=2.0))):
        ev, host = [], []
        for r in range(a.warmup + 8):
            reg = make()
            e, h = timed(stream, lambda: reg.set_target(target))
            if r >= a.warmup:
                ev.append(e); host.append(h)
        print(f"set_target n={a.target} {name}: events {np.median(ev):.3f} ms, host {np.median(host):.3f} ms, "
              f"{len(reg.voxels.mean)} kept voxels", flush=True)
    # the covariance step alone, on a target that is already built
    reg = pcr.VGICP(voxel_size=a.voxel_size, max_dist=2.0)
    reg.set_target(target)
    for mode, label in ((_capi.COV_PLANE, "plane"), (_capi.COV_RAW, "raw")):
        ev = [timed(stream, lambda: reg._target.set_voxel_covariances(mode, 1e-3))[0] for _ in range(a.warmup + 8)][a.warmup:]
        print(f"set_voxel_covariances {label} alone: events {np.median(ev):.3f} ms", flush=True)

    ndt, vgicp = pcr.NDT(voxel_size=a.voxel_size, max_dist=2.0), pcr.VGICP(voxel_size=a.voxel_size, max_dist=2.0, k=10)
    ndt.set_target(target)
    vgicp.set_target(target)
    with ctx.pipeline(variant=1):
        for n in a.scan:
            scan = perturbed_scan(target, n if n < a.target else None, seed=2)[0]
            hn, hv = ndt.upload(scan), vgicp.upload(scan)
            t0 = time.perf_counter()
            vgicp.calc_H_g_e2(T, hv)                      # (estimates the scan's covariances: once per uploaded scan)
            first = (time.perf_counter() - t0) * 1e3
            res = {"ndt": ([], []), "vgicp": ([], [])}
            for r in range(a.warmup + a.reps):
                for name, reg, h in (("ndt", ndt, hn), ("vgicp", vgicp, hv)):
                    e, hms = timed(stream, lambda: reg.calc_H_g_e2(T, h))
                    if r >= a.warmup:
                        res[name][0].append(e); res[name][1].append(hms)
            line = " | ".join(f"{name}: events {np.median(v[0]):.3f} ms (min {np.min(v[0]):.3f}), host {np.median(v[1]):.3f} ms"
                              for name, v in res.items())
            print(f"pass scan={len(scan)} target={a.target}: {line} | first VGICP pass incl. scan covariances {first:.2f} ms "
                  f"| kept ndt {ndt.last_correspondences} vgicp {vgicp.last_correspondences}", flush=True)
            hn.close(); hv.close()


if __name__ == "__main__":
    main()
