#!/usr/bin/env python3
"""Developer probe for the rows kernels (csrc/rows.hip) and the scan coreset.  Needs an MI355X; there is no CPU fall-back.

(a) kernel times: k_rows (MODE 0 rows, MODE 2 flags + MODE 1 terms) against the reduce kernel on the same inputs -- a
    100 k- and a 1.06 M-point scan against the 1.06 M-point stand-in, PlaneICP and NDT.  (The reduce kernel of this tree IS
    the parent's: tools/isa_diff.py finds the device code of kernels.hip unchanged.)  Kernel times come from the per-launch
    records of `rocprofv3 --kernel-trace` in a run of its own, one run per scan size:

        rocprofv3 --kernel-trace --output-format csv -d OUT -o rows100k -- python tools/rows_probe.py --child kernels --points 100000 --meta OUT/rows100k.json
        python tools/rows_probe.py --report OUT/.../rows100k_kernel_trace.csv --meta OUT/rows100k.json

    The child runs 2 warm-up passes and then `--reps` passes of each entry point (search + reduce pipeline forced, so that the
    reduce kernel exists at 100 k points too) and as many launches of a streaming kernel that reads 1 GiB and writes 1 GiB,
    whose time is the copy ceiling of the report; it writes what it did (points of the scan, passes, warm-up) to --meta.  The
    report drops every kernel's warm-up launches and prints, per kernel, the MEDIAN time of the rest with their spread, the
    bytes per point the algorithm needs (counted here, from the shapes) and the achieved fraction of the measured copy rate.

(b) coreset end to end at the 1.06 M-point scan, host clock around calls that end in a device synchronise, the two routes
    alternating, medians of `--reps` after a warm-up:
      host route    J and r on the host (produced once by linearize, not counted) -> create_gn_set -> fast_caratheodory
      device route  Registration.coreset on an uploaded scan: terms kernel + levels on the device-resident P

        python tools/rows_probe.py --coreset [--reps 7]
"""

import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# algorithmic bytes per scan point (read, written), gated-in fraction ~1: index 4 + point 12 + record, rows out
BYTES = {
    ("plane", "reduce"): (4 + 12 + 32, 0),
    ("plane", "rows"): (4 + 12 + 32 + 4, 48 + 8 + 8 + 8),            # + order; J, r, w, idx
    ("plane", "flags"): (4 + 12 + 32 + 4, 4 + 4),
    ("plane", "terms"): (4 + 4 + 4 + 4 + 12 + 32, 28 * 8 + 8),        # flag, inv, off, index, point, record; P, col_idx
    ("ndt", "reduce"): (4 + 12 + 32 + 48, 0),
    ("ndt", "rows"): (4 + 12 + 32 + 48 + 4, 144 + 24 + 8 + 72 + 8),
    ("ndt", "flags"): (4 + 12 + 32 + 4, 4 + 4),
    ("ndt", "terms"): (4 + 4 + 4 + 4 + 12 + 32 + 48, 28 * 8 + 8),
}
KIND_NAMES = {1: "plane", 3: "ndt"}           # the KIND template argument (include/pcr.h: PCR_PLANE, PCR_NDT)
MODE_NAMES = {0: "rows", 1: "terms", 2: "flags"}
COPY_BYTES = 1 << 30
WARMUP = 2


def classify(kernel_name):
    """(kind, what) of a kernel the report covers, "copy" for the streaming kernel, None for everything else."""
    m = re.search(r"\bk_rows<(\d+), *(\d+)>", kernel_name)
    if m and int(m.group(1)) in KIND_NAMES:
        return KIND_NAMES[int(m.group(1))], MODE_NAMES[int(m.group(2))]
    m = re.search(r"\bk_reduce_finalize<(\d+),", kernel_name)
    if m and int(m.group(1)) in KIND_NAMES:
        return KIND_NAMES[int(m.group(1))], "reduce"
    if "elementwise_kernel" in kernel_name and "add" in kernel_name.lower():
        return "copy"
    return None


def setup(points):
    import numpy as np
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd import _capi
    from point_cloud_registration_amd.synthetic import street, perturbed_scan
    assert _capi.device_count() >= 1, "rows_probe needs an MI355X"
    target = street(1_060_000, seed=0)
    scan, _ = perturbed_scan(target, None if points >= len(target) else points, seed=2)
    T = np.eye(4); T[:3, 3] = [0.01, -0.02, 0.015]
    plane = pcr.PlaneICP(max_dist=2.0, k=10)
    plane.set_target(target)
    ndt = pcr.NDT(voxel_size=1.0, max_dist=2.0)
    ndt.set_target(target)
    return np, pcr, _capi, scan, T, {"plane": plane, "ndt": ndt}


def child_kernels(points, reps, meta_path):
    np, pcr, _capi, scan, T, regs = setup(points)
    import torch
    ctx = _capi.get_context(0)
    with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=0):
        for name, reg in regs.items():
            sc = _capi.Scan(ctx, scan, flags=_capi.FLAG_KEEP_ORDER)
            for it in range(reps + WARMUP):
                _capi.linearize(reg._target, sc, reg.KIND, T, 2.0)
                _capi.linearize_rows(reg._target, sc, reg.KIND, T, 2.0, reg._flags)
                _capi.linearize_weighted(reg._target, sc, reg.KIND, T, 2.0, np.ones(sc.n), reg._flags)
            sc.close()
    # the ceiling: a streaming kernel that reads 1 GiB and writes 1 GiB (the only elementwise add of this process)
    a = torch.empty(COPY_BYTES // 4, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    for _ in range(reps + WARMUP):
        torch.add(a, 1.0, out=b)
    torch.cuda.synchronize()
    meta = {"points": int(len(scan)), "reps": reps, "warmup": WARMUP, "copy_bytes": COPY_BYTES}
    if meta_path:
        with open(meta_path, "w") as f:
            json.dump(meta, f)
    print(json.dumps(meta))


def report(path, meta_path):
    with open(meta_path) as f:
        meta = json.load(f)
    points, warmup = meta["points"], meta["warmup"]
    rows = list(csv.DictReader(open(path)))
    key = {k.lower(): k for k in rows[0]}
    name_key, t0_key, t1_key = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows.sort(key=lambda r: int(r[t0_key]))
    launches = {}                     # kernel name -> durations in ns, in launch order
    for r in rows:
        launches.setdefault(r[name_key], []).append(int(r[t1_key]) - int(r[t0_key]))
    timed = {}                        # (kind, what) or "copy" -> (kernel name, durations after the warm-up launches)
    for name, ns in launches.items():
        c = classify(name)
        if c is None:
            continue
        assert len(ns) == meta["reps"] + warmup, (name, len(ns), "launches: expected warm-up + reps")
        assert c not in timed, (c, name, timed[c][0])
        timed[c] = (name, ns[warmup:])
    assert "copy" in timed, "the streaming kernel is not in the trace"
    copy_ns = statistics.median(timed["copy"][1])
    ceiling = 2 * meta["copy_bytes"] / (copy_ns * 1e-9)           # bytes moved per second: read + write
    print(f"{points} scan points, {meta['reps']} launches per kernel after {warmup} warm-up launches")
    print(f"copy ceiling: {ceiling / 1e12:.2f} TB/s (1 GiB read + 1 GiB written, median {copy_ns / 1e3:.1f} us, "
          f"min {min(timed['copy'][1]) / 1e3:.1f}, max {max(timed['copy'][1]) / 1e3:.1f})")
    print("| kind | kernel | median (us) | min | max | bytes / point (read + written) | GB/s | fraction of the copy ceiling |\n|---|---|---|---|---|---|---|---|")
    for c in sorted(k for k in timed if k != "copy"):
        name, ns = timed[c]
        med = statistics.median(ns)
        rd, wr = BYTES[c]
        rate = (rd + wr) * points / (med * 1e-9)
        short = re.search(r"k_\w+<[^>]*>", name).group(0)
        print(f"| {c[0]} | {c[1]} `{short}` | {med / 1e3:.1f} | {min(ns) / 1e3:.1f} | {max(ns) / 1e3:.1f} | {rd} + {wr} | {rate / 1e9:.0f} | {rate / ceiling:.2f} |")


def coreset_probe(reps):
    np, pcr, _capi, scan, T, regs = setup(1_060_000)
    reg = regs["plane"]
    ctx = _capi.get_context(0)
    J, r, w = reg.linearize(T, scan)
    keep = w > 0
    J2, r1 = np.ascontiguousarray(J[keep, 0, :]), np.ascontiguousarray(r[keep, 0])
    u = np.ones(len(r1))
    handle = reg.upload(scan, keep_order=True)

    def host_route():
        P = pcr.create_gn_set(J2, r1)
        return pcr.fast_caratheodory(P, u, 64, 1024)

    def host_route_coreset_only(P):
        return pcr.fast_caratheodory(P, u, 64, 1024)

    def device_route():
        return reg.coreset(T, handle, N_target=1024, k=64)

    P = pcr.create_gn_set(J2, r1)
    times = {"host: create_gn_set + fast_caratheodory": [], "host: fast_caratheodory alone": [], "device: coreset": []}
    for it in range(reps + 2):
        for key, fn in (("host: create_gn_set + fast_caratheodory", host_route),
                        ("host: fast_caratheodory alone", lambda: host_route_coreset_only(P)), ("device: coreset", device_route)):
            ctx.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ctx.synchronize()
            if it >= 2:
                times[key].append((time.perf_counter() - t0) * 1e3)
    print(f"gated-in points: {int(keep.sum())} of {len(scan)}; N_target 1024, k 64; {reps} repetitions after 2 warm-up rounds")
    print("| route | median (ms) | min | max |\n|---|---|---|---|")
    for key, v in times.items():
        print(f"| {key} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |")
    ind, wts = device_route()
    H, g, e2 = reg.calc_H_g_e2(T, scan)
    Hc, gc, ec = reg.calc_H_g_e2(T, np.ascontiguousarray(scan[ind]), weights=wts)
    print(f"device route: {len(ind)} points, max |dH| / max |H| {np.max(np.abs(H - Hc)) / np.max(np.abs(H)):.2e}, |de2| / e2 {abs(e2 - ec) / e2:.2e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", choices=["kernels"])
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--report", help="the kernel trace CSV of a --child kernels run")
    ap.add_argument("--meta", help="JSON file the child writes and the report reads")
    ap.add_argument("--coreset", action="store_true")
    args = ap.parse_args()
    if args.child == "kernels":
        child_kernels(args.points, args.reps, args.meta)
    elif args.report:
        if not args.meta:
            ap.error("--report needs --meta (written by the --child kernels run)")
        report(args.report, args.meta)
    elif args.coreset:
        coreset_probe(args.reps)
    else:
        ap.error("one of --child kernels, --report CSV, --coreset")
