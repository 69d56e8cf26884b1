"""Worker of tests/test_gpu_group.py::test_group_at_scale (a script, not a test module): single-process groups of N contexts of
GPU 0 on the pipelines that large shards run -- ``python tests/group_scale_check.py <scenario> <N> <out.npz>``.  Exit code 0
and GROUP_SCALE_OK = every check passed; every sum, pose, trace and iteration count it produced is saved to out.npz, so that
the test can compare runs.

"SPMD sums": every shard (distributed.shard_scan) run on one plain context with FLAG_LOCAL_ONLY under the same pipeline, the
local sums added in rank order starting from 0.0 -- what k_p2p_allreduce (csrc/comm.hip) does.

Scenarios:
  b01       the g8 fixture (the reference on the 1.06 M-point B-01 stand-in): all five kinds on the full perturbed scan and the
            100 k one; which pipeline every member ran (profiling counters); the group's sums against the SPMD sums (bits), the
            oracle (1e-9) and the reference (the bars of test_g8_hip_matches_reference_at_b01_size); every member's matches;
            device-resident loop against host loop, trace rows against group_linearize; a sequence of exchanges (short aligns,
            a singular align, 70 passes through the 64-slot table)
  straddle  N = 2 over 2 C + 1 points (C = CUs x 1024, the crossover of variant 2): member 0 runs split, member 1 fused
  tiny      N = 8 over scans of 1 to 9 points: members with empty shards
  lidar     the g11 LiDAR sweep (heavy-cell index, its LB search kernels under PCR_VARIANT=1)
"""
import os
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from point_cloud_registration_amd import _capi, distributed as pdist      # noqa: E402
from conftest import load_golden, rel_H, step_err                         # noqa: E402
from oracle import oracle as orc                                          # noqa: E402

FL = _capi.FLAG_ICP_RR_QUIRK
LOCAL = FL | _capi.FLAG_LOCAL_ONLY
OKIND = {_capi.ICP: orc.ICP, _capi.PLANE: orc.PLANE, _capi.VPLANE: orc.VPLANE, _capi.NDT: orc.NDT}
OUT = {}


def same(a, b):
    """Bit for bit (NaN payloads and signed zeros included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def save(key, val):
    assert key not in OUT, key
    OUT[key] = np.asarray(val)


def crossover():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 1024


class Pair:
    """One target on the group and the same target on the plain context, one scan sharded on both."""

    def __init__(self, grp, ctx, n, gt, pt):
        self.grp, self.ctx, self.n, self.gt, self.pt = grp, ctx, n, gt, pt

    def scans(self, scan):
        gs = _capi.Scan(self.grp, scan)
        shards = [_capi.Scan(self.ctx, np.ascontiguousarray(pdist.shard_scan(scan, r, self.n))) for r in range(self.n)]
        return gs, shards

    def spmd(self, shards, kind, T, md):
        tot = np.zeros(29)
        for sc in shards:
            tot = tot + _capi.linearize(self.pt, sc, kind, T, md, LOCAL)
        return tot


def check_pipeline(grp, n, gs, tag):
    """Which kernels every member launched since the last reset: search + reduce (k_nn_scan + k_reduce_finalize) where its
    shard is above the crossover of variant 2 or PCR_VARIANT=1, the fused small-scan kernel otherwise, and the exchange."""
    C = crossover()
    split = []
    for i in range(n):
        c = grp.member(i)
        prof = c.profile_read()
        ni, v = gs.member(i).n, c.get_variant()
        want = v == 1 or (v == 2 and ni > C)
        lin, nn, red, ar = (prof[k][0] for k in ("linearize", "nn", "reduce", "allreduce"))
        if want:
            assert nn > 0 and red > 0 and lin == 0, (tag, i, ni, v, prof)
        else:
            assert lin > 0 and nn == 0 and red == 0, (tag, i, ni, v, prof)
        assert n == 1 or ar > 0, (tag, i, prof)
        c.profile_reset()
        split.append(want)
    save(f"{tag}_split", split)
    return split


def check_oracle(out, kind, otgt, T, scan, md, tag):
    H, g, e2, cnt = _capi.unpack29(out)
    Ho, go, e2o, cnto = orc.calc_H_g_e2(OKIND[kind], otgt, T, scan, md, with_count=True)
    assert cnt == cnto, (tag, cnt, cnto)
    if cnto:
        assert rel_H(H, Ho) <= 1e-9, (tag, rel_H(H, Ho))
        assert np.max(np.abs(g - go)) <= 1e-9 * max(np.max(np.abs(H)), np.max(np.abs(go)), 1e-300), tag
        assert abs(e2 - e2o) <= 1e-9 * max(abs(e2o), 1e-300), (tag, e2, e2o)


def check_ref(out, Hr, gr, e2r, g0, step_bar, tag):
    H, g, e2, cnt = _capi.unpack29(out)
    assert rel_H(H, Hr) <= 1e-5, (tag, rel_H(H, Hr))
    assert np.max(np.abs(g - gr)) <= 1e-4 * np.max(np.abs(g0)), tag
    assert abs(e2 - e2r) <= 1e-4 * abs(e2r), (tag, e2, e2r)
    assert step_err(H, g, Hr, gr) <= step_bar, (tag, step_err(H, g, Hr, gr))


def oracle_voxels(tgt, vs):
    """The oracle's nearest-centroid target on the GPU's own voxel statistics (member 0's)."""
    st = tgt.voxel_stats(("mean", "norm", "icov"))
    ov = orc.TargetVoxels.__new__(orc.TargetVoxels)
    ov.mean, ov.norm, ov.icov = st["mean"], st["norm"], st["icov"]
    ov.icov6 = np.ascontiguousarray(ov.icov.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]])
    ov._brute = ov.mean.shape[0] <= 4096
    if not ov._brute:
        ov.grid = orc.Grid(ov.mean, vs)
    return ov


def align_both(gt, gs, kind, T0, max_iter, md, tag):
    """Device-resident loop and host loop of the group: bit-identical pose, iteration count and trace.  Returns
    (T, iterations, trace), or None when both raised the singular-matrix error."""
    res = []
    for fl in (_capi.FLAG_DEVICE_LOOP, _capi.FLAG_HOST_LOOP):
        try:
            res.append(_capi.align(gt, gs, kind, T0, max_iter, 1e-3, md, FL | fl, want_trace=True))
        except np.linalg.LinAlgError:
            res.append(None)
    if res[0] is None or res[1] is None:
        assert res[0] is None and res[1] is None, (tag, "one loop singular, the other not")
        return None
    (Td, itd, trd), (Th, ith, trh) = res
    assert same(Td, Th) and itd == ith and same(trd, trh), (tag, "device loop != host loop", itd, ith)
    save(f"{tag}_T", Td), save(f"{tag}_its", itd), save(f"{tag}_trace", trd)
    return Td, itd, trd


def trace_rows_match(gt, gs, kind, trace, md, tag):
    """The 29 sums of every trace row = group_linearize at that row's pose (device-decided hand-out and list set against
    host-driven passes)."""
    for k, row in enumerate(trace):
        assert same(row[16:], _capi.linearize(gt, gs, kind, row[:16].reshape(4, 4), md)), (tag, "trace row", k)


def pose_err(T, ref):
    dR = T[:3, :3] @ ref[:3, :3].T
    return float(np.max(np.abs(T[:3, 3] - ref[:3, 3]))), float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))


# ------------------------------------------------------------------------------------------------------------------ b01
def g8_clouds():
    from point_cloud_registration_amd.synthetic import street, perturbed_scan, street_normals
    g = load_golden("g8_b01_fullsize.npz")
    target = street(int(g["n"]), seed=0)
    clouds = {"target": target, "pert100k": perturbed_scan(target, 100_000, seed=2)[0],
              "pertfull": perturbed_scan(target, None, seed=2)[0], "given_normals": street_normals(target)}
    for name, arr in clouds.items():
        assert zlib.crc32(arr.tobytes()) == int(g[f"crc32_{name}"]), f"{name}: the generator no longer reproduces the fixture's cloud"
    g.update(clouds)
    return g


def g8_targets(g8, grp, ctx, n):
    target, md, vs = g8["target"], float(g8["max_dist"]), float(g8["voxel_size"])
    own_g, own_p = _capi.Target.points(grp, target), _capi.Target.points(ctx, target)
    normals = own_g.estimate_normals(int(g8["k"]), compat=True)                 # pcr_group_target_estimate_normals
    assert same(normals, own_p.estimate_normals(int(g8["k"]), compat=True)), "group normals != one context's"
    for i in range(n):
        assert same(own_g.member(i).get_normals(), normals), ("member", i, "normals")
    giv_g, giv_p = (_capi.Target.points(c, target, g8["given_normals"]) for c in (grp, ctx))
    vox_g, vox_p = (_capi.Target.voxels(c, target, vs, 10) for c in (grp, ctx))
    for i in range(n):
        assert vox_g.member(i).size() == int(g8["n_voxels"]), ("member", i, "voxels")
    assert vox_p.size() == int(g8["n_voxels"])
    o_own = orc.TargetPoints(target, normals=normals)
    o_giv = orc.TargetPoints(target, normals=g8["given_normals"])
    o_vox = oracle_voxels(vox_g, vs)
    return {"icp": (_capi.ICP, Pair(grp, ctx, n, own_g, own_p), o_own),
            "plane": (_capi.PLANE, Pair(grp, ctx, n, own_g, own_p), o_own),
            "planeg": (_capi.PLANE, Pair(grp, ctx, n, giv_g, giv_p), o_giv),
            "vplane": (_capi.VPLANE, Pair(grp, ctx, n, vox_g, vox_p), o_vox),
            "ndt": (_capi.NDT, Pair(grp, ctx, n, vox_g, vox_p), o_vox)}


def scenario_b01(n):
    g8 = g8_clouds()
    md = float(g8["max_dist"])
    grp, ctx = _capi.Group([0] * n), _capi.get_context(0)
    for i in range(n):
        grp.member(i).profile_enable(True)
    tg = g8_targets(g8, grp, ctx, n)
    scans = {}
    for sname in ("pertfull", "pert100k"):
        scans[sname] = tg["icp"][1].scans(g8[sname])
    split_full = None
    for cname, (kind, pr, otgt) in tg.items():
        for sname in ("pertfull", "pert100k"):
            # the poses: the reference's trajectory on this scan, or (voxel kinds on the full scan) the 100 k scan's
            src = f"{sname}_{cname}" if f"{sname}_{cname}_T" in g8 else f"pert100k_{cname}"
            if cname in ("icp", "plane", "planeg") and sname == "pert100k":
                continue                                  # (their trajectories on the full scan are the fixture's B-01 runs)
            gs, shards = scans[sname]
            for i in range(n):
                grp.member(i).profile_reset()
            Ts, lin = g8[f"{src}_T"], []
            for k in range(Ts.shape[0]):
                tag = f"{sname}_{cname}_{k}"
                out = _capi.linearize(pr.gt, gs, kind, Ts[k], md)
                assert same(out, pr.spmd(shards, kind, Ts[k], md)), (tag, "group sums != SPMD sums")
                check_oracle(out, kind, otgt, Ts[k], g8[sname], md, tag)
                if src == f"{sname}_{cname}":
                    check_ref(out, g8[f"{src}_H"][k], g8[f"{src}_g"][k], g8[f"{src}_e2"][k], g8[f"{src}_g"][0],
                              1e-4 if cname == "plane" else 5e-5, tag)
                lin.append(out)
            save(f"{sname}_{cname}_lin", lin)
            split = check_pipeline(grp, n, gs, f"{sname}_{cname}")
            if sname == "pertfull":
                split_full = split
            # every split member's correspondences = the plain context's for the same shard (the SPMD pass just ran there)
            for i in range(n):
                if split[i]:
                    assert same(gs.member(i).matches(), shards[i].matches()), (sname, cname, "member", i, "matches")
            # group_align: device loop == host loop; the reference's iteration count and final pose; trace rows
            tag = f"{sname}_{cname}_align"
            Ta, its, tr = align_both(pr.gt, gs, kind, np.eye(4), 30, md, tag)
            if src == f"{sname}_{cname}":
                assert its == g8[f"{src}_T"].shape[0], (tag, its)
                dt, dr = pose_err(Ta, g8[f"{src}_final"])
                assert dt <= 1e-4 and dr <= 1e-4, (tag, dt, dr)
            trace_rows_match(pr.gt, gs, kind, tr, md, tag)
            if sname == "pertfull":
                exchange_sequence(pr, gs, shards, kind, g8[f"{src}_final"], its, tr, md, f"{sname}_{cname}")
        print(f"b01[{n}] {cname}: ok", flush=True)
    # the deeper list set exists on the first and the last member wherever the members ran search + reduce passes
    for cname in ("icp", "planeg"):
        gt = tg[cname][1].gt
        for i in (0, n - 1):
            rec = gt.member(i).index_info()["halo2_records"]
            save(f"halo2_{cname}_{i}", rec)
            if split_full[i]:
                assert rec > 0, (cname, "member", i, "has no deeper list set")


def exchange_sequence(pr, gs, shards, kind, T_fin, its, tr, md, tag):
    """Exchanges after the reference-length align: short aligns (their poses = the long run's trace), an align from the final
    pose, a singular align (all members alike, no PCR_ERR_COMM), then 70 passes -- the 64-slot table wraps with the dead
    iterations of the aligns inside it."""
    for m in (1, 3):
        T, it = _capi.align(pr.gt, gs, kind, np.eye(4), m, 1e-3, md)
        save(f"{tag}_short{m}_T", T), save(f"{tag}_short{m}_its", it)
        if its > m:
            assert it == m and same(T, tr[m][:16].reshape(4, 4)), (tag, "max_iter", m)
    T, it = _capi.align(pr.gt, gs, kind, T_fin, 30, 1e-3, md)
    assert it < 30, (tag, "align from the final pose", it)
    save(f"{tag}_fromfinal_T", T), save(f"{tag}_fromfinal_its", it)
    far = np.array(T_fin, dtype=np.float64)
    far[:3, 3] += 1000.0
    try:
        _capi.align(pr.gt, gs, kind, far, 30, 1e-3, md)
        raise AssertionError((tag, "align 1 km off did not fail"))
    except np.linalg.LinAlgError:
        pass                                                  # PCR_ERR_SINGULAR from every member (PCR_ERR_COMM raises PcrError)
    rng = np.random.default_rng(7)
    xs = []
    for i in range(70):
        Tq = np.array(T_fin, dtype=np.float64)
        Tq[:3, 3] += rng.normal(0, 0.05, 3)
        o = _capi.linearize(pr.gt, gs, kind, Tq, md)
        if i in (0, 12, 13, 63, 64, 69):
            assert same(o, pr.spmd(shards, kind, Tq, md)), (tag, "exchange", i)
        xs.append(o)
    save(f"{tag}_xchg", xs)


# ------------------------------------------------------------------------------------------------------------- straddle
def scenario_straddle(n):
    assert n == 2
    C = crossover()
    g8 = g8_clouds()
    md = float(g8["max_dist"])
    scan = np.ascontiguousarray(g8["pertfull"][:2 * C + 1])
    grp, ctx = _capi.Group([0] * n), _capi.get_context(0)
    for i in range(n):
        grp.member(i).profile_enable(True)
    giv_g, giv_p = (_capi.Target.points(c, g8["target"], g8["given_normals"]) for c in (grp, ctx))
    o_giv = orc.TargetPoints(g8["target"], normals=g8["given_normals"])
    pr = Pair(grp, ctx, n, giv_g, giv_p)
    gs, shards = pr.scans(scan)
    assert gs.member(0).n == C + 1 and gs.member(1).n == C
    for cname, kind in (("planeg", _capi.PLANE), ("icp", _capi.ICP)):
        lin = []
        for k, T in enumerate(g8["pertfull_planeg_T"]):
            out = _capi.linearize(giv_g, gs, kind, T, md)
            assert same(out, pr.spmd(shards, kind, T, md)), (cname, k, "group sums != SPMD sums")
            check_oracle(out, kind, o_giv, T, scan, md, f"straddle_{cname}_{k}")
            lin.append(out)
        save(f"straddle_{cname}_lin", lin)
        split = check_pipeline(grp, n, gs, f"straddle_{cname}")
        assert split == [True, False], ("member 0 must run split and member 1 fused", split)
        Ta, its, tr = align_both(giv_g, gs, kind, np.eye(4), 30, md, f"straddle_{cname}_align")
        trace_rows_match(giv_g, gs, kind, tr, md, f"straddle_{cname}_align")
        print(f"straddle {cname}: {its} iterations, members split / fused", flush=True)


# ----------------------------------------------------------------------------------------------------------------- tiny
def scenario_tiny(n):
    g2 = load_golden("g2_mini_street.npz")
    md, vs = float(g2["max_dist"]), float(g2["voxel_size"])
    target, source = g2["target"], g2["source"].astype(np.float32)
    grp, ctx = _capi.Group([0] * n), _capi.get_context(0)
    pts = Pair(grp, ctx, n, *(_capi.Target.points(c, target, g2["plane_normals"]) for c in (grp, ctx)))
    vox = Pair(grp, ctx, n, *(_capi.Target.voxels(c, target, vs, 10) for c in (grp, ctx)))
    full, full_shards = pts.scans(source)
    kinds = (("icp", _capi.ICP, pts), ("plane", _capi.PLANE, pts), ("vplane", _capi.VPLANE, vox), ("ndt", _capi.NDT, vox))
    for m in (1, 3, 7, 8, 9):
        sub = np.ascontiguousarray(source[:m])
        gs, shards = pts.scans(sub)
        assert sum(gs.member(i).n == 0 for i in range(n)) == max(n - m, 0)
        for cname, kind, pr in kinds:
            tag = f"tiny{m}_{cname}"
            out = _capi.linearize(pr.gt, gs, kind, g2["T"], md)
            assert same(out, pr.spmd(shards, kind, g2["T"], md)), (tag, "group sums != SPMD sums")
            save(f"{tag}_lin", out)
            r = align_both(pr.gt, gs, kind, np.eye(4), 30, md, f"{tag}_align")
            save(f"{tag}_singular", r is None)
            # a normal pass afterwards: the exchange is still in step
            o = _capi.linearize(pr.gt, full, kind, g2["T"], md)
            assert same(o, pr.spmd(full_shards, kind, g2["T"], md)), (tag, "g2 pass after it")
            save(f"{tag}_after", o)
        print(f"tiny: {m} points over {n} members ok", flush=True)


# ---------------------------------------------------------------------------------------------------------------- lidar
def scenario_lidar(n):
    from point_cloud_registration_amd.synthetic import lidar_sweep, lidar_normals, perturbed_scan
    g11 = load_golden("g11_lidar_sweep.npz")
    target = lidar_sweep(int(g11["n"]), seed=0)
    scan = perturbed_scan(target, int(g11["n_scan"]), seed=2)[0]
    normals = lidar_normals(target)
    assert zlib.crc32(target.tobytes()) == int(g11["crc32_target"]), "lidar_sweep() no longer reproduces the fixture's cloud"
    assert zlib.crc32(scan.tobytes()) == int(g11["crc32_scan"]) and zlib.crc32(normals.tobytes()) == int(g11["crc32_normals"])
    md, vs = float(g11["max_dist"]), float(g11["voxel_size"])
    grp, ctx = _capi.Group([0] * n), _capi.get_context(0)
    for i in range(n):
        grp.member(i).profile_enable(True)
        assert grp.member(i).get_variant() == 1, "the lidar scenario runs under PCR_VARIANT=1"
    pts = Pair(grp, ctx, n, *(_capi.Target.points(c, target, normals) for c in (grp, ctx)))
    vox = Pair(grp, ctx, n, *(_capi.Target.voxels(c, target, vs, 10) for c in (grp, ctx)))
    for i in range(n):
        assert pts.gt.member(i).index_info()["heavy"], ("member", i, "heavy index")
        assert vox.gt.member(i).size() == int(g11["n_voxels"])
    gs, shards = pts.scans(scan)
    for cname, kind, pr in (("icp", _capi.ICP, pts), ("planeg", _capi.PLANE, pts), ("vplane", _capi.VPLANE, vox),
                            ("ndt", _capi.NDT, vox)):
        Ts, lin = g11[f"{cname}_T"], []
        for k in range(Ts.shape[0]):
            tag = f"lidar_{cname}_{k}"
            out = _capi.linearize(pr.gt, gs, kind, Ts[k], md)
            assert same(out, pr.spmd(shards, kind, Ts[k], md)), (tag, "group sums != SPMD sums")
            check_ref(out, g11[f"{cname}_H"][k], g11[f"{cname}_g"][k], g11[f"{cname}_e2"][k], g11[f"{cname}_g"][0], 5e-5, tag)
            lin.append(out)
        save(f"lidar_{cname}_lin", lin)
        assert all(check_pipeline(grp, n, gs, f"lidar_{cname}"))
        Ta, its, tr = align_both(pr.gt, gs, kind, np.eye(4), 30, md, f"lidar_{cname}_align")
        assert its == Ts.shape[0], (cname, its, Ts.shape[0])
        dt, dr = pose_err(Ta, g11[f"{cname}_final"])
        assert dt <= 1e-4 and dr <= 1e-4, (cname, dt, dr)
        print(f"lidar[{n}] {cname}: {its} iterations ok", flush=True)


if __name__ == "__main__":
    scenario, n, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    {"b01": scenario_b01, "straddle": scenario_straddle, "tiny": scenario_tiny, "lidar": scenario_lidar}[scenario](n)
    np.savez(out, **OUT)
    print("GROUP_SCALE_OK", flush=True)
