"""Two processes sharing the one GPU of the test box: the sharded GPU path end to end.

RCCL refuses two ranks on the same device, so ``Communicator(ctx, in_library=True)`` must detect the
failure on every rank, agree on it, and fall back to the host all-reduce (gloo) -- exactly the
fallback a broken RCCL set-up would take on a real 8-GPU node.  Each rank runs the HIP kernels on its
scan shard; the result must equal the single-process run on the whole scan."""

import os
import socket
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q, transport=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", PCR_DEVICE="0")
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd import _capi, distributed as pdist
    pdist.init_from_env("gloo")
    g2 = load_golden("g2_mini_street.npz")
    ctx = _capi.get_context(0)
    # RCCL init fails (same GPU twice) -> agreed fallback; the peer-to-peer transport does work between two processes on one GPU
    comm = pdist.Communicator(ctx, in_library=True, transport=transport)
    md, vs = float(g2["max_dist"]), float(g2["voxel_size"])
    shard = pdist.shard_scan(g2["source"], rank, world)
    out = {}
    for name in ("plane", "icp", "vplane", "ndt"):             # all four kinds through the sharded path
        if name == "plane":
            reg = pcr.PlaneICP(max_dist=md, k=int(g2["k"]), comm=comm)
            reg.set_target(g2["target"], None, None)
            reg.set_target(g2["target"], reg.kdtree, g2["plane_normals"])
        elif name == "icp":
            reg = pcr.ICP(max_dist=md, comm=comm); reg.set_target(g2["target"])
        elif name == "vplane":
            reg = pcr.VPlaneICP(voxel_size=vs, max_dist=md, comm=comm); reg.set_target(g2["target"])
        else:
            reg = pcr.NDT(voxel_size=vs, max_dist=md, comm=comm); reg.set_target(g2["target"])
        T = reg.align(shard, np.eye(4))
        H, g, e2 = reg.calc_H_g_e2(g2["T"], shard)
        out[name] = (T, H, reg.last_iterations, reg.last_correspondences)
        if name == "plane" and transport == "p2p" and comm.in_library:
            # 70 exchanges in a row (the 64-slot table wraps) with one rank arriving 50 ms late at the tenth: the others
            # spin inside k_p2p_allreduce (bounded) and must come out with the same sums
            import time
            acc = []
            t_pass = time.perf_counter()
            for i in range(70):
                Tq = np.array(g2["T"], dtype=np.float64); Tq[0, 3] += 1e-3 * i
                if i == 10 and rank == world - 1:
                    time.sleep(0.05)
                Hq, gq, e2q = reg.calc_H_g_e2(Tq, shard)
                acc.append(np.concatenate([Hq.ravel(), gq, [e2q]]))
            # (per-pass wall time of this rank, the 50 ms nap included once: time-sliced ranks on one GPU, so a latency bound on
            # the exchange, not a scaling number -- profiles/r06_p2p_ranks.txt)
            out["wrap"] = (np.array(acc), None, 0, 0)
            out["pass_ms"] = ((time.perf_counter() - t_pass - (0.05 if rank == world - 1 else 0.0)) / 70 * 1e3, None, 0, 0)
    failed = ctx.comm_p2p_failed() if (comm.in_library and comm.transport == "p2p") else False
    q.put((rank, comm.in_library, out, comm.transport, failed))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("transport,world", [("rccl", 2), ("p2p", 2), ("p2p", 4), ("p2p", 8)])
def test_two_ranks_one_gpu_sharded_plane_icp(g2, transport, world):
    """transport "p2p" (round 5): the in-library exchange between two PROCESSES on the one GPU -- IPC-mapped slots, a one-wave
    kernel between fold and hand-off -- which is also the first time the N > 1 branch of the device-resident loop (exchange in
    front of k_gn_update, the top-up of the queue) runs with more than one rank."""
    import multiprocessing as mp            # (not torch.multiprocessing: keep torch out of the parent)
    import queue as queue_mod
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, transport)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    except queue_mod.Empty:
        for p in procs:
            p.kill()
        pytest.fail("a rank did not report within 600 s")
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    (_, lib_a, out_a, tr_a, fail_a) = res[0]
    for (_, lib_b, out_b, tr_b, fail_b) in res[1:]:
        assert lib_a == lib_b and tr_a == tr_b                # every rank took the same transport
    print("transport:", tr_a, "inside libpcr_hip.so" if lib_a else "(host all-reduce, gloo: the agreed fallback)")
    if transport == "p2p":
        # (a silent fallback used to be indistinguishable from the transport under test in the driver's
        # record -- it is a FAILURE now unless the box is known not to offer hipIpc between processes)
        if not lib_a and os.environ.get("PCR_ALLOW_FALLBACK") == "1":
            pytest.skip("hipIpc between processes is not available on this box: the ranks agreed on the host fallback")
        assert lib_a and tr_a == "p2p", "the peer-to-peer transport fell back to the host all-reduce (PCR_ALLOW_FALLBACK=1 tolerates it)"
        assert not any(r[4] for r in res)
        for r in res[1:]:
            assert np.array_equal(res[0][2]["wrap"][0], r[2]["wrap"][0]), "ranks disagree after the wrap / the late rank"
        print(f"p2p world {world}: calc_H_g_e2 of a {2000 // world}-point shard incl. the exchange, ms per pass and rank:",
              [round(r[2]["pass_ms"][0], 4) for r in res])
    for name in ("plane", "icp", "vplane", "ndt"):
        (Ta, Ha, ita, ca) = out_a[name]
        for r in res[1:]:
            (Tb, Hb, itb, cb) = r[2][name]
            assert np.array_equal(Ta, Tb) and np.array_equal(Ha, Hb) and ita == itb and ca == cb, name
        assert ita == g2[f"align_{name}_T"].shape[0], name    # the sharded run = the reference's single-process run
        final = g2[f"align_{name}_final"]
        assert np.max(np.abs(Ta[:3, 3] - final[:3, 3])) < 1e-4, name
        assert np.max(np.abs(Ha - g2[f"T_{name}_H"])) < 1e-5 * np.max(np.abs(g2[f"T_{name}_H"])), name


def _b01_clouds():
    """The g8 cloud, its full perturbed scan and the supplied normals, regenerated and checksum-guarded (as conftest.g8)."""
    import zlib
    from point_cloud_registration_amd.synthetic import street, perturbed_scan, street_normals
    g = load_golden("g8_b01_fullsize.npz")
    target = street(int(g["n"]), seed=0)
    clouds = {"target": target, "pertfull": perturbed_scan(target, None, seed=2)[0], "given_normals": street_normals(target)}
    for name, arr in clouds.items():
        assert zlib.crc32(arr.tobytes()) == int(g[f"crc32_{name}"]), name
    g.update(clouds)
    return g


# what every rank of the run at size evaluates: PlaneICP with the supplied normals at its B-01 trajectory, NDT at the 100 k
# scan's trajectory (the fixture's poses), then one align() each
_AT_SIZE = (("planeg", "pertfull_planeg_T"), ("ndt", "pert100k_ndt_T"))


def _at_size_targets(ctx, g):
    from point_cloud_registration_amd import _capi
    return {"planeg": (_capi.PLANE, _capi.Target.points(ctx, g["target"], g["given_normals"])),
            "ndt": (_capi.NDT, _capi.Target.voxels(ctx, g["target"], float(g["voxel_size"]), 10))}


def _worker_at_size(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", PCR_DEVICE="0")
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    from point_cloud_registration_amd import _capi, distributed as pdist
    pdist.init_from_env("gloo")
    g = _b01_clouds()
    ctx = _capi.get_context(0)
    comm = pdist.Communicator(ctx, in_library=True, transport="p2p")
    md = float(g["max_dist"])
    out = {}
    if comm.in_library:                       # (the agreed host fallback: nothing of the in-library exchange to check)
        sc = _capi.Scan(ctx, np.ascontiguousarray(pdist.shard_scan(g["pertfull"], rank, world)))
        for name, (kind, tgt) in _at_size_targets(ctx, g).items():
            sums = np.array([_capi.linearize(tgt, sc, kind, T, md) for T in g[dict(_AT_SIZE)[name]]])
            T, its = _capi.align(tgt, sc, kind, np.eye(4), 30, 1e-3, md)
            out[name] = (sums, T, its)
    failed = ctx.comm_p2p_failed() if comm.in_library else False
    q.put((rank, comm.in_library, out, comm.transport, failed))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_p2p_ranks_at_b01_size(world):
    """The peer-to-peer transport between PROCESSES at B-01 size: rank r holds shard r of the 1.06 M-point scan (530 k / 353 k
    points: the search + reduce kernels feed the exchange, not the fused small-scan kernel of the g2 cases above).  Ranks are
    bit-identical; every exchanged result equals the SPMD sums computed here shard by shard on one context; at world 2 a
    [0, 0] group in this process returns the same sums, pose and iteration count (include/pcr.h: "what the SPMD run with the
    same sharding returns, bit for bit")."""
    import multiprocessing as mp
    import queue as queue_mod
    from point_cloud_registration_amd import _capi, distributed as pdist
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_worker_at_size, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    except queue_mod.Empty:
        for p in procs:
            p.kill()
        pytest.fail("a rank did not report within 600 s")
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert len({(r[1], r[3]) for r in res}) == 1                # every rank took the same transport
    if not res[0][1] and os.environ.get("PCR_ALLOW_FALLBACK") == "1":
        pytest.skip("hipIpc between processes is not available on this box: the ranks agreed on the host fallback")
    assert res[0][1] and res[0][3] == "p2p", "the peer-to-peer transport fell back to the host all-reduce (PCR_ALLOW_FALLBACK=1 tolerates it)"
    assert not any(r[4] for r in res)
    out = res[0][2]
    for r in res[1:]:
        for name in out:
            assert all(np.array_equal(a, b) for a, b in zip(out[name], r[2][name])), (name, "ranks disagree")
    g = _b01_clouds()
    md = float(g["max_dist"])
    ctx = _capi.get_context(0)
    shards = [_capi.Scan(ctx, np.ascontiguousarray(pdist.shard_scan(g["pertfull"], r, world))) for r in range(world)]
    for name, (kind, tgt) in _at_size_targets(ctx, g).items():
        poses = g[dict(_AT_SIZE)[name]]
        spmd = np.zeros((poses.shape[0], 29))
        for sc in shards:                       # rank order from 0.0, as k_p2p_allreduce adds the slots
            spmd = spmd + np.array([_capi.linearize(tgt, sc, kind, T, md, _capi.FLAG_ICP_RR_QUIRK | _capi.FLAG_LOCAL_ONLY)
                                    for T in poses])
        assert np.array_equal(out[name][0], spmd), (name, "exchanged sums != SPMD sums")
        print(f"p2p world {world} {name}: {out[name][2]} iterations, {int(spmd[0, 28])} correspondences at the first pose")
    if world == 2:
        grp = _capi.get_group((0, 0))          # (process-wide: released after its targets and scans at exit)
        gs = _capi.Scan(grp, g["pertfull"])
        for name, (kind, tgt) in _at_size_targets(grp, g).items():
            sums = np.array([_capi.linearize(tgt, gs, kind, T, md) for T in g[dict(_AT_SIZE)[name]]])
            T, its = _capi.align(tgt, gs, kind, np.eye(4), 30, 1e-3, md)
            assert np.array_equal(sums, out[name][0]), (name, "group sums != the ranks' sums")
            assert np.array_equal(T, out[name][1]) and its == out[name][2], (name, "group align != the ranks' align")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["rccl_then_torch", "torch_then_rccl"])
def test_process_exits_cleanly_with_rccl_and_torch(order):
    """Interpreter exit after RCCL was used through libpcr_hip.so AND torch was imported, in either
    order: must be exit code 0 (regression: librocm_smi64.so in the global symbol scope clashed with
    torch's libamd_smi.so -> 'double free or corruption' in a static destructor)."""
    import subprocess
    import sys
    body = ("from point_cloud_registration_amd import _capi\n"
            "ctx = _capi.get_context(0)\n"
            "ctx.comm_init(_capi.comm_unique_id(), 1, 0); ctx.comm_destroy()\n")
    torch_part = "import torch\ntorch.zeros(4).cuda(); torch.cuda.synchronize()\n"
    code = f"import sys; sys.path.insert(0, {REPO!r})\n" + (body + torch_part if order == "rccl_then_torch" else torch_part + body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
