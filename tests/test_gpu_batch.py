"""Batched alignment on the GPU: every item of a batch -- sums, trace rows, iteration count, pose -- is BIT-IDENTICAL to the
single path over that scan alone (the batched kernel gives TileIter, the ticket fold and the Gauss-Newton step the arguments
a single fused launch gives them), items do not influence each other, a singular item stays its own problem, and the
reference's results come out through the new door."""

import ctypes as C

import numpy as np
import pytest

from conftest import rel_H

pytestmark = pytest.mark.gpu

TOL_REF = 1e-5
NAMES = ["icp", "plane", "vplane", "ndt"]
LOOP_CASES = ((0, 1e-3), (1, 1e-3), (2, 1e-3), (3, 1e9), (30, 1e-3))     # those of test_align_loop_edge_cases


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


def _pose_close(T, ref, tol=1e-4):
    dR = T[:3, :3] @ ref[:3, :3].T
    ang = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    return np.max(np.abs(T[:3, 3] - ref[:3, 3])) < tol and ang < tol


@pytest.fixture(scope="module")
def regs(capi, g2):
    """The four classes with g2's target set (PlaneICP with the reference's normals)."""
    import point_cloud_registration_amd as pcr
    md, vs, k = float(g2["max_dist"]), float(g2["voxel_size"]), int(g2["k"])
    r = {"icp": pcr.ICP(max_dist=md), "plane": pcr.PlaneICP(max_dist=md, k=k),
         "vplane": pcr.VPlaneICP(voxel_size=vs, max_dist=md), "ndt": pcr.NDT(voxel_size=vs, max_dist=md)}
    for name, obj in r.items():
        if name == "plane":
            obj.set_target(g2["target"], "given", g2["plane_normals"])
        else:
            obj.set_target(g2["target"])
    return r


def _single_align(capi, target, scan, kind, T0, max_iter, tol, md):
    """pcr_align(PCR_FLAG_DEVICE_LOOP) of one scan, WITHOUT turning a singular item into an exception:
    (status, T, iterations, trace rows)."""
    T0 = np.ascontiguousarray(T0, dtype=np.float64).reshape(16)
    T, iters, trace = np.zeros(16), C.c_int(0), np.zeros((max(max_iter, 1), 45))
    st = capi.lib().pcr_align(target.handle, scan.handle, int(kind), T0, int(max_iter), float(tol), float(md),
                              capi.FLAG_ICP_RR_QUIRK | capi.FLAG_DEVICE_LOOP, T, C.byref(iters), trace.ctypes.data_as(C.c_void_p))
    assert st in (capi.PCR_OK, capi.PCR_ERR_SINGULAR), capi.lib().pcr_last_error()
    return st, T.reshape(4, 4), iters.value, trace[:iters.value]


def _mixed_items(g2):
    """g2's source, prefixes of 1 / 255 / 256 / 257 / 1000 points, an empty scan, g2's source again at g2's T: distinct arrays,
    the scan index of every item, the poses."""
    src, T = g2["source"], np.array(g2["T"])
    arrays = [src, src[:1], src[:255], src[:256], src[:257], src[:1000], np.zeros((0, 3), np.float32)]
    item_scan = [0, 1, 2, 3, 4, 5, 6, 0]
    Ts = np.stack([np.eye(4), T, np.eye(4), T, np.eye(4), T, np.eye(4), T])
    return arrays, item_scan, Ts


def _check_items_against_single(capi, ctx, target, kind, md, arrays, item_scan, Ts, loop_cases=LOOP_CASES):
    """Every item of the batch against the single path over its scan alone; returns the batch results of the last loop case."""
    batch = capi.ScanBatch(ctx, arrays)
    singles = [capi.Scan(ctx, a) for a in arrays]
    assert batch.size() == (len(arrays), sum(a.shape[0] for a in arrays))
    B = len(item_scan)
    out = capi.linearize_batch(target, batch, kind, Ts, md, item_scan=item_scan)
    for i in range(B):
        alone = capi.linearize(target, singles[item_scan[i]], kind, Ts[i], md)
        assert np.array_equal(out[i], alone), (i, np.max(np.abs(out[i] - alone)))
    res = None
    for max_iter, tol in loop_cases:
        Tb, itb, stb, trb = capi.align_batch(target, batch, kind, Ts, max_iter, tol, md, item_scan=item_scan, want_trace=True)
        for i in range(B):
            st, T1, it1, tr1 = _single_align(capi, target, singles[item_scan[i]], kind, Ts[i], max_iter, tol, md)
            what = (i, max_iter, tol)
            assert stb[i] == st and itb[i] == it1, (what, stb[i], st, itb[i], it1)
            assert np.array_equal(Tb[i], T1), what
            assert np.array_equal(trb[i, :it1], tr1) and not trb[i, it1:].any(), what
        res = (Tb, itb, stb, trb)
    batch.close()
    for s in singles:
        s.close()
    return res


@pytest.mark.parametrize("name", NAMES)
def test_equality_with_the_single_path(capi, ctx, g2, regs, name):
    """1. Items of different sizes and poses (an empty scan among them) under the fused pipeline: linearize rows, iteration
    counts, poses and traces equal to the single path, bit for bit, for every loop case."""
    arrays, item_scan, Ts = _mixed_items(g2)
    with ctx.pipeline(variant=0, fuse_finalize=1, nn_mode=0, reuse=0):
        Tb, itb, stb, trb = _check_items_against_single(capi, ctx, regs[name]._target, regs[name].KIND, float(g2["max_dist"]),
                                                        arrays, item_scan, Ts)
    # the empty scan is what it is on the single path: zero correspondences, singular at the first solve, pose untouched
    assert stb[6] == capi.PCR_ERR_SINGULAR and itb[6] == 1 and np.array_equal(Tb[6], Ts[6])
    assert stb[0] == capi.PCR_OK and stb[7] == capi.PCR_OK


@pytest.mark.parametrize("name", NAMES)
def test_items_are_independent(capi, ctx, g2, regs, name):
    """2. An item's outputs do not depend on what else is in the batch or where it stands."""
    arrays, item_scan, Ts = _mixed_items(g2)
    tgt, kind, md = regs[name]._target, regs[name].KIND, float(g2["max_dist"])
    B = len(item_scan)
    with ctx.pipeline(variant=0, fuse_finalize=1, nn_mode=0, reuse=0):
        batch = capi.ScanBatch(ctx, arrays)
        ref_out = capi.linearize_batch(tgt, batch, kind, Ts, md, item_scan=item_scan)
        ref = capi.align_batch(tgt, batch, kind, Ts, 30, 1e-3, md, item_scan=item_scan, want_trace=True)
        # the same call again
        again = capi.align_batch(tgt, batch, kind, Ts, 30, 1e-3, md, item_scan=item_scan, want_trace=True)
        assert all(np.array_equal(x, y) for x, y in zip(ref, again))
        assert np.array_equal(ref_out, capi.linearize_batch(tgt, batch, kind, Ts, md, item_scan=item_scan))
        # permuted
        perm = np.random.default_rng(3).permutation(B)
        p_scan = [item_scan[j] for j in perm]
        out = capi.linearize_batch(tgt, batch, kind, Ts[perm], md, item_scan=p_scan)
        got = capi.align_batch(tgt, batch, kind, Ts[perm], 30, 1e-3, md, item_scan=p_scan, want_trace=True)
        assert np.array_equal(out, ref_out[perm])
        assert all(np.array_equal(x, y[perm]) for x, y in zip(got, ref))
        # every item alone, as a batch of one
        for i in range(B):
            one = capi.align_batch(tgt, batch, kind, Ts[i:i + 1], 30, 1e-3, md, item_scan=[item_scan[i]], want_trace=True)
            assert all(np.array_equal(x[0], y[i]) for x, y in zip(one, ref)), i
            assert np.array_equal(capi.linearize_batch(tgt, batch, kind, Ts[i:i + 1], md, item_scan=[item_scan[i]])[0], ref_out[i])
        batch.close()


@pytest.mark.parametrize("name", NAMES)
def test_one_bad_item(capi, ctx, g2, regs, name):
    """3. An item a kilometre away has zero correspondences: PCR_ERR_SINGULAR with its start pose, for that item only."""
    src = g2["source"]
    far = (src + np.float32(1000.0)).astype(np.float32)
    T = np.array(g2["T"])
    arrays, item_scan, Ts = [src, far, src[:1000]], [0, 1, 2, 0], np.stack([np.eye(4), T, T, T])
    reg = regs[name]
    with ctx.pipeline(variant=0, fuse_finalize=1, nn_mode=0, reuse=0):
        Tb, itb, stb, trb = _check_items_against_single(capi, ctx, reg._target, reg.KIND, float(g2["max_dist"]), arrays, item_scan, Ts,
                                                        loop_cases=((30, 1e-3),))
        assert stb.tolist() == [capi.PCR_OK, capi.PCR_ERR_SINGULAR, capi.PCR_OK, capi.PCR_OK]
        assert itb[1] == 1 and np.array_equal(Tb[1], Ts[1]) and trb[1, 0, 16 + 28] == 0
        sources = [arrays[k] for k in item_scan]
        with pytest.raises(np.linalg.LinAlgError, match=r"\[1\]"):
            reg.align_batch(sources, Ts)
        assert reg.last_batch_status.tolist() == stb.tolist()
        Tc, info = reg.align_batch(sources, Ts, return_info=True)
        assert info["singular"] == [1] and info["status"].tolist() == stb.tolist() and info["iterations"].tolist() == itb.tolist()
        assert np.array_equal(Tc, Tb) and info["correspondences"][1] == 0 and info["correspondences"][0] > 0
        H, g, e2 = reg.calc_H_g_e2_batch(Ts, sources)
        assert not H[1].any() and not g[1].any() and e2[1] == 0 and reg.last_batch_correspondences[1] == 0


@pytest.mark.parametrize("name", NAMES)
def test_multi_start(capi, ctx, g2, regs, name):
    """4. One scan, 8 start poses through the single-array form: 8 single aligns; the points are held once."""
    from point_cloud_registration_amd.math_tools import plus
    src, T = g2["source"], np.array(g2["T"])
    rng = np.random.default_rng(11)
    Ts = [np.eye(4), T] + [plus(T, np.concatenate([rng.normal(0, 0.03, 3), rng.normal(0, 0.01, 3)])) for _ in range(6)]
    Ts = np.stack(Ts)
    reg = regs[name]
    md = float(g2["max_dist"])
    with ctx.pipeline(variant=0, fuse_finalize=1, nn_mode=0, reuse=0):
        Tb, info = reg.align_batch(src, Ts, return_info=True)
        assert Tb.shape == (8, 4, 4) and Tb.dtype == np.float64
        scan = capi.Scan(ctx, src)
        for i in range(8):
            st, T1, it1, tr1 = _single_align(capi, reg._target, scan, reg.KIND, Ts[i], reg.max_iter, reg.tol, md)
            assert info["status"][i] == st and info["iterations"][i] == it1 and np.array_equal(Tb[i], T1), i
            assert info["correspondences"][i] == int(round(tr1[it1 - 1, 16 + 28]))
        H, g, e2 = reg.calc_H_g_e2_batch(Ts, src)
        for i in range(8):
            H1, g1, e21, _ = capi.unpack29(capi.linearize(reg._target, scan, reg.KIND, Ts[i], md))
            assert np.array_equal(H[i], H1) and np.array_equal(g[i], g1) and e2[i] == e21
        batch = capi.ScanBatch(ctx, [src])
        assert batch.size() == (1, src.shape[0])
        T8, it8, st8 = capi.align_batch(reg._target, batch, reg.KIND, Ts, reg.max_iter, reg.tol, md, item_scan=[0] * 8)
        assert np.array_equal(T8, Tb) and batch.size() == (1, src.shape[0])
        batch.close()
    # the same array object several times in a sequence is the same batch
    T_seq = reg.align_batch([src] * 8, Ts, return_info=True)[0]
    assert np.array_equal(T_seq, Tb)


@pytest.mark.parametrize("name", NAMES)
def test_reference_parity_through_the_new_door(capi, g2, regs, name):
    """5. The reference's own alignment of g2 and its normal equations at g2's T, through align_batch / calc_H_g_e2_batch."""
    reg = regs[name]
    T = reg.align_batch([g2["source"]], np.eye(4))
    assert T.shape == (1, 4, 4)
    assert reg.last_batch_iterations[0] == g2[f"align_{name}_T"].shape[0]
    assert _pose_close(T[0], g2[f"align_{name}_final"])
    assert reg.last_batch_status[0] == 0 and reg.last_batch_correspondences[0] > 0
    H, g, e2 = reg.calc_H_g_e2_batch(g2["T"], [g2["source"]])
    assert H.shape == (1, 6, 6) and g.shape == (1, 6) and e2.shape == (1,)
    assert rel_H(H[0], g2[f"T_{name}_H"]) < TOL_REF


@pytest.fixture(scope="module")
def b01():
    from point_cloud_registration_amd.synthetic import street, harness_scan
    target = street(1_060_000, seed=0)
    return {"target": target, "scans": [harness_scan(target, 100_000, seed=s) for s in (1, 2, 3, 4)],
            "big": harness_scan(target, 300_000, seed=9)}


@pytest.mark.parametrize("name", NAMES)
def test_default_pipeline_larger_items(capi, ctx, b01, name):
    """6. B-01 stand-in under the DEFAULT pipeline: four 100 k-point harness scans (below the fused crossover: the single
    align runs the same kernel, so equal bits); one 300 k-point item (above it: the single path runs search + reduce, only
    the order of summation differs -- the 1e-12 of test_scan_order_independence)."""
    import point_cloud_registration_amd as pcr
    reg = {"icp": pcr.ICP, "plane": pcr.PlaneICP, "vplane": pcr.VPlaneICP, "ndt": pcr.NDT}[name](max_iter=30, tol=1e-3, max_dist=2.0)
    reg.set_target(b01["target"])
    assert ctx.get_pipeline()["variant"] == 2
    Tb = reg.align_batch(b01["scans"])
    itb = reg.last_batch_iterations.copy()
    for i, scan in enumerate(b01["scans"]):
        T1 = reg.align(scan)
        assert reg.last_iterations == itb[i] and np.array_equal(Tb[i], T1), (i, itb[i], reg.last_iterations)
    big = b01["big"]
    Hb, gb, e2b = reg.calc_H_g_e2_batch(np.eye(4), [big])
    cnt = reg.last_batch_correspondences[0]
    H1, g1, e21 = reg.calc_H_g_e2(np.eye(4), big)
    assert cnt == reg.last_correspondences
    assert np.allclose(Hb[0], H1, rtol=1e-12, atol=1e-12) and np.allclose(gb[0], g1, rtol=1e-12, atol=1e-12)
    assert np.allclose(e2b[0], e21, rtol=1e-12, atol=1e-12)
    Tbig = reg.align_batch([big])[0]
    T1 = reg.align(big)
    assert reg.last_batch_iterations[0] == reg.last_iterations and _pose_close(Tbig, T1)


def test_no_growth(capi, ctx, g2, regs):
    """7. 50 create / align / destroy cycles of a batch leave device memory where it was once the block cache is trimmed."""
    import gc
    import torch
    arrays, item_scan, Ts = _mixed_items(g2)
    reg = regs["plane"]
    md = float(g2["max_dist"])

    def cycle():
        batch = capi.ScanBatch(ctx, arrays)
        capi.align_batch(reg._target, batch, reg.KIND, Ts, 30, 1e-3, md, item_scan=item_scan, want_trace=True)
        capi.linearize_batch(reg._target, batch, reg.KIND, Ts, md, item_scan=item_scan)
        batch.close()

    cycle(); gc.collect(); ctx.trim()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        cycle()
    gc.collect(); ctx.trim()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20


def test_unsupported_configurations_are_refused(capi, ctx, g2):
    """Out of scope, refused with a clear error: PlaneICP over a float64 point target (quirk Q6), a context with a communicator."""
    import point_cloud_registration_amd as pcr
    reg = pcr.PlaneICP(max_dist=float(g2["max_dist"]), k=int(g2["k"]))
    reg.set_target(g2["target"].astype(np.float64))
    assert getattr(reg._target, "has_f64", False)          # (g2's coordinates are well inside float32 range)
    with pytest.raises(capi.PcrError, match="float64"):
        reg.align_batch([g2["source"]])
    with pytest.raises(capi.PcrError, match="float64"):
        reg.calc_H_g_e2_batch(np.eye(4), [g2["source"]])
    batch = capi.ScanBatch(ctx, [g2["source"]])
    icp = pcr.ICP(max_dist=float(g2["max_dist"]))
    icp.set_target(g2["target"])
    with pytest.raises(ValueError):
        capi.align_batch(icp._target, batch, capi.ICP, np.eye(4)[None], 30, 1e-3, 0.5, item_scan=[1])      # no such scan
    with pytest.raises(ValueError):
        capi.linearize_batch(icp._target, batch, capi.ICP, np.stack([np.eye(4)] * 2), 0.5)                 # 2 items, 1 scan, no map
    # a context with a communicator attached (here: one rank): PCR_ERR_UNSUPPORTED from both entry points, whatever the flags
    ok = capi.linearize_batch(icp._target, batch, capi.ICP, np.eye(4)[None], 0.5)
    ctx.comm_init(capi.comm_unique_id(), 1, 0)
    try:
        for flags in (capi.FLAG_ICP_RR_QUIRK, capi.FLAG_ICP_RR_QUIRK | capi.FLAG_LOCAL_ONLY):
            with pytest.raises(capi.PcrError, match="communicator"):
                capi.linearize_batch(icp._target, batch, capi.ICP, np.eye(4)[None], 0.5, flags)
            with pytest.raises(capi.PcrError, match="communicator"):
                capi.align_batch(icp._target, batch, capi.ICP, np.eye(4)[None], 30, 1e-3, 0.5, flags)
    finally:
        ctx.comm_destroy()
    assert np.array_equal(ok, capi.linearize_batch(icp._target, batch, capi.ICP, np.eye(4)[None], 0.5))
    batch.close()
