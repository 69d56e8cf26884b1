"""The host takes the last level of the fold of a host-driven single-GPU pass (pass.hip: pcr_run_linearize; pass_device.h:
ticket_fold_emit with FinArgs::host_rows; gn_math.h: gn_fold8_rows).  PCR_HOST_FOLD=0, read when a context is created, keeps
the device path.

The 29 sums of every case of tests/fold_cases.py with the switch on (this process) and off (a child process) must be equal bit
for bit: PlaneICP (given normals), VPlaneICP and NDT on a 20 k-point street target, scans of 1 ... 20 000 points, the split and
the fused variant, a scan with no match.  Then 70 calls in a row, and host-fold passes mixed with ICP passes (device path), an
align (device-resident loop) and an align_batch on one context, each against its result from a fresh context: a stale group
flag or a ticket that was not re-armed shows there.  Context.host_fold_passes() says which path ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fold_cases as fc
from conftest import REPO

pytestmark = pytest.mark.gpu
HOST_KINDS = ("plane", "vplane", "ndt")


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    assert os.environ.get("PCR_HOST_FOLD", "1") != "0", "this suite compares the default with the switch"
    return _capi


@pytest.fixture(scope="module")
def on(capi):
    ctx = capi.get_context(0)
    before = ctx.host_fold_passes()
    res = fc.run_linearize(capi, ctx)
    return res, ctx.host_fold_passes() - before


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_fold") / "off.npz")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), PCR_HOST_FOLD="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "fold_cases.py"), out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(out))


def test_which_path_ran(capi, on, off):
    res, host_passes = on
    scans = len(fc.SIZES) + 2
    assert len(res) == 4 * scans
    # every pass of the three kinds, both variants, went through the host fold; no ICP pass did; none with the switch off
    assert host_passes == len(HOST_KINDS) * scans * 2
    assert int(off["host_fold_passes"]) == 0


@pytest.mark.parametrize("kind", HOST_KINDS + ("icp",))
def test_host_and_device_fold_agree(kind, on, off):
    res, _ = on
    for s in list(map(str, fc.SIZES)) + ["far"]:
        name = f"{kind}/{s}"
        assert res[name].shape == (2, 29)
        assert np.array_equal(res[name], off[name]), name
    assert fc.same_bits(res[f"{kind}/nan"], off[f"{kind}/nan"])
    assert not res[f"{kind}/far"].any()                          # no match inside the gate: sums 0, count 0
    assert (res[f"{kind}/20000"][:, 28] > 2_000).all()


def _fixture_clouds(capi, ctx):
    target, normals, scan = fc.clouds()
    tg, owned = fc.targets(capi, ctx, target, normals)
    return tg, owned, scan


def test_seventy_calls_in_a_row(capi, off):
    ctx = capi.get_context(0)
    tg, owned, scan = _fixture_clouds(capi, ctx)
    sc = capi.Scan(ctx, fc.scan_of(scan, 2049))
    before = ctx.host_fold_passes()
    for variant in (1, 0):
        with ctx.pipeline(variant=variant, reuse=0):
            for k in range(35):
                out = capi.linearize(tg["plane"], sc, capi.PLANE, fc.T0, fc.MAX_DIST)
                assert np.array_equal(out, off["plane/2049"][1 - variant]), (variant, k)
    assert ctx.host_fold_passes() - before == 70
    sc.close()
    for t in owned:
        t.close()


def _ops(capi, ctx):
    """the operations of the interleaving test on `ctx`, in order: name -> a function of (targets, scan, batch)"""
    eye = np.eye(4)
    Ts = np.stack([fc.T0, eye])
    KIND = dict(fc.kinds(capi))

    def lin(kname, variant):
        def f(tg, sc, batch):
            with ctx.pipeline(variant=variant, reuse=0):
                return capi.linearize(tg[kname], sc, KIND[kname], fc.T0, fc.MAX_DIST).copy()
        return f

    def align(flag):
        def f(tg, sc, batch):
            T, it = capi.align(tg["plane"], sc, capi.PLANE, eye, 30, 1e-3, fc.MAX_DIST, flags=capi.FLAG_ICP_RR_QUIRK | flag)
            return np.concatenate([np.asarray(T, np.float64).reshape(-1), [it]])
        return f

    def align_batch(tg, sc, batch):
        Tb, itb, stb = capi.align_batch(tg["plane"], batch, capi.PLANE, Ts, 30, 1e-3, fc.MAX_DIST)
        return np.concatenate([np.asarray(Tb, np.float64).reshape(-1), np.asarray(itb, np.float64), np.asarray(stb, np.float64)])

    return [("plane split", lin("plane", 1)), ("icp split", lin("icp", 1)), ("ndt fused", lin("ndt", 0)),
            ("align, device loop", align(capi.FLAG_DEVICE_LOOP)), ("vplane split", lin("vplane", 1)), ("icp fused", lin("icp", 0)),
            ("plane fused", lin("plane", 0)), ("align_batch", align_batch), ("ndt split", lin("ndt", 1)),
            ("align, host loop", align(capi.FLAG_HOST_LOOP)), ("icp split again", lin("icp", 1)),
            ("plane split again", lin("plane", 1)), ("vplane fused", lin("vplane", 0))]


def _with_objects(capi, ctx, f):
    tg, owned, scan = _fixture_clouds(capi, ctx)
    sc = capi.Scan(ctx, fc.scan_of(scan, 2049))
    batch = capi.ScanBatch(ctx, [fc.scan_of(scan, 2049), fc.scan_of(scan, 257)])
    try:
        return f(tg, sc, batch)
    finally:
        batch.close(); sc.close()
        for t in owned:
            t.close()


def test_interleaved_with_device_path_passes(capi):
    shared = capi.get_context(0)
    before = shared.host_fold_passes()
    mixed = _with_objects(capi, shared, lambda tg, sc, batch: [(name, f(tg, sc, batch)) for name, f in _ops(capi, shared)])
    # the linearize passes that are not ICP and the passes of the host-driven align (one per iteration: api.hip,
    # pcr_align_host_loop); the ICP passes, the device-resident align and align_batch stay on the device
    it = int(dict(mixed)["align, host loop"][16])
    lin = sum(1 for name, _ in mixed if name.split()[0] in HOST_KINDS)
    assert it >= 2 and lin == 7 and shared.host_fold_passes() - before == lin + it
    for k, (name, got) in enumerate(mixed):
        fresh = capi.Context(0)
        try:
            alone = _with_objects(capi, fresh, _ops(capi, fresh)[k][1])
        finally:
            fresh.close()
        assert np.array_equal(got, alone), name
