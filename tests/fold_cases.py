"""The cases tests/test_gpu_fold_bits.py and tests/test_gpu_host_fold.py share, and tools/make_golden_fold_bits.py records: the
29 sums of `linearize` on a 20 k-point street target for scans whose sizes walk the fold of the block partials
(pass_device.h: wave_fold32, ticket_fold_emit) through one lane, a partial wave, a partial block, blocks with no tile in most
of the 8 groups and a second row in one group.  Everything is seeded; the normals are the analytic ones, not estimated.

Run as a script it writes every case to the .npz it is given (the child process of the host-fold test, under PCR_HOST_FOLD=0)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
MAX_DIST = 1.0
VOXEL = 2.0
SIZES = (1, 63, 64, 65, 255, 256, 257, 2049, 20_000)


def _pose():
    """the true pose of the scans, a few centimetres off: nearly every point has a match within the gate"""
    from point_cloud_registration_amd.synthetic import make_T, T_TRUE_SO3, T_TRUE_T
    T = make_T(T_TRUE_SO3, T_TRUE_T)
    T[:3, 3] += [0.02, -0.03, 0.015]
    return T


T0 = _pose()


def clouds():
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=51)
    scan, _ = perturbed_scan(target, None, seed=52)
    order = np.random.default_rng(53).permutation(len(scan))
    return np.ascontiguousarray(target, np.float32), np.ascontiguousarray(street_normals(target), np.float32), np.ascontiguousarray(scan[order], np.float32)


def scan_of(scan, n):
    return np.ascontiguousarray(scan[:n])


def far_scan():
    """no point within the gate of anything"""
    return np.ascontiguousarray(np.random.default_rng(54).uniform(-5.0, 5.0, (300, 3)) + [0.0, 0.0, 500.0], np.float32)


def nan_scan(scan):
    s = scan_of(scan, 257).copy()
    s[100, 1] = np.nan
    return s


def kinds(capi):
    return (("icp", capi.ICP), ("plane", capi.PLANE), ("vplane", capi.VPLANE), ("ndt", capi.NDT))


def _sums(capi, ctx, tgt, sc, kind, T):
    """[split, fused]: search + reduce (variant 1) and the fused small-scan kernel (variant 0)"""
    out = []
    for variant in (1, 0):
        with ctx.pipeline(variant=variant, reuse=0):
            out.append(capi.linearize(tgt, sc, kind, T, MAX_DIST).copy())
    return np.stack(out)


def targets(capi, ctx, target, normals):
    pt = capi.Target.points(ctx, target, normals)
    vx = capi.Target.voxels(ctx, target, VOXEL, 3)
    return {"icp": pt, "plane": pt, "vplane": vx, "ndt": vx}, (pt, vx)


def run_linearize(capi, ctx, which=None):
    """{"<kind>/<n>": (2, 29)} for every kind (or those of `which`) and size, plus the scan without a match and the one
    with a NaN point"""
    target, normals, scan = clouds()
    tg, owned = targets(capi, ctx, target, normals)
    res = {}
    named = [(str(n), scan_of(scan, n)) for n in SIZES] + [("far", far_scan()), ("nan", nan_scan(scan))]
    for sname, pts in named:
        sc = capi.Scan(ctx, pts)
        for kname, kind in kinds(capi):
            if which is None or kname in which:
                res[f"{kname}/{sname}"] = _sums(capi, ctx, tg[kname], sc, kind, T0)
        sc.close()
    for t in owned:
        t.close()
    return res


def run_batch(capi, ctx):
    target, normals, scan = clouds()
    tgt = capi.Target.points(ctx, target, normals)
    batch = capi.ScanBatch(ctx, [scan_of(scan, 2049), scan_of(scan, 257), scan_of(scan, 65)])
    T1 = np.eye(4)
    Ts = np.stack([T0, T1, T0])
    out = np.asarray(capi.linearize_batch(tgt, batch, capi.PLANE, Ts, MAX_DIST)).copy()
    batch.close(); tgt.close()
    return out


def run_gicp(capi, ctx):
    target, normals, scan = clouds()
    t = capi.Target.points(ctx, target)
    t.estimate_covariances(10, capi.COV_PLANE, 1e-3, want=False)
    s = capi.Scan(ctx, scan_of(scan, 2049), flags=capi.FLAG_KEEP_ORDER)
    s.estimate_covariances(10, capi.COV_PLANE, 1e-3, want=False)
    out = np.asarray(capi.gicp_linearize(t, s, T0, MAX_DIST)).copy()
    s.close(); t.close()
    return out


def run_all(capi, ctx):
    res = run_linearize(capi, ctx)
    res["batch/plane"] = run_batch(capi, ctx)
    res["gicp/2049"] = run_gicp(capi, ctx)
    return res


def same_bits(a, b):
    """== on every value, NaNs in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


if __name__ == "__main__":
    from point_cloud_registration_amd import _capi
    c =_capi.get_context(0)
    out = run_all(_capi, c)
    out["host_fold_passes"] = np.array(c.host_fold_passes())
    np.savez(sys.argv[1], **out)
