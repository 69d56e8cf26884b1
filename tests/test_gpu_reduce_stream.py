"""The streaming loop of the reduce kernels (csrc/pass_device.h: reduce_stream), point targets: a lane loads the index and
the coordinates of W scan points, then their W matched records, then accumulates them in index order.  A slot past the end
of the lane's range and a slot without a match load a stand-in and are skipped.  What can go wrong there is the pairing of
index, coordinates and record across the W slots and the predication of the slots, so every case forces the search +
reduce pipeline (variant 1: small scans run k_nn_scan + k_reduce_finalize too) and compares ``linearize`` with the oracle
at the suite's bar (TOL_ORC, count exact), ICP and PlaneICP.

Which slots are live.  The reduce grid has min(ceil(n / 256), 1024) blocks (rounded to a multiple of 8), and a block's tiles
are those of its XCD's span dealt round-robin over the XCD's blocks.  A scan under 262 144 points therefore gives every
block ONE tile: only slot 0 is live, slots 1 .. W - 1 are past the end.  The small scans below test exactly that (and the
edges of the scan); everything about slots u >= 1 is tested on scans of 1.4 M points and more, where a lane owns tiles
b, b + 128, b + 256, ... of its span -- 5.3 of them at 1.4 M: slots 0 .. 4 of the first trip and slot 0 (or 0 and 1) of a second.
In the caller's order (FLAG_NO_SCAN_SORT) slot u of a lane is point (tile b + 128 u) * 256 + lane of the span.

Run on the GPU box:  python -m pytest tests/test_gpu_reduce_stream.py -m gpu -q
"""

import numpy as np
import pytest

from conftest import rel_H

pytestmark = pytest.mark.gpu

TOL_ORC = 1e-10
MAX_DIST = 1.0
W = 5                                            # PCR_RED_W of the shipped build: scan points per lane and trip
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2049, 8 * 256 * W + 1]
KINDS = ["icp", "plane"]
N_BIG = 1_400_000                                # more than 2 x 262 144: slots 0 .. 4 of a lane live, a second trip
OFF = 100.0                                      # metres along y: the street spans |y| <= 30, so at least 40 m off the cloud


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


@pytest.fixture
def split(ctx):
    """search + reduce whatever the size of the scan; the shipped selection is restored afterwards"""
    before = ctx.get_pipeline()
    with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=0, reuse=0):
        yield
    assert ctx.get_pipeline() == before


def kind_of(capi, name):
    return {"icp": capi.ICP, "plane": capi.PLANE}[name]


@pytest.fixture(scope="module")
def street20k(capi, orc, ctx):
    """20 k-point street target with analytic normals (GPU + oracle) and one 12 k-point perturbed scan the cases cut from"""
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=3)
    normals = street_normals(target)
    scan, T_true = perturbed_scan(target, 12_000, seed=4)
    T = T_true.copy()
    T[:3, 3] += [0.01, -0.02, 0.015]
    return {"target": target, "normals": normals, "scan": scan, "T": T,
            "gt": capi.Target.points(ctx, target, normals), "ot": orc.TargetPoints(target, normals=normals)}


def check(capi, orc, gt, ot, name, T, src, flags=0, max_dist=MAX_DIST, tol=TOL_ORC):
    """linearize against the oracle: count exact, H / g / e2 at `tol` (g cancels: 100 x, e2: 10 x, as test_gpu_parity.py)"""
    sc = capi.Scan(gt.ctx, src, flags=flags)
    out = capi.linearize(gt, sc, kind_of(capi, name), T, max_dist)
    H, g, e2, cnt = capi.unpack29(out)
    Ho, go, e2o, cnto = orc.calc_H_g_e2(kind_of(capi, name), ot, T, src, max_dist, with_count=True)
    print(f"{name} n={len(src)} count {cnt}/{cnto}", end=" ")
    assert cnt == cnto
    if cnto == 0:
        assert not np.any(out), out
        return out, cnt
    print(f"rel_H {rel_H(H, Ho):.3e} rel_g {rel_H(g, go):.3e} e2 {abs(e2 - e2o) / max(abs(e2o), 1e-30):.3e}")
    assert rel_H(H, Ho) < tol, (name, rel_H(H, Ho))
    assert rel_H(g, go) < tol * 100, (name, rel_H(g, go))
    assert abs(e2 - e2o) <= tol * max(abs(e2o), 1e-30) * 10
    return out, cnt


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_edges_of_the_predication(capi, orc, street20k, split, name, n):
    """Scans of 1 point up to one point more than 8 x 256 x W: one tile per block, so slot 0 is live and slots 1 .. W - 1
    are past the end in every lane; lanes past the end in slot 0 too, XCD spans that are empty, a partial last tile."""
    s = street20k
    _, cnt = check(capi, orc, s["gt"], s["ot"], name, s["T"], s["scan"][:n])
    assert cnt > 0.9 * n


@pytest.fixture(scope="module")
def big_scans(street20k):
    """perturbed copies of the target's points with repetition, in random order: 1.4 M (two trips per lane on the
    1024-block grid, the second partial) and 2.7 M points (three trips)"""
    rng = np.random.default_rng(11)
    T = street20k["T"]
    Rinv = T[:3, :3].T
    tinv = -Rinv @ T[:3, 3]
    out = {}
    for n in (N_BIG, 2_700_000):
        p = street20k["target"][rng.integers(0, len(street20k["target"]), n)].astype(np.float64)
        p = p @ Rinv.T + tinv + rng.normal(0.0, 0.01, (n, 3))
        out[n] = np.ascontiguousarray(p, dtype=np.float32)
    return out


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("n", [N_BIG, 2_700_000])
def test_more_than_one_trip(capi, orc, street20k, big_scans, split, name, n):
    s = street20k
    _, cnt = check(capi, orc, s["gt"], s["ot"], name, s["T"], big_scans[n])
    assert cnt > 0.9 * n


def thirds_off(src):
    """every third point moved off the cloud.  In the caller's order the slots of a lane are 128 * 256 points apart,
    = 2 mod 3: the points of slots u, u + 1, u + 2 of one lane fall in three different classes mod 3, so `no match`
    sits on different slots of the same lane, and on every slot in some lane"""
    out = src.copy()
    out[::3, 1] += OFF
    return out


@pytest.mark.parametrize("name", KINDS)
def test_unmatched_points_inside_a_group(capi, orc, street20k, big_scans, split, name):
    """1.4 M points, every third without a match: slots 0 .. 4 live, `no match` mixed among them (see thirds_off)."""
    s = street20k
    src = thirds_off(big_scans[N_BIG])
    _, cnt = check(capi, orc, s["gt"], s["ot"], name, s["T"], src, flags=capi.FLAG_NO_SCAN_SORT)
    assert 0 < cnt <= len(src) - len(src[::3])
    check(capi, orc, s["gt"], s["ot"], name, s["T"], src)                 # ... and Morton-sorted
    # (one tile per block: the same in slot 0 alone)
    check(capi, orc, s["gt"], s["ot"], name, s["T"], thirds_off(s["scan"][:11_777]), flags=capi.FLAG_NO_SCAN_SORT)


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("n", [3_001, N_BIG])
def test_nothing_matched(capi, orc, street20k, big_scans, split, name, n):
    """Every point without a match: count 0 and every sum exactly 0 (the stand-in records are never accumulated), with
    slot 0 alone and with every slot live."""
    s = street20k
    src = big_scans[N_BIG][:n].copy()
    src[:, 1] += OFF
    out, cnt = check(capi, orc, s["gt"], s["ot"], name, s["T"], src, flags=capi.FLAG_NO_SCAN_SORT)
    assert cnt == 0 and not np.any(out)


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("n", [5 * 256 + 77, N_BIG])
def test_only_the_last_tile_matched(capi, orc, street20k, big_scans, split, name, n):
    """The caller's order, the last tile partial, only its points matched: 6 tiles (slot 0 of one block), and 5469 tiles,
    where the last one is slot 5 = the second trip's slot 0 of its lane, behind a first trip of five unmatched slots."""
    s = street20k
    last = n % 256
    assert last > 0
    src = big_scans[N_BIG][:n].copy()
    src[:n - last, 1] += OFF
    _, cnt = check(capi, orc, s["gt"], s["ot"], name, s["T"], src, flags=capi.FLAG_NO_SCAN_SORT)
    assert 0 < cnt <= last


def lattice():
    """65 x 65 x 5 lattice of spacing 1/4 (|x|, |y| <= 8: mapped onto itself by a quarter turn about z), axis-aligned unit
    normals that change from point to point, and the scan: the same points shifted by (1/16, 0, 1/32)"""
    a = np.arange(-32, 33) / 4.0
    zz = np.arange(5) / 4.0
    pts = np.stack(np.meshgrid(a, a, zz, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(5)
    pts = pts[rng.permutation(len(pts))]
    axis = rng.integers(0, 3, len(pts))
    normals = np.zeros_like(pts)
    normals[np.arange(len(pts)), axis] = np.where(rng.integers(0, 2, len(pts)) == 1, 1.0, -1.0)
    scan = pts + np.array([1 / 16, 0.0, 1 / 32], np.float32)
    return pts, normals, scan


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("pose", ["identity", "quarter_turn"])
def test_exact_arithmetic(capi, orc, ctx, split, name, pose):
    """Coordinates, offsets, normals and the rotation are small dyadic numbers: every product and every partial sum of
    the 29 is exactly representable (sums below 2^38 in units of 2^-10), so the order of the sums cannot show and the
    GPU's numbers equal the oracle's BIT FOR BIT.  The lattice scan is repeated 67 times to 1.4 M points: slots 0 .. 4 of
    a lane are live and, in the caller's order, 32 768 points = 11 643 lattice points apart, so a record, a coordinate or
    an index taken from another slot has no tolerance to hide behind.  Also with every third point far off the lattice
    (by 64: still exact), and once at lattice size (slot 0 alone)."""
    pts, normals, scan = lattice()
    gt = capi.Target.points(ctx, pts)
    gt.set_normals(normals)
    ot = orc.TargetPoints(pts, normals=normals)
    T = np.eye(4)
    if pose == "quarter_turn":
        T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    big = np.tile(scan, (67, 1))
    assert len(big) > N_BIG
    holes = big.copy()
    holes[::3, 1] += 64.0
    for tag, src, every in (("lattice", scan, True), ("x67", big, True), ("x67 thirds off", holes, False)):
        Ho, go, e2o, cnto = orc.calc_H_g_e2(kind_of(capi, name), ot, T, src, MAX_DIST, with_count=True)
        assert cnto == (len(src) if every else len(src) - len(src[::3]))
        for flags in (0, capi.FLAG_NO_SCAN_SORT):
            out = capi.linearize(gt, capi.Scan(ctx, src, flags=flags), kind_of(capi, name), T, MAX_DIST)
            H, g, e2, cnt = capi.unpack29(out)
            print(f"{name} {pose} {tag} flags {flags} count {cnt}/{cnto} max|dH| {np.max(np.abs(H - Ho))} "
                  f"max|dg| {np.max(np.abs(g - go))} de2 {e2 - e2o}")
            assert cnt == cnto
            assert np.array_equal(H, Ho) and np.array_equal(g, go) and e2 == e2o


@pytest.fixture(scope="module")
def f64_target(capi, orc, ctx, street20k):
    s = street20k
    rng = np.random.default_rng(7)
    t64 = s["target"].astype(np.float64) + rng.normal(0.0, 1e-5, s["target"].shape)
    gt = capi.Target.points(ctx, t64.astype(np.float32), s["normals"])
    assert gt.set_points_f64(t64)
    return gt, orc.TargetPoints(t64, normals=s["normals"], tree_f64=True)


@pytest.mark.parametrize("n", [257, 2049, 8 * 256 * W + 1])
def test_float64_plane_target(capi, orc, street20k, f64_target, split, n):
    """Quirk Q6: a float64 PlaneICP target runs k_reduce_finalize<PLANE, FIX> -- the float64 search of the pending points
    in front of the same loop.  One tile per block: slot 0."""
    s = street20k
    _, cnt = check(capi, orc, f64_target[0], f64_target[1], "plane", s["T"], s["scan"][:n])
    assert cnt > 0.9 * n


@pytest.mark.parametrize("holes", [False, True])
def test_float64_plane_target_every_slot(capi, orc, street20k, big_scans, f64_target, split, holes):
    """... and at 1.4 M points: that instantiation takes W = 4, so a lane runs slots 0 .. 3 and a second trip of two;
    all matched, and with every third point unmatched in the caller's order."""
    s = street20k
    src = thirds_off(big_scans[N_BIG]) if holes else big_scans[N_BIG]
    _, cnt = check(capi, orc, f64_target[0], f64_target[1], "plane", s["T"], src, flags=capi.FLAG_NO_SCAN_SORT if holes else 0)
    assert cnt > 0.6 * len(src)
