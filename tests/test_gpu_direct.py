"""VGICP's direct voxel neighbourhoods on the GPU: the containing-voxel lookup, the sums of one pass over 1 / 7 / 27 voxels per
point, the robust pass, residuals, the per-point loop of the class, align, and what the pass must leave undisturbed.

Fixture: g2_mini_street -- voxel size 1.0, 218 kept voxels, 2000 scan points at a non-identity pose.  tests/test_direct_cases.py
pins the restated pair counts (gates 0.8 and 2.0) and that no pair distance lies within 5e-6 relative of either gate, so masks,
indices and counts compare exactly.  The sums are restated (tests/direct_cases.py) from the GPU's own read-back keys, centroids
and covariances -- what the pass used.

Bounds:
  lookup      exact
  sums        per entry gicp_cases.sum_bound over the kept PAIRS: (pairs + 16 / eps_min) 2^-53 sum |term| against math.fsum of
              the restated terms; conftest.step_err <= 1e-10; robust: 1.5 x that bound (robust_cases.reference)
  residuals   (16 / eps_min + 16) 2^-53 |d|^T |M| |d|, the bound of VGICP's residuals
  align       the class's own loop of calc_H_g_e2 + solve + plus: the same iteration count, max|dT| <= 1e-10"""

import numpy as np
import pytest

import direct_cases as dn
import gicp_cases as gc
import robust_cases as rc
import vgicp_cases as vc
from conftest import step_err

pytestmark = pytest.mark.gpu

EPS = 1e-3
NAMES = ("raw", "plane", "spd")
NEIGHBORS = (1, 7, 27)
GATES = (0.8, 2.0)
PREFIXES = (0, 1, 63, 64, 65, 257, 2000)
PAIRS = {0.8: {1: 1596, 7: 4607, 27: 5931}, 2.0: {1: 1625, 7: 9699, 27: 27504}}      # tests/test_direct_cases.py


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


def voxel_target(capi, ctx, g2, voxel_size=None, min_points=10):
    return capi.Target.voxels(ctx, g2["target"], float(g2["voxel_size"]) if voxel_size is None else voxel_size, min_points)


@pytest.fixture(scope="module")
def tp(g2):
    out = vc.xform32(g2["T"], g2["source"])
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def sides(capi, ctx, g2):
    """name -> (Cp float32 (N, 6), target with its voxel covariances set, Cv, centroids, keys read back), as the ``sides`` of
    tests/test_gpu_vgicp.py build them: raw / plane voxel covariances under the scan's estimated PLANE ones, random SPD
    matrices with condition <= 100 from default_rng(0) on both sides.  Computed once, never modified."""
    src = g2["source"]
    rng = np.random.default_rng(0)
    cp_plane = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER).estimate_covariances(10, capi.COV_PLANE, EPS)
    cp_spd = gc.random_spd(len(src), rng)
    cv_spd = gc.random_spd(218, rng).astype(np.float64)
    out = {}
    for name in NAMES:
        t = voxel_target(capi, ctx, g2)
        if name == "raw":
            t.set_voxel_covariances(capi.COV_RAW)
        elif name == "plane":
            t.set_voxel_covariances(capi.COV_PLANE, EPS)
        else:
            t.set_voxel_covariances(cov=cv_spd)
        cp = cp_spd if name == "spd" else cp_plane
        st = t.voxel_stats(("mean", "keys"))
        cv, mean, keys = t.get_voxel_covariances(), st["mean"], st["keys"]
        for a in (cp, cv, mean, keys):
            a.setflags(write=False)
        out[name] = (cp, t, cv, mean, keys)
    return out


@pytest.fixture(scope="module")
def restated(g2, sides, tp):
    """(name, neighbors, gate) -> (terms (pairs, 28) in the order they are added, eps_min, mask (N, neighbors)), computed on
    first use and shared."""
    cache = {}

    def get(name, nb, gate):
        if (name, nb, gate) not in cache:
            cp, _, cv, mean, keys = sides[name]
            idx = dn.lookup(tp, float(g2["voxel_size"]), keys, nb)
            t, eps_min, mask = dn.terms(g2["T"], g2["source"], tp, mean, cp, cv, idx, gate)
            assert len(t) == int(mask.sum()) == PAIRS[gate][nb]
            t.setflags(write=False)
            cache[(name, nb, gate)] = (t, eps_min, mask)
        return cache[(name, nb, gate)]
    return get


def reference(restated, name, nb, gate, n=None):
    """(fsum per column, bound per column, pairs) over the pairs of the first n scan points."""
    t, eps_min, mask = restated(name, nb, gate)
    pairs = int(mask[:n].sum()) if n is not None else len(t)
    ref, mag = gc.fsum_cols(t[:pairs])                      # (pairs are ordered by scan point)
    return ref, gc.sum_bound(pairs, eps_min, mag), pairs


def scan_of(capi, ctx, g2, cp, n=None, flags=None):
    n = len(cp) if n is None else n
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    s.set_covariances(np.ascontiguousarray(cp[:n]))
    return s


# ----------------------------------------------------------------------------- 1. lookup
@pytest.mark.parametrize("nb", NEIGHBORS)
def test_lookup(capi, ctx, g2, sides, tp, nb):
    _, t, _, mean, keys = sides["plane"]
    want = dn.lookup(tp, 1.0, keys, nb)
    assert int((want >= 0).sum()) == {1: 1625, 7: 9699, 27: 29475}[nb]
    for n in PREFIXES:
        got = t.lookup(tp[:n], nb)
        assert got.dtype == np.int64 and got.shape == (n, nb) and np.array_equal(got, want[:n]), n
    # the target's own points find the voxel whose key is theirs, iff it is kept
    from point_cloud_registration_amd.voxel import get_keys
    tk = get_keys(g2["target"], 1.0)
    own = t.lookup(g2["target"], nb)[:, 13 if nb == 27 else 0]
    kept = np.isin(tk, keys)
    assert int(kept.sum()) == 4786 and np.array_equal(own >= 0, kept) and np.array_equal(keys[own[kept]], tk[kept])
    # outside the box, far outside, not a number
    lo, hi = g2["target"].min(axis=0), g2["target"].max(axis=0)
    q = np.array([hi + 10.0, lo - 10.0, [1e30, 0, 0], [0, -1e30, 0], [0, 0, 1e30], [-1e30, -1e30, -1e30], [np.nan, 0, 0],
                  [0, np.nan, 0], [0, 0, np.inf], [3e12, 0, 0]], np.float32)
    assert np.all(t.lookup(q, nb) == -1) and np.all(dn.lookup(q, 1.0, keys, nb) == -1)
    assert t.lookup(np.zeros((0, 3), np.float32), nb).shape == (0, nb)


@pytest.mark.parametrize("voxel_size", [0.3, 0.5])
def test_lookup_other_voxel_sizes(capi, ctx, g2, tp, voxel_size):
    """The restatement divides in float64 as the lookup does, so a voxel size that is no power of two compares exactly too.
    Voxels of 3 points and more are kept: 651 at 0.3 and 824 at 0.5, where 10 points keep 1 and 67."""
    t = voxel_target(capi, ctx, g2, voxel_size, min_points=3)
    keys = t.voxel_stats(("keys",))["keys"]
    assert len(keys) == {0.3: 651, 0.5: 824}[voxel_size] and np.all(np.diff(keys) > 0)
    for nb in NEIGHBORS:
        want = dn.lookup(tp, voxel_size, keys, nb)
        assert int((want >= 0).sum()) > 500 and np.array_equal(t.lookup(tp, nb), want), nb
    # the class's grid returns rows of its ``mean``
    from point_cloud_registration_amd.voxel import VoxelGrid
    grid = VoxelGrid(voxel_size, min_points=3)
    grid.set_points(g2["target"])
    assert np.array_equal(grid.lookup(tp, 7), dn.lookup(tp, voxel_size, keys, 7))
    assert np.array_equal(grid.lookup(tp.astype(np.float64), 1), dn.lookup(tp, voxel_size, keys, 1))      # cast to float32


# ----------------------------------------------------------------------------- 2. sums
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("nb", NEIGHBORS)
@pytest.mark.parametrize("name", NAMES)
def test_sums(capi, ctx, g2, sides, restated, name, nb, gate):
    cp, t = sides[name][:2]
    s = scan_of(capi, ctx, g2, cp)
    out = capi.vgicp_direct_linearize(t, s, g2["T"], gate, nb)
    ref, bound, pairs = reference(restated, name, nb, gate)
    assert pairs == PAIRS[gate][nb] and out[28] == pairs
    err = np.abs(out[:28] - ref)
    H, g, _ = gc.unpack28(out[:28])
    Href, gref, _ = gc.unpack28(ref)
    se = step_err(H, g, Href, gref)
    print(f"{name} x{nb} gate {gate}: pairs {pairs}, eps_min {restated(name, nb, gate)[1]:.3e}, max err / bound "
          f"{np.max(err / bound):.3e}, step_err {se:.3e}")
    assert np.all(err <= bound)
    assert se <= 1e-10
    # two calls return the same bits
    assert np.array_equal(out, capi.vgicp_direct_linearize(t, s, g2["T"], gate, nb))
    # rb = PCR_ROBUST_NONE is the plain pass
    assert np.array_equal(out, capi.vgicp_direct_linearize(t, s, g2["T"], gate, nb, robust=(capi.ROBUST_NONE, 1.0)))
    # no bit of the caller's flags word reaches the kernels
    assert np.array_equal(out, capi.vgicp_direct_linearize(t, s, g2["T"], gate, nb, flags=0xFFFFFFFF))
    # the scan in the caller's order on the device
    nosort = capi.vgicp_direct_linearize(t, scan_of(capi, ctx, g2, cp, flags=capi.FLAG_NO_SCAN_SORT), g2["T"], gate, nb)
    assert nosort[28] == pairs and np.all(np.abs(nosort[:28] - ref) <= bound) and np.all(np.abs(nosort[:28] - out[:28]) <= bound)


@pytest.mark.parametrize("n", PREFIXES)
def test_sums_prefixes(capi, ctx, g2, sides, restated, n):
    """The pairs of a prefix of the scan are the pairs of its points."""
    for name, nb, gate in (("plane", 1, 0.8), ("raw", 7, 2.0), ("spd", 27, 0.8), ("plane", 27, 2.0)):
        cp, t = sides[name][:2]
        out = capi.vgicp_direct_linearize(t, scan_of(capi, ctx, g2, cp, n=n), g2["T"], gate, nb)
        ref, bound, pairs = reference(restated, name, nb, gate, n)
        assert out[28] == pairs
        assert np.all(np.abs(out[:28] - ref) <= bound)
        if n == 0:
            assert np.array_equal(out, np.zeros(29))


# ----------------------------------------------------------------------------- 3. robust
@pytest.fixture(scope="module")
def robust_case(g2, sides, tp):
    """The kept pairs of 7 neighbours at gate 2.0 in the order they are added: (scan rows, voxels)."""
    _, _, _, mean, keys = sides["plane"]
    idx = dn.lookup(tp, 1.0, keys, 7)
    rows, vox, _ = dn.pairs(tp, mean, idx, 2.0)
    return rows, vox


@pytest.mark.parametrize("kind", ["cauchy", "tukey"])
def test_robust(capi, ctx, g2, sides, tp, robust_case, kind):
    cp, t, cv, mean, _ = sides["plane"]
    rows, vox = robust_case
    src = g2["source"]
    ones = np.ones(len(rows), bool)
    _, plain, s, _, eps_min = rc.terms_dist(None, 1.0, g2["T"], src[rows], tp[rows], mean[vox], cp[rows], cv[vox], ones, "f64")
    c = rc.median_scale(s)
    tw = rc.terms_dist(kind, c, g2["T"], src[rows], tp[rows], mean[vox], cp[rows], cv[vox], ones, "f64")[0]
    ref, bound = rc.reference(tw, plain, lambda mag: gc.sum_bound(len(rows), eps_min, mag))
    sc = scan_of(capi, ctx, g2, cp)
    out = capi.vgicp_direct_linearize(t, sc, g2["T"], 2.0, 7, robust=capi.check_robust(kind, c))
    err = np.abs(out[:28] - ref)
    print(f"{kind} c {c:.3e}: pairs {len(rows)}, max err / bound {np.max(err / bound):.3e}")
    assert out[28] == len(rows) == 9699
    assert np.all(err <= bound)
    assert np.array_equal(out, capi.vgicp_direct_linearize(t, sc, g2["T"], 2.0, 7, robust=capi.check_robust(kind, c)))
    plain_out = capi.vgicp_direct_linearize(t, sc, g2["T"], 2.0, 7)
    assert not np.array_equal(out[:28], plain_out[:28])
    # the class hands its kernel to the same entry point
    import point_cloud_registration_amd as pcr
    reg = pcr.VGICP(voxel_size=1.0, max_dist=2.0, eps=EPS, neighbors=7, robust=kind, robust_scale=c)
    reg.set_target(g2["target"])
    H, g, e2 = reg.calc_H_g_e2(g2["T"], g2["source"], source_cov=cp)
    assert np.array_equal(np.concatenate([H[gc.TRIU], g, [e2]]), out[:28]) and reg.last_correspondences == 9699


def test_huber_above_every_residual_is_the_plain_pass(capi, ctx, g2, sides):
    cp, t = sides["plane"][:2]
    sc = scan_of(capi, ctx, g2, cp)
    for nb in NEIGHBORS:
        res = capi.vgicp_direct_residuals(t, sc, g2["T"], 2.0, nb)
        c = 2.0 * float(np.sqrt(res[np.isfinite(res)].max()))
        plain = capi.vgicp_direct_linearize(t, sc, g2["T"], 2.0, nb)
        assert np.array_equal(plain, capi.vgicp_direct_linearize(t, sc, g2["T"], 2.0, nb, robust=capi.check_robust("huber", c)))


# ----------------------------------------------------------------------------- 4. residuals
@pytest.mark.parametrize("nb", NEIGHBORS)
def test_residuals(capi, ctx, g2, sides, tp, restated, nb):
    cp, t, cv, mean, keys = sides["plane"]
    idx = dn.lookup(tp, 1.0, keys, nb)
    for gate in GATES:
        want, mag, eps_min = dn.pair_residuals(g2["T"], tp, mean, cp, cv, idx, gate)
        got = capi.vgicp_direct_residuals(t, scan_of(capi, ctx, g2, cp), g2["T"], gate, nb)
        assert got.shape == (2000, nb) and got.dtype == np.float64
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isfinite(got), restated("plane", nb, gate)[2])
        fin = np.isfinite(want)
        bound = (16.0 / eps_min + 16.0) * gc.EPS53 * mag[fin]
        print(f"x{nb} gate {gate}: max err / bound {np.max(np.abs(got[fin] - want[fin]) / bound):.3e}")
        assert np.all(np.abs(got[fin] - want[fin]) <= bound)
        # a permuted upload: every row arrives where the caller put its point
        perm = np.random.default_rng(3).permutation(2000)
        s2 = capi.Scan(ctx, np.ascontiguousarray(g2["source"][perm]), flags=capi.FLAG_KEEP_ORDER)
        s2.set_covariances(np.ascontiguousarray(cp[perm]))
        assert np.array_equal(capi.vgicp_direct_residuals(t, s2, g2["T"], gate, nb), got[perm])
    # the class: (N, neighbors), the same bits
    import point_cloud_registration_amd as pcr
    reg = pcr.VGICP(voxel_size=1.0, max_dist=2.0, eps=EPS, neighbors=nb)
    reg.set_target(g2["target"])
    assert np.array_equal(reg.residuals(g2["T"], g2["source"], source_cov=cp), got)


# ----------------------------------------------------------------------------- 5. the per-point loop of the class
def test_no_parallel_ver(g2, sides, restated):
    import point_cloud_registration_amd as pcr
    cp, _, cv, _, _ = sides["plane"]
    reg = pcr.VGICP(voxel_size=1.0, max_dist=0.8, eps=EPS, neighbors=7)
    reg.set_target(g2["target"])
    assert np.array_equal(reg.covariance, cv)
    ref, bound, pairs = reference(restated, "plane", 7, 0.8)
    H, g, e2 = reg.calc_H_g_e2_no_parallel_ver(g2["T"], g2["source"], source_cov=cp)
    assert np.all(np.abs(np.concatenate([H[gc.TRIU], g, [e2]]) - ref) <= bound)
    Hk, gk, e2k = reg.calc_H_g_e2(g2["T"], g2["source"], source_cov=cp)
    assert reg.last_correspondences == pairs == 4607
    assert np.all(np.abs(np.concatenate([Hk[gc.TRIU], gk, [e2k]]) - ref) <= bound)
    assert np.all(np.abs(np.concatenate([(H - Hk)[gc.TRIU], g - gk, [e2 - e2k]])) <= bound)
    keep, idx, res = reg._match(vc.xform32(g2["T"], g2["source"]))
    assert len(keep) == pairs and np.all(np.diff(keep) >= 0) and len(np.unique(keep)) == 1765


# ----------------------------------------------------------------------------- 6. align
@pytest.fixture(scope="module")
def case():
    target, scan, T_true = gc.align_case()
    for a in (target, scan, T_true):
        a.setflags(write=False)
    return target, scan, T_true


@pytest.mark.parametrize("max_dist", [2.0, 0.6])
@pytest.mark.parametrize("nb", NEIGHBORS)
def test_align(capi, case, nb, max_dist):
    """A NumPy prototype of the definition reaches, from |dR|_F 3.81e-2 / |dt| 0.1136 m: one voxel 5.3e-3 / 4.9e-2 (gate 2.0) and
    4.6e-3 / 5.6e-2 (0.6); seven 2.9e-3 / 2.4e-2 and 4.0e-3 / 8.1e-3; twenty-seven 3.0e-3 / 4.5e-3 and 3.9e-3 / 6.9e-3.  One
    voxel per point reaches 0.0558 m against half the start, 0.0568 m, at gate 0.6: it gets the weaker bound only."""
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.math_tools import plus
    target, scan, T_true = case
    reg = pcr.VGICP(voxel_size=1.0, max_dist=max_dist, k=10, neighbors=nb)
    reg.set_target(target)
    assert len(reg.voxels.mean) == 200
    T = reg.align(scan)
    iters = reg.last_iterations
    dR, dt = np.linalg.norm(T[:3, :3] - T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])
    dR0, dt0 = np.linalg.norm(np.eye(3) - T_true[:3, :3]), np.linalg.norm(T_true[:3, 3])
    print(f"x{nb} max_dist {max_dist}: {iters} iterations, pairs {reg.last_correspondences}, |dR|_F {dR:.3e} (start {dR0:.3e}), "
          f"|dt| {dt:.3e} (start {dt0:.3e})")
    assert dR < dR0 and dt < dt0
    if nb > 1:
        assert dR < 0.5 * dR0 and dt < 0.5 * dt0
    # the same loop in the test: calc_H_g_e2 + solve + plus
    cur, it = np.eye(4), 0
    for it in range(reg.max_iter):
        H, g, _ = reg.calc_H_g_e2(cur, scan)
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < reg.tol:
            break
        cur = plus(cur, dx)
    assert iters == it + 1
    assert np.max(np.abs(T - cur)) <= 1e-10
    # every trace row's sums are the bits pcr_vgicp_direct_linearize returns at that row's pose
    dev = reg._gicp_scan(scan, None)
    T2, iters2, trace = capi.vgicp_direct_align(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, max_dist, nb, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(capi.vgicp_direct_linearize(reg._target, dev, row[:16], max_dist, nb), row[16:])


# ----------------------------------------------------------------------------- 7. isolation
def test_nearest_centroid_pass_is_undisturbed(capi, ctx, g2, sides):
    """VGICP() returns the same bits before and after direct passes on the same handles."""
    cp = sides["plane"][0]
    t = voxel_target(capi, ctx, g2)
    t.set_voxel_covariances(capi.COV_PLANE, EPS)
    s = scan_of(capi, ctx, g2, cp)
    T, md = g2["T"], float(g2["max_dist"])
    before = capi.vgicp_linearize(t, s, T, md)
    res_before = capi.vgicp_residuals(t, s, T, md)
    for nb in NEIGHBORS:
        capi.vgicp_direct_linearize(t, s, T, md, nb)
        capi.vgicp_direct_residuals(t, s, T, md, nb)
        t.lookup(g2["source"], nb)
        capi.vgicp_direct_align(t, s, T, 3, 1e-3, md, nb)
    assert np.array_equal(before, capi.vgicp_linearize(t, s, T, md)) and before[28] == 1785
    assert np.array_equal(res_before, capi.vgicp_residuals(t, s, T, md))
    # the class with neighbors=None makes the calls it made
    import point_cloud_registration_amd as pcr
    reg = pcr.VGICP(voxel_size=1.0, max_dist=md, eps=EPS)
    reg.set_target(g2["target"])
    H, g, e2 = reg.calc_H_g_e2(T, g2["source"], source_cov=cp)
    assert np.array_equal(np.concatenate([H[gc.TRIU], g, [e2]]), before[:28]) and reg.last_correspondences == 1785


def test_set_covariance_between_two_passes(capi, ctx, g2, sides, restated):
    """The lookup data outlive a change of the voxel covariances, and the pass reads the new ones."""
    cp, _, cv_spd, _, _ = sides["spd"]
    t = voxel_target(capi, ctx, g2)
    t.set_voxel_covariances(capi.COV_RAW)
    s = scan_of(capi, ctx, g2, cp)
    first = capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 27)
    t.set_voxel_covariances(cov=cv_spd)
    second = capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 27)
    ref, bound, pairs = reference(restated, "spd", 27, 0.8)
    assert first[28] == second[28] == pairs and not np.array_equal(first[:28], second[:28])
    assert np.all(np.abs(second[:28] - ref) <= bound)
    assert np.array_equal(second, capi.vgicp_direct_linearize(sides["spd"][1], s, g2["T"], 0.8, 27))


# ----------------------------------------------------------------------------- 8. refusals and empties
def test_refusals_write_nothing(capi, ctx, g2, sides):
    cp, t = sides["plane"][:2]
    s = scan_of(capi, ctx, g2, cp)
    bare = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER)
    T = np.ascontiguousarray(g2["T"], dtype=np.float64).reshape(16)
    L = capi.lib()
    other = capi.Context(0)
    try:
        foreign = scan_of(capi, other, g2, cp)
        points = capi.Target.points(ctx, g2["target"])
        nocov = voxel_target(capi, ctx, g2)
        bad_kind, keep1 = capi._rb((9, 1.0))
        bad_scale, keep2 = capi._rb((capi.ROBUST_HUBER, 0.0))
        # (target, scan, max_dist, neighbors, rb) -> status; the first reason in the order of include/pcr.h wins
        cases = [((t, s, 0.8, 5, None), capi.PCR_ERR_INVALID), ((t, s, 0.8, 0, bad_kind), capi.PCR_ERR_INVALID),
                 ((points, s, 0.8, 26, None), capi.PCR_ERR_INVALID),
                 ((t, s, 0.8, 7, bad_kind), capi.PCR_ERR_INVALID), ((t, s, 0.8, 7, bad_scale), capi.PCR_ERR_INVALID),
                 ((points, bare, -1.0, 7, bad_kind), capi.PCR_ERR_INVALID),
                 ((points, s, 0.8, 7, None), capi.PCR_ERR_NO_TARGET), ((nocov, s, 0.8, 7, None), capi.PCR_ERR_NO_TARGET),
                 ((t, bare, 0.8, 7, None), capi.PCR_ERR_NO_TARGET), ((points, foreign, -1.0, 7, None), capi.PCR_ERR_NO_TARGET),
                 ((t, foreign, 0.8, 7, None), capi.PCR_ERR_INVALID), ((t, foreign, -1.0, 7, None), capi.PCR_ERR_INVALID),
                 ((t, s, 0.0, 7, None), capi.PCR_ERR_INVALID), ((t, s, -1.0, 27, None), capi.PCR_ERR_INVALID),
                 ((t, s, float("nan"), 1, None), capi.PCR_ERR_INVALID)]
        for (tt, ss, md, nb, rb), status in cases:
            out, Tout, res = np.full(29, 7.0), np.full(16, 7.0), np.full((2000, 27), 7.0)
            iters = capi.C.c_int(-5)
            assert L.pcr_vgicp_direct_linearize(tt.handle, ss.handle, T, md, nb, rb, 0, out) == status, (md, nb, status)
            assert L.pcr_vgicp_direct_align(tt.handle, ss.handle, T, 5, 1e-3, md, nb, rb, 0, Tout, capi.C.byref(iters), None) == status
            if rb is None:
                assert L.pcr_vgicp_direct_residuals(tt.handle, ss.handle, T, md, nb, 0, capi._ptr(res)) == status
            assert np.all(out == 7.0) and np.all(Tout == 7.0) and np.all(res == 7.0) and iters.value == -5
        # the messages of the nearest-centroid pass
        with pytest.raises(ValueError, match="different contexts"):
            capi.vgicp_direct_linearize(t, foreign, g2["T"], 0.8, 7)
        with pytest.raises(ValueError, match="scan has no covariances"):
            capi.vgicp_direct_linearize(t, bare, g2["T"], 0.8, 7)
        with pytest.raises(ValueError, match="target has no covariances"):
            capi.vgicp_direct_align(nocov, s, g2["T"], 3, 1e-3, 0.8, 7)
        with pytest.raises(ValueError, match="voxel target"):
            capi.vgicp_direct_residuals(points, s, g2["T"], 0.8, 7)
        with pytest.raises(ValueError, match="neighbors"):
            capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 9)
        with pytest.raises(ValueError, match="neighbors"):
            t.lookup(g2["source"], 3)
        with pytest.raises(ValueError, match="voxel target"):
            points.lookup(g2["source"], 7)
        # residuals need the caller's order
        sorted_scan = capi.Scan(ctx, g2["source"])
        sorted_scan.estimate_covariances(10, want=False)
        with pytest.raises(ValueError, match="caller's order"):
            capi.vgicp_direct_residuals(t, sorted_scan, g2["T"], 0.8, 7)
        assert capi.vgicp_direct_linearize(t, sorted_scan, g2["T"], 0.8, 7)[28] == 4607
        foreign.close()
    finally:
        other.close()


def _raw_entry_points(capi):
    """The three entry points with plain pointer arguments, so that a NULL can stand where ``_capi`` wants an array."""
    C, L = capi.C, capi.lib()
    vp = C.c_void_p
    return (C.cast(L.pcr_vgicp_direct_linearize, C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_double, C.c_int, vp, C.c_uint, vp)),
            C.cast(L.pcr_vgicp_direct_align, C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, C.c_uint, vp, vp, vp)),
            C.cast(L.pcr_vgicp_direct_residuals, C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_double, C.c_int, C.c_uint, vp)),
            C.cast(L.pcr_target_voxels_lookup, C.CFUNCTYPE(C.c_int, vp, vp, C.c_int64, C.c_int, vp)))


def test_null_arguments_are_refused_first(capi, ctx, g2, sides):
    """The first refusal of the list: a NULL argument is PCR_ERR_INVALID whatever else is wrong with the call (neighbors 5, a
    bad kernel, max_dist -1 here), and nothing is written."""
    cp, t = sides["plane"][:2]
    s = scan_of(capi, ctx, g2, cp)
    lin, align, resid, lookup = _raw_entry_points(capi)
    T = np.ascontiguousarray(g2["T"], dtype=np.float64).reshape(16)
    bad_kind, keep = capi._rb((9, 1.0))
    q = np.ascontiguousarray(g2["source"][:4])
    p = lambda a: a.ctypes.data                                                   # noqa: E731
    for nb, rb, md in ((7, None, 0.8), (5, bad_kind, -1.0)):
        out, Tout, res, idx = np.full(29, 7.0), np.full(16, 7.0), np.full((2000, 27), 7.0), np.full((4, 27), 7, np.int64)
        iters = capi.C.c_int(-5)
        it = capi.C.addressof(iters)
        for args in ((None, s.handle, p(T), md, nb, rb, 0, p(out)), (t.handle, None, p(T), md, nb, rb, 0, p(out)),
                     (t.handle, s.handle, None, md, nb, rb, 0, p(out)), (t.handle, s.handle, p(T), md, nb, rb, 0, None)):
            assert lin(*args) == capi.PCR_ERR_INVALID, args
        for args in ((None, s.handle, p(T), 5, 1e-3, md, nb, rb, 0, p(Tout), it, None),
                     (t.handle, None, p(T), 5, 1e-3, md, nb, rb, 0, p(Tout), it, None),
                     (t.handle, s.handle, None, 5, 1e-3, md, nb, rb, 0, p(Tout), it, None),
                     (t.handle, s.handle, p(T), 5, 1e-3, md, nb, rb, 0, None, it, None)):
            assert align(*args) == capi.PCR_ERR_INVALID, args
        for args in ((None, s.handle, p(T), md, nb, 0, p(res)), (t.handle, None, p(T), md, nb, 0, p(res)),
                     (t.handle, s.handle, None, md, nb, 0, p(res)), (t.handle, s.handle, p(T), md, nb, 0, None)):
            assert resid(*args) == capi.PCR_ERR_INVALID, args
        for args in ((None, p(q), 4, nb, p(idx)), (t.handle, None, 4, nb, p(idx)), (t.handle, p(q), 4, nb, None),
                     (t.handle, p(q), -1, nb, p(idx))):
            assert lookup(*args) == capi.PCR_ERR_INVALID, args
        assert b"NULL argument" in capi.lib().pcr_last_error()
        assert np.all(out == 7.0) and np.all(Tout == 7.0) and np.all(res == 7.0) and np.all(idx == 7) and iters.value == -5
    # iterations and the trace may be NULL: they are optional
    assert align(t.handle, s.handle, p(T), 2, 1e-3, 0.8, 7, None, 0, p(Tout), None, None) == capi.PCR_OK and not np.all(Tout == 7.0)


def test_context_with_a_communicator_is_refused(capi, ctx, g2, sides):
    """The last refusal of the list: PCR_ERR_UNSUPPORTED from all three entry points while a communicator (here: one rank) is
    attached to the context, whatever the flags; nothing is written, and the sums afterwards are the bits from before."""
    cp, t = sides["plane"][:2]
    s = scan_of(capi, ctx, g2, cp)
    T = np.ascontiguousarray(g2["T"], dtype=np.float64).reshape(16)
    L = capi.lib()
    before = {nb: capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, nb) for nb in NEIGHBORS}
    res_before = capi.vgicp_direct_residuals(t, s, g2["T"], 0.8, 7)
    cauchy, keep = capi._rb(capi.check_robust("cauchy", 1.0))
    empty = capi.Target.voxels(ctx, np.ascontiguousarray(g2["target"][:5]), 1.0)
    empty.set_voxel_covariances(capi.COV_RAW)
    ctx.comm_init(capi.comm_unique_id(), 1, 0)
    try:
        for nb in NEIGHBORS:
            for flags in (0, capi.FLAG_LOCAL_ONLY):
                for rb in (None, cauchy):
                    out, Tout, res = np.full(29, 7.0), np.full(16, 7.0), np.full((2000, nb), 7.0)
                    iters = capi.C.c_int(-5)
                    assert L.pcr_vgicp_direct_linearize(t.handle, s.handle, T, 0.8, nb, rb, flags, out) == capi.PCR_ERR_UNSUPPORTED
                    assert L.pcr_vgicp_direct_align(t.handle, s.handle, T, 5, 1e-3, 0.8, nb, rb, flags, Tout, capi.C.byref(iters),
                                                    None) == capi.PCR_ERR_UNSUPPORTED
                    assert L.pcr_vgicp_direct_residuals(t.handle, s.handle, T, 0.8, nb, flags, capi._ptr(res)) == capi.PCR_ERR_UNSUPPORTED
                    assert np.all(out == 7.0) and np.all(Tout == 7.0) and np.all(res == 7.0) and iters.value == -5
            with pytest.raises(capi.PcrError, match="communicator"):
                capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, nb)
            with pytest.raises(capi.PcrError, match="communicator"):
                capi.vgicp_direct_align(t, s, g2["T"], 5, 1e-3, 0.8, nb)
            with pytest.raises(capi.PcrError, match="communicator"):
                capi.vgicp_direct_residuals(t, s, g2["T"], 0.8, nb)
        # what comes earlier in the list still wins
        with pytest.raises(ValueError, match="max_dist"):
            capi.vgicp_direct_linearize(t, s, g2["T"], 0.0, 7)
        with pytest.raises(ValueError, match="neighbors"):
            capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 9)
        # a target with no kept voxel does not get past it either
        with pytest.raises(capi.PcrError, match="communicator"):
            capi.vgicp_direct_linearize(empty, s, g2["T"], 0.8, 7)
        # the lookup is a query of the target, not a pass: it stays available
        assert t.lookup(g2["source"][:8], 7).shape == (8, 7)
    finally:
        ctx.comm_destroy()
    for nb in NEIGHBORS:
        assert np.array_equal(before[nb], capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, nb))
    assert np.array_equal(res_before, capi.vgicp_direct_residuals(t, s, g2["T"], 0.8, 7))


def test_direct_times_line(g2):
    """PCR_DIRECT_TIMES=1 (tools/direct_time.py reads it): one line per direct pass on stderr, its prefix one of
    tools/timing.py's, the phases kernel_ms and fold_ms in that order, read back through timing.py's own regex.  The switch
    is read once per process, so the calls run in one fresh child; without it a pass writes nothing."""
    import importlib.util
    import math
    import os
    import re
    import subprocess
    import sys
    from conftest import REPO
    spec = importlib.util.spec_from_file_location("pcr_tools_timing", os.path.join(REPO, "tools", "timing.py"))
    timing = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(timing)
    child = r"""
import sys
import numpy as np
from point_cloud_registration_amd import _capi
g = dict(np.load(sys.argv[1]))
ctx = _capi.get_context(0)
t = _capi.Target.voxels(ctx, g["target"], 1.0)
t.set_voxel_covariances(_capi.COV_PLANE, 1e-3)
s = _capi.Scan(ctx, g["source"], flags=_capi.FLAG_KEEP_ORDER)
s.estimate_covariances(10, want=False)
for nb in (1, 7, 27):
    _capi.vgicp_direct_linearize(t, s, g["T"], 0.8, nb)
_capi.vgicp_direct_linearize(t, s, g["T"], 0.8, 7, robust=(_capi.ROBUST_CAUCHY, 1.0))
_capi.vgicp_linearize(t, s, g["T"], 0.8)
_capi.vgicp_direct_residuals(t, s, g["T"], 0.8, 7)
"""
    fixture = os.path.join(REPO, "tests", "golden", "g2_mini_street.npz")
    for switch, want in (("1", [1, 7, 27, 7]), ("0", [])):
        env = dict(os.environ, PCR_DIRECT_TIMES=switch, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", child, fixture], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [line for line in r.stderr.splitlines() if line.startswith("pcr_")]
        assert len(lines) == len(want), lines
        for line, nb in zip(lines, want):
            assert re.match(rf"^pcr_direct_times n 2000 neighbors {nb} kernel_ms [0-9]+\.[0-9]{{4}} fold_ms [0-9]+\.[0-9]{{4}}$", line), line
            assert line.split(" ", 1)[0] in timing.PREFIXES
            got = timing.phase_ms(line)
            assert [name for name, _ in got] == ["kernel_ms", "fold_ms"] and all(math.isfinite(v) and v >= 0 for _, v in got), line


def test_target_with_no_kept_voxel(capi, ctx, g2, sides):
    cp = sides["plane"][0]
    t = capi.Target.voxels(ctx, np.ascontiguousarray(g2["target"][:5]), 1.0)
    assert t.size() == 0
    t.set_voxel_covariances(capi.COV_RAW)
    s = scan_of(capi, ctx, g2, cp)
    for nb in NEIGHBORS:
        assert np.array_equal(capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, nb), np.zeros(29))
        assert np.all(np.isposinf(capi.vgicp_direct_residuals(t, s, g2["T"], 0.8, nb)))
        assert np.all(t.lookup(g2["source"], nb) == -1)
        # ... and what the refusals refuse is still refused
        with pytest.raises(ValueError):
            capi.vgicp_direct_linearize(t, s, g2["T"], 0.0, nb)
    import point_cloud_registration_amd as pcr
    reg = pcr.VGICP(voxel_size=1.0, neighbors=7)
    reg.set_target(np.ascontiguousarray(g2["target"][:5]))
    H, g, e2 = reg.calc_H_g_e2(np.eye(4), g2["source"])
    assert not H.any() and not g.any() and e2 == 0.0 and reg.last_correspondences == 0


def test_from_stats_targets(capi, ctx, g2, sides, tp):
    """A target made from statistics has no keys until the caller supplies them; keys that do not ascend strictly are refused
    by the first call that needs the lookup, and ascending ones serve it."""
    cp, t0, cv, mean, keys = sides["plane"]
    st = t0.voxel_stats(("norm", "icov"))
    t = capi.Target.voxels_from_stats(ctx, mean, st["norm"], st["icov"], 1.0)
    t.set_voxel_covariances(cov=cv)
    s = scan_of(capi, ctx, g2, cp)
    with pytest.raises(ValueError, match="holds no keys"):
        t.lookup(tp, 7)
    with pytest.raises(ValueError, match="holds no keys"):
        capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 7)
    for bad in (keys[::-1], np.concatenate([keys[:1], keys[:-1]])):          # descending; one key twice
        t.set_voxel_keys(np.ascontiguousarray(bad))
        with pytest.raises(ValueError, match="ascend"):
            t.lookup(tp, 7)
        out = np.full(29, 7.0)
        T = np.ascontiguousarray(g2["T"], dtype=np.float64).reshape(16)
        assert capi.lib().pcr_vgicp_direct_linearize(t.handle, s.handle, T, 0.8, 7, None, 0, out) == capi.PCR_ERR_INVALID
        assert np.all(out == 7.0)
    t.set_voxel_keys(keys)
    assert np.array_equal(t.lookup(tp, 27), dn.lookup(tp, 1.0, keys, 27))
    assert np.array_equal(capi.vgicp_direct_linearize(t, s, g2["T"], 0.8, 7), capi.vgicp_direct_linearize(t0, s, g2["T"], 0.8, 7))
    with pytest.raises(ValueError, match="build"):
        t0.set_voxel_keys(keys)
    with pytest.raises(ValueError):
        t.set_voxel_keys(keys[:-1])
