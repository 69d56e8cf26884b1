"""Robust kernels inside the pass of GICP, VGICP, SymmetricICP and ColoredICP on the GPU: the squared residuals, the weighted
sums, weights of one, determinism and isolation, refusals, and align on the end-to-end case of tests/robust_cases.py.

Fixtures and base scans are those of the plain passes' tests: g2_mini_street with random unit scan normals (test_gpu_symm.py) or
random gradients and scan intensities (test_gpu_color.py), 1823 of 2000 kept; the point / voxel lattice of g16_pass_cases with
random covariances and dist_cases.base_scan (test_gpu_dist_pass.py), 1600 of 2000 kept at gate 1.  tests/robust_cases.py
restates the kernels on the restated terms of symm_cases / color_cases / dist_cases.

The bound on the weighted sums, per entry: 1.5 x the plain pass's own bound (symm_cases.sum_bound, color_cases.sum_bound,
gicp_cases.sum_bound) evaluated on the sums of the UNWEIGHTED magnitudes.  Every weight is <= 1, so the plain bound on the
unweighted magnitudes covers the roundings of the weighted terms and of their summation.  What it does not cover is the
weight itself, computed from an s that carries a relative error delta (a handful of roundings; for GICP / VGICP the
conditioning of the inverse, the 16 / eps_min of gicp_cases.sum_bound): a weighted term w(s) x moves by |dw/ds| s delta |x|, and
|s dw/ds| <= 1/2 for all four kernels --
    huber   w = c s^-1/2 above c2:      s dw/ds = -w / 2,                      |.| <= 1/2
    cauchy  w = 1 / (1 + u), u = s/c2:  s dw/ds = -u / (1 + u)^2,              |.| <= 1/4
    tukey   w = (1 - u)^2 below c2:     s dw/ds = -2 u (1 - u),                |.| <= 1/2
    gm      w = 1 / (1 + u)^2:          s dw/ds = -2 u / (1 + u)^3,            |.| <= 8/27
-- so the weight adds at most delta / 2 of the term's unweighted size, half of what the plain bound already allows for delta:
the factor 1.5.  It is derived, not tuned."""

import numpy as np
import pytest

import color_cases as cc
import dist_cases as dc
import gicp_cases as gc
import pass_cases as pc
import robust_cases as rc
import symm_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu

ALIGNERS = ("symm", "color", "gicp", "vgicp")
SMALL = (1, 2, 255, 256, 257)
# points per lane in flight of the robust kernels (SYMM_ROBUST_W, COLOR_ROBUST_W, GICP_ROBUST_W, VGICP_ROBUST_W); the plain ones
ROBUST_W = {"symm": 2, "color": 2, "gicp": 3, "vgicp": 2}
PLAIN_W = {"symm": 3, "color": 2, "gicp": 3, "vgicp": 2}
LAMBDA = 0.968
KIND_ID = {"huber": 1, "cauchy": 2, "tukey": 3, "gm": 4}


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    return capi.get_context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def case():
    return rc.e2e_case()


class Side:
    """One aligner over its base scan: the device target, the restated unweighted terms t (m N0, 28), s (N0, m), keep (N0,),
    and how to upload a scan of rows of the base with its payload."""

    def __init__(self, name, capi, ctx, tgt, T, md, scan, payload, extra, t, s, keep, bound):
        self.name, self.capi, self.ctx, self.tgt, self.T, self.md = name, capi, ctx, tgt, T, md
        self.scan, self.payload, self.extra = scan, payload, extra
        self.t, self.s, self.keep, self.bound = t, s, keep, bound
        self.m = s.shape[1]
        self.c = rc.median_scale(s[keep])
        for a in (self.t, self.s, self.keep):
            a.setflags(write=False)
        self.plain = getattr(capi, f"{name}_linearize")
        self.robust = getattr(capi, f"{name}_linearize_robust")
        self.resid = getattr(capi, f"{name}_residuals")

    def upload(self, rows, flags=None):
        s = self.capi.Scan(self.ctx, np.ascontiguousarray(self.scan[rows]), flags=self.capi.FLAG_KEEP_ORDER if flags is None else flags)
        setter = {"symm": s.set_normals, "color": s.set_intensity, "gicp": s.set_covariances, "vgicp": s.set_covariances}[self.name]
        setter(np.ascontiguousarray(self.payload[rows]))
        return s

    def lin(self, s, kind=None, c=None, T=None):
        T = self.T if T is None else T
        if kind is None:
            return self.plain(self.tgt, s, T, self.md, *self.extra)
        return self.robust(self.tgt, s, T, self.md, *self.extra, robust=(KIND_ID[kind], self.c if c is None else c))

    def residuals(self, s):
        r = self.resid(self.tgt, s, self.T, self.md, *self.extra)
        return r.reshape(len(r), self.m)

    def reference(self, mult, kind, c=None):
        """The weighted sums of the scan in which base row i appears mult[i] times -> (ref, bound, count)."""
        mm = np.tile(np.asarray(mult, dtype=np.float64), self.m)
        tm = self.t * mm[:, None]
        w = rc.weight(kind, self.s.T.ravel(), self.c if c is None else c)
        ref = gc.fsum_cols(tm * w[:, None])[0]
        mag = gc.fsum_cols(tm)[1]
        count = int(round(float(np.sum(np.asarray(mult, dtype=np.float64) * self.keep))))
        return ref, 1.5 * self.bound(count, mag), count


def _symm_side(capi, ctx, orc, g2):
    T, src, md = g2["T"], g2["source"], float(g2["max_dist"])
    n_p = sc.unit_normals(len(src))
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(md)
    _, t, s, keep = rc.terms_symm(None, 1.0, T, src, orc.transform(T, src), g2["target"][j], n_p, g2["plane_normals"][j], mask)
    tgt = capi.Target.points(ctx, g2["target"])
    tgt.set_normals(g2["plane_normals"])
    return Side("symm", capi, ctx, tgt, T, md, src, n_p, (0.0,), t, s[:, None], keep, sc.sum_bound)


def _color_side(capi, ctx, orc, g2):
    T, src, md = g2["T"], g2["source"], float(g2["max_dist"])
    I_q = cc.field(g2["target"])
    G = (0.3 * np.random.default_rng(1).normal(size=(5000, 3))).astype(np.float32)
    I_p = np.random.default_rng(0).uniform(0, 1, 2000).astype(np.float32)
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(md)
    _, t, s, keep = rc.terms_color(None, 1.0, T, src, orc.transform(T, src), g2["target"][j], g2["plane_normals"][j], I_q[j], G[j], I_p,
                                   mask, LAMBDA)
    tgt = capi.Target.points(ctx, g2["target"])
    tgt.set_normals(g2["plane_normals"])
    tgt.set_intensity(I_q, G)
    return Side("color", capi, ctx, tgt, T, md, src, I_p, (LAMBDA,), t, s, keep, cc.sum_bound)


def _dist_side(name, capi, ctx, orc, built):
    which = "pt" if name == "gicp" else "vox"
    T, scan, cls = dc.base_scan(which)
    tp = orc.transform(T, scan)
    if name == "gicp":
        t32 = built["pt"]["target32"]
        Cp, Cq = dc.spd_pair(len(scan), len(t32), seed=24)
        tgt = capi.Target.points(ctx, t32)
        tgt.set_covariances(Cq)
        dist, idx = orc.nn_brute(t32, tp)
        mask = dist < np.float32(dc.BASE_GATE)
        q, Cm, res = t32[idx], Cq[idx], "f32"
    else:
        vox = built["vox"]
        Cp, cv = dc.spd_pair(len(scan), 64, seed=25)
        tgt = capi.Target.voxels(ctx, vox["target64"], vox["voxel_size"])
        tgt.set_voxel_covariances(cov=cv.astype(np.float64))
        mean, Cv = tgt.voxel_stats(("mean",))["mean"], tgt.get_voxel_covariances()
        dist, idx = orc.nn_brute_f64(mean, tp)
        mask = dist < dc.BASE_GATE
        q, Cm, res = mean[idx], Cv[idx], "f64"
    assert np.array_equal(mask, cls == 0)
    _, t, s, keep, eps_min = rc.terms_dist(None, 1.0, T, scan, tp, q, Cp, Cm, mask, res)
    side = Side(name, capi, ctx, tgt, T, dc.BASE_GATE, scan, Cp, (), t, s[:, None], keep, lambda n, mag: gc.sum_bound(n, eps_min, mag))
    # |d|^T |M| |d| and eps_min, for the bound on s itself
    M = dc.weights_closed(T, Cp, Cm)[0]
    d = (tp - q).astype(np.float64) if res == "f32" else tp.astype(np.float64) - q
    side.s_mag = np.einsum("ni,nij,nj->n", np.abs(d), np.abs(M), np.abs(d))
    side.eps_min = eps_min
    return side


@pytest.fixture(scope="module")
def sides(capi, ctx, orc, g2):
    built = pc.build_all(load_golden("g16_pass_cases.npz"))
    out = {"symm": _symm_side(capi, ctx, orc, g2), "color": _color_side(capi, ctx, orc, g2),
           "gicp": _dist_side("gicp", capi, ctx, orc, built), "vgicp": _dist_side("vgicp", capi, ctx, orc, built)}
    return out


def _sizes(side):
    return SMALL + (len(side.scan),)


# ----------------------------------------------------------------------------- 1. residuals
@pytest.mark.parametrize("name", ALIGNERS)
def test_residuals(sides, name):
    """s of every scan point in the caller's order, inf where the point has no correspondence.  SymmetricICP, ColoredICP: the
    restated bits.  GICP, VGICP: within (16 / eps_min + 16) 2^-53 |d|^T |M| |d| -- the relative error of the inverse that the
    eps_min argument of gicp_cases.sum_bound stands for, and a handful of roundings of the quadratic form."""
    side = sides[name]
    N0 = len(side.scan)
    ref = side.s
    assert np.array_equal(np.isinf(ref[:, 0]), ~side.keep) and 0 < side.keep.sum() < N0
    perm = np.random.default_rng(3).permutation(N0)
    for rows in [np.arange(n) for n in _sizes(side)] + [perm]:
        for flags in (side.capi.FLAG_KEEP_ORDER, side.capi.FLAG_NO_SCAN_SORT):
            got = side.residuals(side.upload(rows, flags))
            want = ref[rows]
            assert got.shape == want.shape and got.dtype == np.float64
            assert np.array_equal(np.isinf(got), np.isinf(want)), (name, len(rows))
            fin = np.isfinite(want)
            assert np.all(got[fin] >= 0.0)
            if name in ("symm", "color"):
                assert np.array_equal(got, want), (name, len(rows), np.max(np.abs(got[fin] - want[fin])))
            else:
                tol = (16.0 / side.eps_min + 16.0) * gc.EPS53 * side.s_mag[rows][:, None]
                err = np.abs(got[fin] - want[fin])
                print(f"{name} n {len(rows)}: max error / bound {np.max(err / tol[fin]):.3e}")
                assert np.all(err <= tol[fin]), (name, len(rows))
    # a scan that does not know the caller's order is refused, with a payload estimated on it (which needs no order)
    if name != "color":
        plain = side.capi.Scan(side.ctx, side.scan)
        plain.estimate_normals(10, want=False) if name == "symm" else plain.estimate_covariances(10, want=False)
        side.plain(side.tgt, plain, side.T, side.md, *side.extra)
        with pytest.raises(ValueError, match="order"):
            side.resid(side.tgt, plain, side.T, side.md, *side.extra)


def test_residuals_through_the_classes(sides, g2):
    """MatchPass.residuals takes the extras as calc_H_g_e2 takes them and returns the entry point's array."""
    import point_cloud_registration_amd as pcr
    side = sides["symm"]
    reg = pcr.SymmetricICP(max_dist=side.md)
    reg.set_target(g2["target"], norm=g2["plane_normals"])
    got = reg.residuals(side.T, side.scan, source_normals=side.payload)
    assert got.shape == (2000,) and np.array_equal(got, side.s[:, 0])
    side = sides["color"]
    reg = pcr.ColoredICP(max_dist=side.md, lambda_geometric=LAMBDA, robust="tukey", robust_scale=0.1)
    reg.set_target(g2["target"], cc.field(g2["target"]), norm=g2["plane_normals"],
                   gradient=(0.3 * np.random.default_rng(1).normal(size=(5000, 3))).astype(np.float32))
    got = reg.residuals(side.T, side.scan, source_intensity=side.payload)
    assert got.shape == (2000, 2) and np.array_equal(got, side.s)              # (whatever the object's own kernel)


# ----------------------------------------------------------------------------- 2. sums
@pytest.mark.parametrize("name", ALIGNERS)
def test_both_branches_live(sides, name):
    """c2 = the restated median of s over the kept correspondences: between 20 % and 80 % of them lie above it."""
    side = sides[name]
    s = side.s[side.keep]
    above = np.mean(s > side.c * side.c)
    print(f"{name}: c {side.c:.4e}, s > c2 on {above:.3f} of {s.size} (per row {np.mean(s > side.c * side.c, axis=0)})")
    assert 0.2 <= above <= 0.8


def _check_sums(side, s, mult, what):
    plain = side.lin(s)
    for kind in rc.KINDS:
        out = side.lin(s, kind)
        ref, bound, count = side.reference(mult, kind)
        err = np.abs(out[:28] - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            print(f"{what} {kind}: kept {count}, max error / bound {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3e}")
        assert np.all(np.isfinite(out)) and out[28] == count == plain[28], (what, kind, out[28], count, plain[28])
        assert np.all(err <= bound), (what, kind, np.nonzero(err > bound)[0].tolist())
        assert np.array_equal(side.lin(s, kind), out), (what, kind, "second call")
    return plain


@pytest.mark.parametrize("n", SMALL + (2000,))
@pytest.mark.parametrize("name", ALIGNERS)
def test_sums(sides, name, n):
    side = sides[name]
    s = side.upload(np.arange(n))
    _check_sums(side, s, np.arange(len(side.scan)) < n, (name, n))


def test_grid_rule_on_this_device(cus):
    """The sizes below make slots and trips live only while the reduce grid is 8 blocks per CU."""
    assert dc.stride_points(cus) == 524288, cus


@pytest.mark.parametrize("name, k", [(a, k) for a in ALIGNERS for k in range(ROBUST_W[a])])
def test_sums_live_slots(sides, cus, name, k):
    """dist_cases.big_sizes with the robust kernel's W: slot 1 (.. W - 1), then the second trip carry live points."""
    side = sides[name]
    n = dc.big_sizes(cus, ROBUST_W[name])[k]
    N0 = len(side.scan)
    s = side.upload(np.arange(n) % N0)
    try:
        plain = _check_sums(side, s, np.bincount(np.arange(n) % N0, minlength=N0), (name, n))
        assert 0 < plain[28] < n
    finally:
        s.close()


# ----------------------------------------------------------------------------- 3. weights of one
@pytest.mark.parametrize("name", ALIGNERS)
def test_weights_of_one(sides, name):
    """scale = 1e150: c2 = 1e300, every weight is exactly 1 and every product with it exact, so a robust kernel that keeps the
    plain kernel's W adds the same numbers in the same order: the plain entry point's 29 values bit for bit (color, gicp,
    vgicp).  k_symm_robust carries 2 points per lane where k_symm_reduce carries 3 (its registers: symm.hip), so a lane sums
    other points: the same numbers in another order, within the bound of the sums; the count is exact either way."""
    side = sides[name]
    s = side.upload(np.arange(len(side.scan)))
    plain = side.lin(s)
    for kind in rc.KINDS:
        out = side.lin(s, kind, c=1e150)
        if ROBUST_W[name] == PLAIN_W[name]:
            assert np.array_equal(out, plain), (name, kind)
        else:
            ref, bound, count = side.reference(np.ones(len(side.scan)), None)
            assert out[28] == plain[28] == count
            assert np.all(np.abs(out[:28] - ref) <= bound) and np.all(np.abs(out[:28] - plain[:28]) <= bound), (name, kind)


# ----------------------------------------------------------------------------- 4. determinism and isolation
@pytest.mark.parametrize("name", ALIGNERS)
def test_none_and_null_are_the_plain_pass(sides, name):
    side = sides[name]
    s = side.upload(np.arange(len(side.scan)))
    plain = side.lin(s)
    assert np.array_equal(side.robust(side.tgt, s, side.T, side.md, *side.extra, robust=None), plain)              # rb = NULL
    for scale in (1.0, -1.0, float("nan")):                                                                       # (not read)
        assert np.array_equal(side.robust(side.tgt, s, side.T, side.md, *side.extra, robust=(0, scale)), plain)
    T1, it1, tr1 = getattr(side.capi, f"{name}_align")(side.tgt, s, side.T, 3, 0.0, side.md, *side.extra, want_trace=True)
    T2, it2, tr2 = getattr(side.capi, f"{name}_align_robust")(side.tgt, s, side.T, 3, 0.0, side.md, *side.extra, robust=None, want_trace=True)
    assert it1 == it2 == 3 and np.array_equal(T1, T2) and np.array_equal(tr1, tr2)


def test_neighbours_undisturbed(capi, ctx, g2, sides):
    """A robust call between two plain calls of ICP / GICP / SymmetricICP / ColoredICP on the same device scan and context
    leaves their bits alone, in both pipeline variants -- the pattern of test_gpu_symm.test_neighbours_undisturbed."""
    T, src, tgt, md = g2["T"], g2["source"], g2["target"], float(g2["max_dist"])
    icp = capi.Target.points(ctx, tgt)
    gicp = capi.Target.points(ctx, tgt)
    gicp.estimate_covariances(10, capi.COV_PLANE, 1e-3, want=False)
    symm, color = sides["symm"].tgt, sides["color"].tgt
    s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    s.estimate_covariances(10, capi.COV_PLANE, 1e-3, want=False)
    s.set_normals(sides["symm"].payload)
    s.set_intensity(sides["color"].payload)
    plain = lambda: (capi.linearize(icp, s, capi.ICP, T, md), capi.gicp_linearize(gicp, s, T, md), capi.symm_linearize(symm, s, T, md),
                     capi.color_linearize(color, s, T, md, LAMBDA))
    for variant in (2, 1):
        with ctx.pipeline(variant=variant):
            before = plain()
            rb = (KIND_ID["tukey"], 0.05)
            r1 = (capi.gicp_linearize_robust(gicp, s, T, md, robust=(KIND_ID["huber"], 1.0)), capi.symm_linearize_robust(symm, s, T, md, 0.0, robust=rb),
                  capi.color_linearize_robust(color, s, T, md, LAMBDA, robust=rb), capi.symm_residuals(symm, s, T, md), capi.gicp_residuals(gicp, s, T, md))
            after = plain()
            r2 = (capi.gicp_linearize_robust(gicp, s, T, md, robust=(KIND_ID["huber"], 1.0)), capi.symm_linearize_robust(symm, s, T, md, 0.0, robust=rb),
                  capi.color_linearize_robust(color, s, T, md, LAMBDA, robust=rb), capi.symm_residuals(symm, s, T, md), capi.gicp_residuals(gicp, s, T, md))
            for b, a in zip(before + r1, after + r2):
                assert np.array_equal(b, a)
            assert all(o[28] == 1823 for o in before) and all(o[28] == 1823 for o in r1[:3])
            assert not np.array_equal(r1[1][:28], before[2][:28])                  # (the kernel did weigh)


def test_setting_belongs_to_the_aligner(g2, sides):
    """Two aligners with different kernels over ONE cached device scan: each returns what it returns alone, in any order."""
    import point_cloud_registration_amd as pcr
    side = sides["symm"]
    T, src = side.T, side.scan
    regs = {}
    for key, kw in (("none", {}), ("huber", dict(robust="huber", robust_scale=side.c)), ("tukey", dict(robust="tukey", robust_scale=side.c))):
        regs[key] = pcr.SymmetricICP(max_dist=side.md, **kw)
        regs[key].set_target(g2["target"], norm=g2["plane_normals"])
    scan = regs["none"].upload(src, keep_order=True)
    alone = {k: r.calc_H_g_e2(T, scan, source_normals=side.payload) for k, r in regs.items()}
    for order in (("tukey", "none", "huber"), ("huber", "tukey", "none", "tukey")):
        for k in order:
            got = regs[k].calc_H_g_e2(T, scan, source_normals=side.payload)
            assert all(np.array_equal(a, b) for a, b in zip(got, alone[k])), (order, k)
    assert not np.array_equal(alone["huber"][0], alone["tukey"][0]) and not np.array_equal(alone["none"][0], alone["huber"][0])
    # the class returns the entry point's sums
    s = side.upload(np.arange(len(src)))
    out = side.lin(s, "huber")
    H, g, e2 = alone["huber"]
    assert np.array_equal(H[gc.TRIU], out[:21]) and np.array_equal(g, out[21:27]) and e2 == out[27]
    assert np.array_equal(alone["none"][0][gc.TRIU], side.lin(s)[:21])


# ----------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("name", ALIGNERS)
def test_refusals(sides, name):
    """Bad kind, scale <= 0, NaN, inf, 1e200: PCR_ERR_INVALID with out and T_out untouched.  A Tukey scale below every
    residual: every weight is 0, PCR_ERR_SINGULAR from align."""
    side, capi = sides[name], sides[name].capi
    s = side.upload(np.arange(len(side.scan)))
    L = capi.lib()
    T = np.ascontiguousarray(side.T, dtype=np.float64).reshape(16)
    extra = [float(v) for v in side.extra]
    import ctypes
    for kind, scale in ((5, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (3, float("nan")), (4, float("inf")), (1, 1e200), (3, -float("inf"))):
        p, keep = capi._rb((kind, scale))
        out = np.full(29, 7.25)
        st = getattr(L, f"pcr_{name}_linearize_robust")(side.tgt.handle, s.handle, T, side.md, *extra, p, 0, out)
        assert st == capi.PCR_ERR_INVALID and np.all(out == 7.25), (kind, scale, st)
        T_out, iters, trace = np.full(16, 7.25), ctypes.c_int(-3), np.full((2, 45), 7.25)
        st = getattr(L, f"pcr_{name}_align_robust")(side.tgt.handle, s.handle, T, 2, 1e-3, side.md, *extra, p, 0, T_out, ctypes.byref(iters),
                                                   trace.ctypes.data_as(ctypes.c_void_p))
        assert st == capi.PCR_ERR_INVALID and np.all(T_out == 7.25) and np.all(trace == 7.25) and iters.value == -3, (kind, scale, st)
        with pytest.raises(ValueError):
            side.robust(side.tgt, s, side.T, side.md, *side.extra, robust=(kind, scale))
    # the plain call's refusals stay: a scan without its payload
    bare = capi.Scan(side.ctx, side.scan, flags=capi.FLAG_KEEP_ORDER)
    with pytest.raises(ValueError):
        side.robust(side.tgt, bare, side.T, side.md, *side.extra, robust=(1, 1.0))
    with pytest.raises(ValueError):
        side.resid(side.tgt, bare, side.T, side.md, *side.extra)
    # Tukey below every residual
    tiny = 0.5 * float(np.sqrt(side.s[np.isfinite(side.s) & (side.s > 0)].min()))
    out = side.lin(s, "tukey", c=tiny)
    assert out[28] == side.keep.sum() and not np.any(out[:28])
    with pytest.raises(np.linalg.LinAlgError):
        getattr(capi, f"{name}_align_robust")(side.tgt, s, side.T, 5, 1e-3, side.md, *side.extra, robust=(3, tiny))


@pytest.mark.parametrize("name, word", [("symm", "min_cos"), ("color", "lambda_geometric")])
def test_unit_parameter_is_refused_first(sides, name, word):
    """min_cos / lambda_geometric outside [0, 1] or NaN: PCR_ERR_INVALID from all five entry points with every output
    untouched, and the message names the parameter -- also under a kernel that would itself be refused (the parameter is
    checked before the kernel) and on a scan without its payload (before PCR_ERR_NO_TARGET)."""
    import ctypes
    side, capi = sides[name], sides[name].capi
    L = capi.lib()
    T = np.ascontiguousarray(side.T, dtype=np.float64).reshape(16)
    with_payload = side.upload(np.arange(257))
    bare = capi.Scan(side.ctx, np.ascontiguousarray(side.scan[:257]), flags=capi.FLAG_KEEP_ORDER)
    entry = lambda what: getattr(L, f"pcr_{name}_{what}")
    good, keep_good = capi._rb((1, 1.0))
    bad, keep_bad = capi._rb((5, 1.0))

    def refused(st, what):
        msg = L.pcr_last_error().decode()
        assert st == capi.PCR_ERR_INVALID and word in msg and "robust" not in msg, (what, st, msg)

    for s in (with_payload, bare):
        t, h = side.tgt.handle, s.handle
        for v in (1.5, -0.1, float("nan")):
            for mid in ((v,), (v, good), (v, bad)):
                rob = "_robust" if len(mid) == 2 else ""
                out = np.full(29, 7.25)
                refused(entry("linearize" + rob)(t, h, T, side.md, *mid, 0, out), ("linearize" + rob, v))
                assert np.all(out == 7.25)
                T_out, iters, trace = np.full(16, 7.25), ctypes.c_int(-3), np.full((2, 45), 7.25)
                refused(entry("align" + rob)(t, h, T, 2, 1e-3, side.md, *mid, 0, T_out, ctypes.byref(iters),
                                             trace.ctypes.data_as(ctypes.c_void_p)), ("align" + rob, v))
                assert np.all(T_out == 7.25) and np.all(trace == 7.25) and iters.value == -3
            s_out = np.full((257, side.m), 7.25)
            refused(entry("residuals")(t, h, T, side.md, v, 0, s_out.ctypes.data_as(ctypes.c_void_p)), ("residuals", v))
            assert np.all(s_out == 7.25)
    # (the same calls with a parameter inside [0, 1]: the bad kernel and the missing payload are what is refused)
    out = np.full(29, 7.25)
    assert entry("linearize_robust")(side.tgt.handle, with_payload.handle, T, side.md, *side.extra, bad, 0, out) == capi.PCR_ERR_INVALID
    assert "robust" in L.pcr_last_error().decode() and np.all(out == 7.25)
    assert entry("linearize_robust")(side.tgt.handle, bare.handle, T, side.md, *side.extra, good, 0, out) == capi.PCR_ERR_NO_TARGET
    assert np.all(out == 7.25)


def test_empty_voxel_target_under_a_kernel(g2):
    """The five-point target of test_gpu_vgicp.test_target_with_no_kept_voxel, where set_target accepts it: no voxel, so no
    match whatever the kernel -- 29 zeros from a pass, inf for every point from residuals, and align ends as it ends with
    robust=None."""
    import point_cloud_registration_amd as pcr
    pts, src = np.ascontiguousarray(g2["target"][:5]), g2["source"]

    def ending(reg):
        try:
            return "pose", reg.align(src).tobytes()
        except Exception as exc:                             # noqa: BLE001
            return type(exc).__name__, None

    accepted, ends = [], {}
    for kind in (None,) + rc.KINDS:
        reg = pcr.VGICP(voxel_size=1.0, robust=kind, robust_scale=1.0)
        try:
            reg.set_target(pts)
        except Exception:                                    # noqa: BLE001
            continue
        accepted.append(kind)
        H, g, e2 = reg.calc_H_g_e2(np.eye(4), src)
        assert not H.any() and not g.any() and e2 == 0.0 and reg.last_correspondences == 0, kind
        s = reg.residuals(np.eye(4), src)
        assert s.shape == (len(src),) and np.all(np.isposinf(s)), kind
        ends[kind] = ending(reg)
    print(f"accepted under {accepted}: align ends {ends}")
    assert len(accepted) in (0, 5)
    assert all(e == ends[None] for e in ends.values())


# ----------------------------------------------------------------------------- 6. align on the end-to-end case
def _e2e_reg(name, capi, ctx, case, **kw):
    """(aligner with the case's target and GIVEN payloads on it, keyword arguments of its calc_H_g_e2 / align)."""
    import point_cloud_registration_amd as pcr
    common = dict(max_dist=rc.E2E_MAX_DIST, tol=rc.E2E_TOL, **kw)
    if name == "symm":
        reg = pcr.SymmetricICP(**common)
        reg.set_target(case["target"], norm=case["n_q"])
        return reg, dict(source_normals=case["n_p"])
    if name == "color":
        reg = pcr.ColoredICP(lambda_geometric=rc.E2E_LAMBDA, **common)
        reg.set_target(case["target"], case["I_q"], norm=case["n_q"], gradient=case["g_q"])
        return reg, dict(source_intensity=case["I_p"])
    if name == "gicp":
        reg = pcr.GICP(**common)
        reg.set_target(case["target"], cov=case["Cq"])
        return reg, dict(source_cov=case["Cp"])
    reg = pcr.VGICP(voxel_size=rc.E2E_VOXEL, **common)
    tgt = capi.Target.voxels_from_stats(ctx, case["means"], case["vnorm"], None, rc.E2E_VOXEL)      # the restated voxels
    tgt.set_voxel_covariances(cov=case["Cv"])
    assert np.array_equal(tgt.voxel_stats(("mean",))["mean"], case["means"]) and np.array_equal(tgt.get_voxel_covariances(), case["Cv"])
    reg._set_target_handle(tgt)
    return reg, dict(source_cov=case["Cp"])


@pytest.mark.parametrize("name", ALIGNERS)
def test_align(capi, ctx, case, name):
    """What test_align asserts for the plain pass, under the kernel: the native loop equals the Python loop over calc_H_g_e2
    within 1e-10 with the same iteration count, every trace row is *_linearize_robust at that row's pose bit for bit -- and the
    pose is closer to the truth than robust=None on the same data, within twice the error the restatement recorded."""
    from point_cloud_registration_amd.math_tools import plus
    scan = case["scan"]
    c = rc.E2E_SCALE[name]
    reg, kw = _e2e_reg(name, capi, ctx, case, robust=rc.E2E_KIND, robust_scale=c)
    T = reg.align(scan, **kw)
    iters = reg.last_iterations
    cur, it = np.eye(4), 0
    for it in range(reg.max_iter):
        H, g, _ = reg.calc_H_g_e2(cur, scan, **kw)
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < reg.tol:
            break
        cur = plus(cur, dx)
    assert iters == it + 1 and iters < reg.max_iter
    assert np.max(np.abs(T - cur)) <= 1e-10
    dev = reg._pass_scan(scan, **kw)
    params = reg._pass_params()
    rb = (KIND_ID[rc.E2E_KIND], c)
    T2, iters2, trace = getattr(capi, f"{name}_align_robust")(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, rc.E2E_MAX_DIST, *params,
                                                            robust=rb, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(getattr(capi, f"{name}_linearize_robust")(reg._target, dev, row[:16], rc.E2E_MAX_DIST, *params, robust=rb), row[16:])
    plain, kwp = _e2e_reg(name, capi, ctx, case)
    Tp = plain.align(scan, **kwp)
    ep, er = rc.t_err(Tp, case), rc.t_err(T, case)
    rec_p, rec_r = rc.E2E_ERRORS[name]
    print(f"{name}: plain |dt| {ep:.4e} ({plain.last_iterations} iterations; restated {rec_p:.4e}), "
          f"{rc.E2E_KIND} |dt| {er:.4e} ({iters}; restated {rec_r:.4e})")
    assert er < ep
    assert er <= 2.0 * rec_r
