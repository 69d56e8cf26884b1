"""ColoredICP on the GPU: tangent-plane intensity gradients on a target, the round trips of the payloads, the sums of one pass,
the exact properties of the definition, align, the case the class exists for, and the neighbours it must leave undisturbed.

Fixture: g2_mini_street -- 5000 targets, 2000 scan points, gate 0.8, 1823 kept, non-identity T; no distance within 1e-4 of the
gate and no near-ties, so masks and indices compare exactly; nn_idx / nn_dist are the reference's.  Transformed points come
from orc.transform, which is bit-identical to the kernels' xform.  Target normals are the fixture's plane_normals, the
intensity is color_cases.field everywhere.

Bounds (tests/color_cases.py restates include/pcr.h in float64 NumPy, with its expression order):
  gradients  per component 2^-23 max|g_ref| + 64 cond(M) 2^-53 max|g_ref| against float32(g_ref), on the points with
             cond(M) <= 1e4 -- at least 99 % of them
  sums       per entry (2 n_kept + 16) 2^-53 sum |term| against math.fsum of the restated terms; conftest.step_err <= 1e-10"""

import gc as pygc

import numpy as np
import pytest

import color_cases as cc
import dist_cases as dc
import gicp_cases as gc
from conftest import step_err

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 63, 64, 65, 257)
COLOR_W = 2                                 # points per lane in flight (color.hip)
LAMBDAS = (0.968, 0.5, 0.0, 1.0)


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
    """The street case with colour: (target, scan, T_true, I_target, I_scan) -- the scan's intensity is the field at the truly
    transformed scan."""
    target, scan, T_true = gc.align_case()
    I_q = cc.field(target)
    I_p = cc.field(scan.astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3])
    out = (target, scan, T_true, I_q, I_p)
    for a in out:
        a.setflags(write=False)
    return out


def neighbours(points, k):
    """The GPU's own exact k-NN of every point within its cloud (pinned bit-exact by the k-NN tests); padding = len(points)."""
    import point_cloud_registration_amd as pcr
    return pcr.KDTree(points).query(points, k)[1].reshape(len(points), -1)


def colour_target(capi, ctx, pts, nrm, inten, grad=None, k=None):
    """A point target with normals, intensities and gradients: given, estimated from ``k`` neighbours, or zero."""
    t = capi.Target.points(ctx, np.ascontiguousarray(pts))
    t.set_normals(np.ascontiguousarray(nrm))
    t.set_intensity(inten, grad)
    if k is not None:
        t.estimate_color_gradients(k, want=False)
    return t


def check_gradients(g, ref, cond, what):
    """|g - float32(ref)| within the bound on the well-conditioned points; -> the share compared."""
    assert g.dtype == np.float32 and g.shape == ref.shape and np.all(np.isfinite(g))
    sel = cond <= 1e4
    bound = cc.gradient_bound(ref, cond)
    err = np.max(np.abs(g.astype(np.float64) - ref.astype(np.float32).astype(np.float64)), axis=1)
    pos = sel & (bound > 0)
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    print(f"{what}: compared {sel.mean():.4f}, max err / bound {ratio:.3e}, max|g| {np.abs(ref[sel]).max() if np.any(sel) else 0:.3e}")
    assert np.all(err[sel] <= bound[sel])
    # where the rule makes the gradient zero the kernel agrees exactly
    zero = np.isinf(cond) & np.all(ref == 0, axis=1)
    assert np.array_equal(g[zero], np.zeros((int(zero.sum()), 3), np.float32))
    return float(sel.mean())


# ----------------------------------------------------------------------------- 1. gradients
@pytest.mark.parametrize("k", [10, 20])
def test_gradients(capi, ctx, g2, k):
    tgt, nrm = g2["target"], g2["plane_normals"]
    I = cc.field(tgt)
    t = colour_target(capi, ctx, tgt, nrm, I)
    assert np.array_equal(t.get_color()[1], np.zeros((len(tgt), 3), np.float32))        # zero until estimated
    g = t.estimate_color_gradients(k)
    ref, cond, _ = cc.gradient(tgt, nrm, I, neighbours(tgt, k), full=True)
    assert check_gradients(g, ref, cond, f"k={k}") >= 0.99
    inten, again = t.get_color()
    assert np.array_equal(inten, I) and np.array_equal(again, g)
    # bit for bit: two calls; doubled intensities; a constant intensity; flipped normals
    assert np.array_equal(t.estimate_color_gradients(k), g)
    assert np.array_equal(colour_target(capi, ctx, tgt, nrm, 2 * I).estimate_color_gradients(k), 2 * g)
    const = colour_target(capi, ctx, tgt, nrm, np.full(len(tgt), 0.7, np.float32)).estimate_color_gradients(k)
    assert np.array_equal(const, np.zeros((len(tgt), 3), np.float32))
    flip = np.random.default_rng(3).random(len(tgt)) < 0.5
    assert 0.4 < flip.mean() < 0.6
    assert np.array_equal(colour_target(capi, ctx, tgt, np.where(flip[:, None], -nrm, nrm), I).estimate_color_gradients(k), g)


# ----------------------------------------------------------------------------- 2. gradient edge sizes
def test_gradient_edge_sizes(capi, ctx, g2):
    for n in SIZES:
        pts, nrm = np.ascontiguousarray(g2["target"][:n]), np.ascontiguousarray(g2["plane_normals"][:n])
        I = cc.field(pts)
        g = colour_target(capi, ctx, pts, nrm, I).estimate_color_gradients(10)
        assert g.shape == (n, 3) and np.all(np.isfinite(g))
        if n <= 3:
            assert np.array_equal(g, np.zeros((n, 3), np.float32))
            continue
        nbr = neighbours(pts, 10) if n >= 63 else cc.knn_brute(pts, 10)
        ref, cond, _ = cc.gradient(pts, nrm, I, nbr, full=True)
        check_gradients(g, ref, cond, f"n={n}")
    pts, nrm = np.ascontiguousarray(g2["target"][:64]), np.ascontiguousarray(g2["plane_normals"][:64])
    t = colour_target(capi, ctx, pts, nrm, cc.field(pts))
    # k = 1: every neighbourhood is the point itself
    assert np.array_equal(t.estimate_color_gradients(1), np.zeros((64, 3), np.float32))
    for k in (0, 65):
        with pytest.raises(ValueError):
            t.estimate_color_gradients(k)
    t.estimate_color_gradients(17, want=False)          # (the LDS-list path, without reading back)


# ----------------------------------------------------------------------------- 3. round trips and refusals
def test_scan_intensity_round_trip(capi, ctx, g2):
    src = g2["source"]
    I = np.random.default_rng(0).uniform(0, 1, len(src)).astype(np.float32)
    for flags in (capi.FLAG_KEEP_ORDER, capi.FLAG_NO_SCAN_SORT):
        s = capi.Scan(ctx, src, flags=flags)
        with pytest.raises(ValueError):
            s.get_intensity()                                 # none yet
        s.set_intensity(I)
        assert np.array_equal(s.get_intensity(), I)
        for bad_value in (np.nan, np.inf):
            bad = I.copy()
            bad[1234] = bad_value
            with pytest.raises(ValueError):
                s.set_intensity(bad)
        assert np.array_equal(s.get_intensity(), I)           # a refused set leaves the old ones
        with pytest.raises(ValueError):
            s.set_intensity(I[:-1])
        # intensities, normals and covariances coexist
        s.estimate_normals(10, want=False)
        s.estimate_covariances(10, want=False)
        assert np.array_equal(s.get_intensity(), I)
    plain = capi.Scan(ctx, src)
    with pytest.raises(ValueError):
        plain.set_intensity(I)
    empty = capi.Scan(ctx, src[:0], flags=capi.FLAG_KEEP_ORDER)
    empty.set_intensity(np.zeros(0, np.float32))
    assert empty.get_intensity().shape == (0,)


def test_target_colour_round_trip(capi, ctx, g2):
    tgt, nrm = g2["target"], g2["plane_normals"]
    I = cc.field(tgt)
    G = (0.3 * np.random.default_rng(1).normal(size=(len(tgt), 3))).astype(np.float32)
    bare = capi.Target.points(ctx, tgt)
    with pytest.raises(ValueError):
        bare.set_intensity(I)                                 # no normals
    with pytest.raises(ValueError):
        bare.get_color()
    t = colour_target(capi, ctx, tgt, nrm, I, G)
    inten, grad = t.get_color()
    assert np.array_equal(inten, I) and np.array_equal(grad, G)
    for bad_value in (np.nan, np.inf):
        bad = I.copy()
        bad[77] = bad_value
        with pytest.raises(ValueError):
            t.set_intensity(bad, G)
        badg = G.copy()
        badg[77, 2] = bad_value
        with pytest.raises(ValueError):
            t.set_intensity(I, badg)
    with pytest.raises(ValueError):
        t.set_intensity(I[:-1])
    inten, grad = t.get_color()
    assert np.array_equal(inten, I) and np.array_equal(grad, G)          # refused sets left the old payload
    t.set_intensity(2 * I)                                               # without gradients: zero until estimated
    inten, grad = t.get_color()
    assert np.array_equal(inten, 2 * I) and np.array_equal(grad, np.zeros_like(G))
    nocol = capi.Target.points(ctx, tgt)
    nocol.set_normals(nrm)
    with pytest.raises(ValueError):
        nocol.estimate_color_gradients(10)                    # needs intensities
    vox = capi.Target.voxels(ctx, tgt.astype(np.float64), float(g2["voxel_size"]))
    with pytest.raises(ValueError):
        vox.set_intensity(np.zeros(vox.size(), np.float32))


def test_pass_refusals(capi, ctx, g2):
    T, md, tgt, nrm = g2["T"], float(g2["max_dist"]), g2["target"], g2["plane_normals"]
    I = cc.field(tgt)
    s = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER)
    good = colour_target(capi, ctx, tgt, nrm, I, k=10)
    with pytest.raises(ValueError, match="scan has no intensities"):
        capi.color_linearize(good, s, T, md)
    s.set_intensity(cc.field(g2["source"]))
    assert capi.color_linearize(good, s, T, md)[28] == 1823
    vox = capi.Target.voxels(ctx, tgt.astype(np.float64), float(g2["voxel_size"]))
    with pytest.raises(ValueError, match="point target"):
        capi.color_linearize(vox, s, T, md)
    with pytest.raises(ValueError, match="no normals"):
        capi.color_linearize(capi.Target.points(ctx, tgt), s, T, md)
    nocol = capi.Target.points(ctx, tgt)
    nocol.set_normals(nrm)
    with pytest.raises(ValueError, match="no colour records"):
        capi.color_linearize(nocol, s, T, md)
    with pytest.raises(ValueError):
        capi.color_align(nocol, s, T, 5, 1e-3, md)
    # replacing the normals frees the colour records: refused, not stale
    for replace in (lambda t: t.set_normals(nrm), lambda t: t.estimate_normals(10, compat=False, want=False)):
        t = colour_target(capi, ctx, tgt, nrm, I, k=10)
        replace(t)
        with pytest.raises(ValueError, match="no colour records"):
            capi.color_linearize(t, s, T, md)
        with pytest.raises(ValueError):
            t.get_color()
        t.set_intensity(I)                                    # ... and can be set again
        assert capi.color_linearize(t, s, T, md)[28] == 1823
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            capi.color_linearize(good, s, T, md, lam)
        with pytest.raises(ValueError):
            capi.color_align(good, s, T, 5, 1e-3, md, lam)


# ----------------------------------------------------------------------------- 4. sums, kernel only
@pytest.fixture(scope="module")
def coloursets(capi, ctx, g2, orc):
    """Given gradients and scan intensities, so the sums do not depend on test 1.  Gradients: "random" = 0.3 normal(size =
    (5000, 3)) from default_rng(1), deliberately not tangent; "estimated" = the GPU's, k = 10, read back.  Scan intensities:
    "random" = uniform(0, 1) from default_rng(0); "field" = the field at the transformed scan.  Computed once, never modified."""
    tgt, src = g2["target"], g2["source"]
    I_q = cc.field(tgt)
    out = {"I_q": I_q,
           "G": {"random": (0.3 * np.random.default_rng(1).normal(size=(5000, 3))).astype(np.float32),
                 "estimated": colour_target(capi, ctx, tgt, g2["plane_normals"], I_q).estimate_color_gradients(10)},
           "I_p": {"random": np.random.default_rng(0).uniform(0, 1, 2000).astype(np.float32),
                   "field": cc.field(orc.transform(g2["T"], src))}}
    for a in (I_q, *out["G"].values(), *out["I_p"].values()):
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def restated(g2, orc, coloursets):
    """restated(gname, iname, lam) -> (terms (2 N, 28), mask): the definition at g2's pose from the GOLDEN correspondences."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    tp = orc.transform(T, src)
    cache = {}

    def get(gname, iname, lam, G=None, I_q=None, I_p=None):
        key = (gname, iname, lam)
        if key not in cache:
            G_ = coloursets["G"][gname] if G is None else G
            Iq_ = coloursets["I_q"] if I_q is None else I_q
            Ip_ = coloursets["I_p"][iname] if I_p is None else I_p
            t = cc.terms(T, src, tp, tgt[j], g2["plane_normals"][j], Iq_[j], G_[j], Ip_, mask, lam)
            t.setflags(write=False)
            cache[key] = t
        return cache[key], mask
    return get


def gpu_sums(capi, ctx, g2, coloursets, gname, iname, lam, n=None, flags=None, max_dist=None, nq=None):
    n = 2000 if n is None else n
    t = colour_target(capi, ctx, g2["target"], g2["plane_normals"] if nq is None else nq, coloursets["I_q"], coloursets["G"][gname])
    s = capi.Scan(ctx, np.ascontiguousarray(g2["source"][:n]), flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    s.set_intensity(np.ascontiguousarray(coloursets["I_p"][iname][:n]))
    md = float(g2["max_dist"]) if max_dist is None else max_dist
    return capi.color_linearize(t, s, g2["T"], md, lam), t, s


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("iname", ["random", "field"])
@pytest.mark.parametrize("gname", ["random", "estimated"])
def test_sums(capi, ctx, g2, coloursets, restated, gname, iname, lam):
    out, t, s = gpu_sums(capi, ctx, g2, coloursets, gname, iname, lam)
    ref, bound, kept = cc.reference(*restated(gname, iname, lam))
    assert kept == 1823 and out[28] == kept
    err = np.abs(out[:28] - ref)
    pos = bound > 0
    print(f"{gname} / {iname} / {lam}: max err / bound {np.max(err[pos] / bound[pos]):.3e}, "
          f"bound / max|H| {bound[:21].max() / np.abs(ref[:21]).max():.3e}")
    assert np.all(err <= bound)
    H, g, _ = cc.unpack28(out[:28])
    Href, gref, _ = cc.unpack28(ref)
    if np.linalg.cond(Href) < 1e12:
        se = step_err(H, g, Href, gref)
        print(f"{gname} / {iname} / {lam}: step error {se:.3e}")
        assert se <= 1e-10
    else:
        print(f"{gname} / {iname} / {lam}: H is singular to rounding (cond {np.linalg.cond(Href):.1e}): no step to compare")
        assert lam == 0.0
    # two consecutive calls return the same bits
    assert np.array_equal(out, capi.color_linearize(t, s, g2["T"], float(g2["max_dist"]), lam))
    # the scan in the caller's order on the device
    nosort = gpu_sums(capi, ctx, g2, coloursets, gname, iname, lam, flags=capi.FLAG_NO_SCAN_SORT)[0]
    assert nosort[28] == kept and np.all(np.abs(nosort[:28] - ref) <= bound)


# ----------------------------------------------------------------------------- 5. prefixes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_sums_prefixes(capi, ctx, g2, coloursets, restated, n):
    """Correspondences of a subset of the scan are a subset of g2's."""
    for gname, iname in (("random", "random"), ("estimated", "field")):
        out = gpu_sums(capi, ctx, g2, coloursets, gname, iname, 0.968, n=n)[0]
        ref, bound, kept = cc.prefix(*restated(gname, iname, 0.968), n)
        assert out[28] == kept
        assert np.all(np.abs(out[:28] - ref) <= bound)
        if n == 0:
            assert np.array_equal(out, np.zeros(29))


# ----------------------------------------------------------------------------- 6. more than one trip of the grid
def test_grid_rule_on_this_device(cus):
    """The sizes below make slots and trips live only while the reduce grid is 8 blocks per CU."""
    assert dc.stride_points(cus) == 524288, cus


@pytest.mark.parametrize("order", ["keep_order", "no_scan_sort"])
@pytest.mark.parametrize("k", range(COLOR_W))
def test_live_slots(capi, ctx, cus, g2, coloursets, restated, k, order):
    """Sizes stride + 257 and 2 stride + 513: slot 1, then the second trip carry live points."""
    n = dc.big_sizes(cus, COLOR_W)[k]
    ref, bound, count = cc.tiled(*restated("random", "random", 0.968), n)
    tgt = colour_target(capi, ctx, g2["target"], g2["plane_normals"], coloursets["I_q"], coloursets["G"]["random"])
    s = capi.Scan(ctx, dc.tile_rows(g2["source"], n), flags=capi.FLAG_KEEP_ORDER if order == "keep_order" else capi.FLAG_NO_SCAN_SORT)
    try:
        s.set_intensity(dc.tile_rows(coloursets["I_p"]["random"], n))
        out = capi.color_linearize(tgt, s, g2["T"], float(g2["max_dist"]), 0.968)
        err = np.abs(out[:28] - ref)
        print(f"n {n} {order}: kept {count}, max err / bound {np.max(err / bound):.3e}")
        assert out[28] == count and 0 < count < n
        assert np.all(err <= bound)
        H, g, _ = cc.unpack28(out[:28])
        Href, gref, _ = cc.unpack28(ref)
        assert step_err(H, g, Href, gref) <= 1e-10
        assert np.array_equal(capi.color_linearize(tgt, s, g2["T"], float(g2["max_dist"]), 0.968), out)
    finally:
        s.close()


# ----------------------------------------------------------------------------- 7. exact properties
def test_normal_sign_invariance(capi, ctx, g2, coloursets):
    nq = g2["plane_normals"]
    flip = np.random.default_rng(7).random(len(nq)) < 0.5
    assert 0.4 < flip.mean() < 0.6
    for gname in ("random", "estimated"):
        out = gpu_sums(capi, ctx, g2, coloursets, gname, "field", 0.968)[0]
        assert np.array_equal(gpu_sums(capi, ctx, g2, coloursets, gname, "field", 0.968, nq=np.where(flip[:, None], -nq, nq))[0], out)
        assert np.array_equal(gpu_sums(capi, ctx, g2, coloursets, gname, "field", 0.968, nq=-nq)[0], out)


def test_lambda_one_is_plane_icp(capi, ctx, g2, coloursets, restated):
    import point_cloud_registration_amd as pcr
    T, md, tgt, nrm = g2["T"], float(g2["max_dist"]), g2["target"], g2["plane_normals"]
    out = gpu_sums(capi, ctx, g2, coloursets, "random", "random", 1.0)[0]
    # the same call with all gradients zero and other scan intensities: the same bits
    zero = colour_target(capi, ctx, tgt, nrm, coloursets["I_q"])
    s = capi.Scan(ctx, g2["source"], flags=capi.FLAG_KEEP_ORDER)
    s.set_intensity(coloursets["I_p"]["field"])
    assert np.array_equal(capi.color_linearize(zero, s, T, md, 1.0), out)
    # PlaneICP on the same target and normals, within the sum bound
    ref, bound, kept = cc.reference(*restated("random", "random", 1.0))
    plane = pcr.PlaneICP(max_dist=md)
    plane.set_target(tgt, kdree=object(), norm=nrm)
    H, g, e2 = plane.calc_H_g_e2(T, g2["source"])
    err = np.abs(np.concatenate([H[cc.TRIU], g, [e2]]) - out[:28])
    print(f"lambda = 1 against PlaneICP: max err / bound {np.max(err / bound):.3e}")
    assert plane.last_correspondences == kept == out[28] and np.all(err <= bound)


def test_constant_intensity_scales_plane_icp(capi, ctx, g2, orc):
    """Constant intensity on both clouds: the estimated gradients are zero, r_C = 0, and the sums are lambda x the geometric
    ones up to the rounding of sqrt(lambda)^2 -- inside the sum bound."""
    T, md, tgt, nrm, src = g2["T"], float(g2["max_dist"]), g2["target"], g2["plane_normals"], g2["source"]
    lam = 0.968
    t = colour_target(capi, ctx, tgt, nrm, np.full(len(tgt), 0.5, np.float32), k=10)
    assert np.array_equal(t.get_color()[1], np.zeros((len(tgt), 3), np.float32))
    s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    s.set_intensity(np.full(len(src), 0.5, np.float32))
    one, out = capi.color_linearize(t, s, T, md, 1.0), capi.color_linearize(t, s, T, md, lam)
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(md)
    terms = cc.terms(T, src, orc.transform(T, src), tgt[j], nrm[j], np.full(len(src), 0.5, np.float32), np.zeros((len(src), 3), np.float32),
                     np.full(len(src), 0.5, np.float32), mask, lam)
    _, bound, kept = cc.reference(terms, mask)
    err = np.abs(out[:28] - lam * one[:28])
    print(f"constant intensity: max err / bound {np.max(err / bound):.3e}")
    assert out[28] == one[28] == kept and np.all(err <= bound)


# ----------------------------------------------------------------------------- 8. gates
def test_nothing_inside_the_gate(capi, ctx, g2, coloursets):
    import point_cloud_registration_amd as pcr
    assert np.array_equal(gpu_sums(capi, ctx, g2, coloursets, "random", "random", 0.968, max_dist=1e-6)[0], np.zeros(29))
    reg = pcr.ColoredICP(max_dist=1e-6)
    reg.set_target(g2["target"], coloursets["I_q"], norm=g2["plane_normals"])
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(g2["source"], coloursets["I_p"]["field"], init_T=g2["T"])


def test_gate(case, orc):
    """T = I, max_dist = 0.1: 45.2 % kept, none within 1e-3 relative of the gate: the count equals the restated mask."""
    import point_cloud_registration_amd as pcr
    target, scan, _, I_q, I_p = case
    reg = pcr.ColoredICP(max_dist=0.1, k=10)
    reg.set_target(target, I_q)
    dist = reg.kdtree.query(orc.transform(np.eye(4), scan))[0]
    assert np.min(np.abs(dist / np.float32(0.1) - 1.0)) > 1e-3
    kept = int((dist < np.float32(0.1)).sum())
    assert abs(kept / len(scan) - 0.452) < 0.005, kept / len(scan)
    reg.calc_H_g_e2(np.eye(4), scan, I_p)
    assert reg.last_correspondences == kept


# ----------------------------------------------------------------------------- 9. align
@pytest.mark.parametrize("max_dist", [2.0, 0.15])
def test_align(capi, case, max_dist):
    import point_cloud_registration_amd as pcr
    from point_cloud_registration_amd.math_tools import plus
    target, scan, T_true, I_q, I_p = case
    reg = pcr.ColoredICP(max_dist=max_dist, k=10, tol=1e-4)
    reg.set_target(target, I_q)
    assert reg.normal.shape == (len(target), 3) and reg.gradient.shape == (len(target), 3) and np.array_equal(reg.intensity, I_q)
    T = reg.align(scan, I_p)
    iters = reg.last_iterations
    dR, dt = np.linalg.norm(T[:3, :3] - T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])
    print(f"max_dist {max_dist}: {iters} iterations, |dR|_F {dR:.3e}, |dt| {dt:.3e}")
    assert dR < 5e-4 and dt < 5e-4
    # the same loop in the test: calc_H_g_e2 + solve + plus
    cur, it = np.eye(4), 0
    for it in range(reg.max_iter):
        H, g, _ = reg.calc_H_g_e2(cur, scan, I_p)
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < reg.tol:
            break
        cur = plus(cur, dx)
    assert iters == it + 1
    assert np.max(np.abs(T - cur)) <= 1e-10
    # the per-point host loop over the GPU's correspondences agrees with the kernel to the rounding of its own weights
    Hk, gk, ek = reg.calc_H_g_e2(T, scan, I_p)
    Hl, gl, el = reg.calc_H_g_e2_no_parallel_ver(T, scan, I_p)
    assert np.max(np.abs(Hl - Hk)) <= 1e-9 * np.max(np.abs(Hk)) and np.max(np.abs(gl - gk)) <= 1e-9 * np.max(np.abs(Hk)) \
        and abs(el - ek) <= 1e-9 * ek
    # the Python loop of the class
    slow = pcr.ColoredICP(max_dist=max_dist, k=10, tol=1e-4, native_loop=False)
    slow.set_target(target, I_q)
    assert np.max(np.abs(slow.align(scan, I_p) - T)) <= 1e-10 and slow.last_iterations == iters
    # every trace row's sums are the bits pcr_color_linearize returns at that row's pose
    dev = reg._color_scan(scan, I_p)
    lam = reg.lambda_geometric
    T2, iters2, trace = capi.color_align(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, max_dist, lam, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45)
    for row in trace:
        assert np.array_equal(capi.color_linearize(reg._target, dev, row[:16], max_dist, lam), row[16:])
    # max_iter = 0 returns init_T
    T0 = plus(np.eye(4), np.array([0.01, 0.02, 0.03, 0.001, 0.002, 0.003]))
    reg0 = pcr.ColoredICP(max_dist=max_dist, k=10, max_iter=0)
    reg0.set_target(target, I_q)
    assert np.array_equal(reg0.align(scan, I_p, init_T=T0), T0) and reg0.last_iterations == 0


# ----------------------------------------------------------------------------- 10. what the feature is for
def test_sliding_plane(capi):
    """A flat, textured target and a scan shifted inside the plane: geometry alone cannot see the shift, colour can."""
    import point_cloud_registration_amd as pcr
    P, nrm, I, src, I_src = cc.plane_case()
    flat = pcr.ColoredICP(max_dist=0.2, tol=1e-6, k=10, lambda_geometric=1.0)
    flat.set_target(P, I, norm=nrm)
    H1 = flat.calc_H_g_e2(np.eye(4), src, I_src)[0]
    assert np.linalg.matrix_rank(H1) == 3
    for c in (0, 1, 5):
        assert np.array_equal(H1[:, c], np.zeros(6)) and np.array_equal(H1[c, :], np.zeros(6))
    reg = pcr.ColoredICP(max_dist=0.2, tol=1e-6, k=10, lambda_geometric=0.968)
    reg.set_target(P, I, norm=nrm)
    assert np.linalg.matrix_rank(reg.calc_H_g_e2(np.eye(4), src, I_src)[0]) == 6
    T = reg.align(src, I_src)
    dt, dR = np.linalg.norm(T[:3, 3] - cc.PLANE_SHIFT), np.linalg.norm(T[:3, :3] - np.eye(3))
    print(f"ColoredICP: {reg.last_iterations} iterations, |t - shift| {dt:.3e}, |R - I|_F {dR:.3e}")
    assert dt < 1e-4 and dR < 1e-4
    plane = pcr.PlaneICP(max_dist=0.2, tol=1e-6)
    plane.set_target(P, kdree=object(), norm=nrm)
    try:
        Tp = plane.align(src)
    except np.linalg.LinAlgError:
        print("PlaneICP: LinAlgError")
    else:
        miss = np.linalg.norm(Tp[:3, 3] - cc.PLANE_SHIFT)
        print(f"PlaneICP: misses the shift by {miss:.3e}")
        assert miss > 1e-2


# ----------------------------------------------------------------------------- 11. neighbours undisturbed
def test_neighbours_undisturbed(capi, ctx, g2):
    """ICP / PlaneICP / GICP / SymmetricICP return the same bits before and after a coloured pass: over one context and the
    same scan array, and over the very same device scan -- one that carries covariances, normals AND intensities."""
    import point_cloud_registration_amd as pcr
    T, src, tgt, md = g2["T"], g2["source"], g2["target"], float(g2["max_dist"])
    I_q, I_p = cc.field(tgt), cc.field(src)
    icp, plane, gicp = pcr.ICP(max_dist=md), pcr.PlaneICP(max_dist=md), pcr.GICP(max_dist=md)
    symm, color = pcr.SymmetricICP(max_dist=md), pcr.ColoredICP(max_dist=md)
    icp.set_target(tgt)
    plane.set_target(tgt, kdree=object(), norm=g2["plane_normals"])
    gicp.set_target(tgt)
    symm.set_target(tgt, norm=g2["plane_normals"])
    color.set_target(tgt, I_q, norm=g2["plane_normals"])
    for variant in (2, 1):
        with ctx.pipeline(variant=variant):
            before = [reg.calc_H_g_e2(T, src) for reg in (icp, plane, gicp, symm)]
            first = color.calc_H_g_e2(T, src, I_p)
            after = [reg.calc_H_g_e2(T, src) for reg in (icp, plane, gicp, symm)]
            for b, a in zip(before, after):
                assert all(np.array_equal(x, y) for x, y in zip(b, a))
            assert all(np.array_equal(x, y) for x, y in zip(first, color.calc_H_g_e2(T, src, I_p)))
            s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
            s.estimate_covariances(10, want=False)
            s.estimate_normals(10, want=False)
            s.set_intensity(I_p)
            o1 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g1 = capi.gicp_linearize(gicp._target, s, T, md)
            s1 = capi.symm_linearize(symm._target, s, T, md)
            c1 = capi.color_linearize(color._target, s, T, md)
            o2 = capi.linearize(icp._target, s, capi.ICP, T, md)
            g2_ = capi.gicp_linearize(gicp._target, s, T, md)
            s2 = capi.symm_linearize(symm._target, s, T, md)
            c2 = capi.color_linearize(color._target, s, T, md)
            assert np.array_equal(o1, o2) and np.array_equal(g1, g2_) and np.array_equal(s1, s2) and np.array_equal(c1, c2)
            assert g1[28] == o1[28] == s1[28] == c1[28] == 1823


# ----------------------------------------------------------------------------- 12. the call's parameter decides
def test_lambda_belongs_to_the_call(capi, ctx, g2):
    """Three calls over ONE uploaded scan, lambda = 1, 0.5, 1: the first and the third return the same bits -- PlaneICP's sums
    on the same pair, within the sum bound of test_lambda_one_is_plane_icp -- and the second other sums over the same pairs:
    the weights are parameters of the call, nothing an earlier call leaves on the scan."""
    import point_cloud_registration_amd as pcr
    import symm_cases as sc
    tgt, nq, src, tp, j, mask = sc.call_case(g2)
    T, md = g2["T"], sc.CALL_MAX_DIST
    I_q = cc.field(tgt)
    G = (0.3 * np.random.default_rng(1).normal(size=(len(tgt), 3))).astype(np.float32)
    I_p = np.random.default_rng(0).uniform(0, 1, len(src)).astype(np.float32)
    s = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    s.set_intensity(I_p)
    t = colour_target(capi, ctx, tgt, nq, I_q, G)
    first, second, third = (capi.color_linearize(t, s, T, md, lam) for lam in (1.0, 0.5, 1.0))
    assert np.array_equal(first, third)
    assert second[28] == first[28] == mask.sum() == 216 and not np.array_equal(second[:28], first[:28])
    ref, bound, kept = cc.reference(cc.terms(T, src, tp, tgt[j], nq[j], I_q[j], G[j], I_p, mask, 1.0), mask)
    plane = pcr.PlaneICP(max_dist=md)
    plane.set_target(tgt, kdree=object(), norm=nq)
    H, g, e2 = plane.calc_H_g_e2(T, src)
    err = np.abs(np.concatenate([H[cc.TRIU], g, [e2]]) - first[:28])
    print(f"lambda = 1 against PlaneICP: max err / bound {np.max(err / bound):.3e}")
    assert plane.last_correspondences == kept == first[28] and np.all(err <= bound)


# ----------------------------------------------------------------------------- 13. device memory
def test_align_device_memory_is_stable(capi, ctx, case):
    import torch
    import point_cloud_registration_amd as pcr
    target, scan, _, I_q, I_p = case
    reg = pcr.ColoredICP(max_dist=2.0, k=10)
    reg.set_target(target, I_q)
    first = reg.align(scan, I_p); pygc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        last = reg.align(scan, I_p)
    pygc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
    assert np.array_equal(first, last)
