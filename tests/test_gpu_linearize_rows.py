"""linearize (per-point rows), weighted calc_H_g_e2 and scan coresets on the GPU, on g2_mini_street (5000 targets, 2000 scan
points, gate 0.8, non-identity T; pinned to the reference).  g2 has no near-ties (smallest gap between first and second
neighbour 1.4e-5 m for points, 8.6e-5 m for centroids; no distance within 1e-4 of the gate), so every comparison of indices
and masks is exact and over every point.

Tolerances.  Values (test 2): every entry within 4 * 2^-53 * sum |products of that entry| of a float64 NumPy restatement in
the kernels' expression order (the build has -ffp-contract=off: only association and explicit fma can differ).  Sums (tests
3 and 5): n * 2^-53 * sum_i |term_i| per entry, the classical bound on the pass's own summation of n terms, against the
exactly rounded (math.fsum) sums of the rows.  Coreset (test 6): the per-row error of tests/coreset_cases.py, bound 10 x the
largest figure g15 records for the reference on its M = 28 cases."""

import math

import numpy as np
import pytest

import coreset_cases as cc
from conftest import PIPELINES, load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NAMES = ["icp", "plane", "vplane", "ndt"]
TRIU = np.triu_indices(6)


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
def regs(capi, g2):
    """The four classes over g2's target.  The voxel targets are built from g2's own statistics, so a voxel's position is
    its row in g2["vox_mean"] (what g2["vox_idx"] counts in)."""
    import point_cloud_registration_amd as pcr
    ctx = capi.get_context(0)
    md, vs = float(g2["max_dist"]), float(g2["voxel_size"])
    out = {"icp": pcr.ICP(max_dist=md), "plane": pcr.PlaneICP(max_dist=md), "vplane": pcr.VPlaneICP(voxel_size=vs, max_dist=md),
           "ndt": pcr.NDT(voxel_size=vs, max_dist=md)}
    out["icp"].set_target(g2["target"])
    out["plane"].set_target(g2["target"], kdree=object(), norm=g2["plane_normals"])
    out["vplane"]._set_target_handle(capi.Target.voxels_from_stats(ctx, g2["vox_mean"], g2["vox_norm"], g2["vox_icov"], vs))
    out["ndt"]._set_target_handle(capi.Target.voxels_from_stats(ctx, g2["vox_mean"], g2["vox_norm"], g2["vox_icov"], vs))
    return out


def golden_match(g2, name):
    """(idx, mask) of the reference: nn_idx / vox_idx where the golden distance is inside the gate, -1 elsewhere."""
    point = name in ("icp", "plane")
    mask = (g2["nn_dist"] if point else g2["vox_dist"]) < float(g2["max_dist"])
    return np.where(mask, g2["nn_idx"] if point else g2["vox_idx"], -1), mask


@pytest.fixture(scope="module")
def rows(regs, g2):
    """linearize(T, source, return_index=True) of every class: computed once, shared, never modified."""
    out = {}
    for name in NAMES:
        out[name] = regs[name].linearize(g2["T"], g2["source"], return_index=True)
        for a in out[name]:
            a.setflags(write=False)
    return out


def restate(orc, g2, name):
    """(J, r, W, bound_J, bound_r): float64 NumPy restatement of acc_plane / acc_ndt's expressions from the GOLDEN indices,
    with sum |products| of every entry.  Rows of gated-out points are zero."""
    T, src = g2["T"], g2["source"]
    idx, mask = golden_match(g2, name)
    j = np.where(mask, idx, 0)
    R = T[:3, :3].astype(np.float64)
    tp = orc.transform(T, src)                                    # float32, bit-equal to the kernels' xform by construction
    x, y, z = (src[:, k].astype(np.float64) for k in range(3))
    if name in ("icp", "plane"):
        d = (tp - g2["target"][j]).astype(np.float64)             # float32 subtraction, as the kernels do it
    else:
        d = tp.astype(np.float64) - g2["vox_mean"][j]
    n = len(src)
    W = None
    if name in ("plane", "vplane"):
        nrm = (g2["plane_normals"][j] if name == "plane" else g2["vox_norm"][j]).astype(np.float64)
        n0, n1, n2 = nrm.T
        r = ((n0 * d[:, 0] + n1 * d[:, 1]) + n2 * d[:, 2])[:, None]
        br = (np.abs(n0 * d[:, 0]) + np.abs(n1 * d[:, 1]) + np.abs(n2 * d[:, 2]))[:, None]
        ta = R[0, 0] * n0 + R[1, 0] * n1 + R[2, 0] * n2
        tb = R[0, 1] * n0 + R[1, 1] * n1 + R[2, 1] * n2
        tc = R[0, 2] * n0 + R[1, 2] * n1 + R[2, 2] * n2
        aa, ab, ac = (np.abs(R[0, c] * n0) + np.abs(R[1, c] * n1) + np.abs(R[2, c] * n2) for c in range(3))
        J = np.stack([n0, n1, n2, -z * tb + y * tc, z * ta - x * tc, -y * ta + x * tb], axis=1)[:, None, :]
        bJ = np.stack([np.abs(n0), np.abs(n1), np.abs(n2), np.abs(z) * ab + np.abs(y) * ac, np.abs(z) * aa + np.abs(x) * ac,
                       np.abs(y) * aa + np.abs(x) * ab], axis=1)[:, None, :]
    else:
        J, bJ = np.zeros((n, 3, 6)), np.zeros((n, 3, 6))
        for i in range(3):
            r0, r1, r2 = R[i]
            J[:, i, i] = 1.0
            bJ[:, i, i] = 1.0
            J[:, i, 3] = -(r1 * z - r2 * y)
            J[:, i, 4] = -(-r0 * z + r2 * x)
            J[:, i, 5] = -(r0 * y - r1 * x)
            bJ[:, i, 3] = np.abs(r1 * z) + np.abs(r2 * y)
            bJ[:, i, 4] = np.abs(r0 * z) + np.abs(r2 * x)
            bJ[:, i, 5] = np.abs(r0 * y) + np.abs(r1 * x)
        r, br = d.copy(), np.abs(d)
        if name == "ndt":
            W = g2["vox_icov"][j] * mask[:, None, None]
    J, r, bJ, br = (a * mask.reshape((n,) + (1,) * (a.ndim - 1)) for a in (J, r, bJ, br))
    return J, r, W, bJ, br


def fsum_cols(terms):
    """Exactly rounded sum over axis 0 of terms (n, k) and sum |terms|."""
    t = terms.reshape(terms.shape[0], -1)
    return (np.array([math.fsum(t[:, c]) for c in range(t.shape[1])]).reshape(terms.shape[1:]),
            np.abs(t).sum(axis=0).reshape(terms.shape[1:]))


def row_sums(J, r, ws, weights=None):
    """(H, g, e2) and their sum |term| from rows, exactly rounded; ws (N,) or (N, 3, 3); optional per-point weights."""
    if ws.ndim == 1:
        WJ = ws[:, None, None] * J
        Wr = ws[:, None] * r
    else:
        WJ = np.einsum("nik,nkl->nil", ws, J)
        Wr = np.einsum("nik,nk->ni", ws, r)
    tH = np.einsum("nij,nil->njl", J, WJ)
    tg = np.einsum("nij,ni->nj", J, Wr)
    te = np.einsum("ni,ni->n", r, Wr)[:, None]
    if weights is not None:
        tH, tg, te = tH * weights[:, None, None], tg * weights[:, None], te * weights[:, None]
    (H, aH), (g, ag), (e, ae) = fsum_cols(tH), fsum_cols(tg), fsum_cols(te)
    return (H, g, float(e[0])), (aH, ag, float(ae[0]))


def assert_sums(got, want, mags, n, tag):
    for what, a, b, m in zip(("H", "g", "e2"), got, want, mags):
        err, bound = np.abs(np.asarray(a) - np.asarray(b)), n * EPS * np.asarray(m)
        print(f"{tag} {what}: max |delta| {err.max():.3e}, max delta / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), (tag, what, float(err.max()))


# ----------------------------------------------------------------------------- 1. indices and mask
@pytest.mark.parametrize("name", NAMES)
def test_indices_and_mask(regs, rows, g2, name):
    J, r, ws, idx = rows[name]
    want_idx, mask = golden_match(g2, name)
    n = len(g2["source"])
    assert int(mask.sum()) == (1823 if name in ("icp", "plane") else 1785)
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx)
    m = 1 if name in ("plane", "vplane") else 3
    assert J.shape == (n, m, 6) and r.shape == (n, m) and J.dtype == r.dtype == ws.dtype == np.float64
    if name == "ndt":
        assert ws.shape == (n, 3, 3) and np.array_equal(np.any(ws != 0, axis=(1, 2)), mask)
    else:
        assert ws.shape == (n,) and np.array_equal(ws, mask.astype(np.float64))
    assert not J[~mask].any() and not r[~mask].any()
    assert len(regs[name].linearize(g2["T"], g2["source"])) == 3


# ----------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("name", NAMES)
def test_values(rows, orc, g2, name):
    J, r, ws, idx = rows[name]
    Jn, rn, Wn, bJ, br = restate(orc, g2, name)
    eJ, er = np.abs(J - Jn), np.abs(r - rn)
    print(f"{name}: max |J - J_numpy| {eJ.max():.3e}, max |r - r_numpy| {er.max():.3e}")
    assert np.all(eJ <= 4 * EPS * bJ) and np.all(er <= 4 * EPS * br)
    if name == "ndt":
        assert np.allclose(ws, Wn, rtol=1e-12, atol=0)
        assert np.array_equal(ws, np.swapaxes(ws, 1, 2))


# ----------------------------------------------------------------------------- 3. rows against sums
@pytest.mark.parametrize("name", NAMES)
def test_rows_against_sums(regs, rows, g2, name):
    reg = regs[name]
    J, r, ws, idx = rows[name]
    n = len(r)
    (H, g, e2), mags = row_sums(J, r, ws)
    if name != "icp":
        assert_sums(reg.calc_H_g_e2(g2["T"], g2["source"]), (H, g, e2), mags, n, name)
        return
    import point_cloud_registration_amd as pcr
    plain = pcr.ICP(max_dist=float(g2["max_dist"]), compat_flags=0)
    plain._set_target_handle(reg._target)
    try:
        assert_sums(plain.calc_H_g_e2(g2["T"], g2["source"]), (H, g, e2), mags, n, "icp flags 0")
    finally:
        plain._target = None                    # (borrowed handle)
    Hq, gq, e2q = reg.calc_H_g_e2(g2["T"], g2["source"])
    # quirk Q1: H, g[:3] and e2 are the rows' sums; g[3:] = sum p x (R r), computed from the rows
    R, p = g2["T"][:3, :3], g2["source"].astype(np.float64)
    gq3, _ = fsum_cols(np.cross(p, r @ R.T) * ws[:, None])
    ap, ar = np.abs(p), np.abs(r) @ np.abs(R).T
    aq3 = ((ap[:, [1, 2, 0]] * ar[:, [2, 0, 1]] + ap[:, [2, 0, 1]] * ar[:, [1, 2, 0]]) * ws[:, None]).sum(0)
    gw, mg = g.copy(), mags[1].copy()
    gw[3:], mg[3:] = gq3, aq3
    assert_sums((Hq, gq, e2q), (H, gw, e2), (mags[0], mg, mags[2]), n, "icp quirk")


# ----------------------------------------------------------------------------- 3b. terms against rows
@pytest.mark.parametrize("name", NAMES)
def test_terms_are_products_of_the_rows(regs, g2, name):
    """The rows and the terms of a point come from one definition: calc_H_g_e2 with a one-hot weight (the fixed-order sum is
    then fma(1, P, 0) plus zeros: the point's own terms, exactly) equals the products of linearize's row of that point, each
    rounded once -- `==` throughout, which takes -0.0 for +0.0.  65 points: one full wave and a tail through the two-in-flight
    loop.  Every one of g2's first 65 points has a correspondence, so point 40 of the copy is lifted 50 m off the street:
    the gated-out point, all of whose 29 outputs are zero.  (Written without a GPU at hand: not yet run on hardware.)"""
    import point_cloud_registration_amd as pcr
    T = g2["T"]
    src = np.ascontiguousarray(g2["source"][:65]).copy()
    src[40, 2] += 50.0
    reg = regs[name]
    if name == "icp":                                   # the rows are J = [I, A], r: the flag-0 sums (Q1 changes g[3:] only)
        reg = pcr.ICP(max_dist=float(g2["max_dist"]), compat_flags=0)
        reg._set_target_handle(regs[name]._target)
    try:
        J, r, ws, idx = reg.linearize(T, src, return_index=True)
        mask = idx >= 0
        assert np.array_equal(np.flatnonzero(~mask), [40])
        inside = np.flatnonzero(mask)
        chosen = list(inside[np.round(np.linspace(0, len(inside) - 1, 16)).astype(int)]) + [40]
        assert len(set(chosen)) == 17 and 0 in chosen and 64 in chosen
        for c in chosen:
            onehot = np.zeros(len(src))
            onehot[c] = 1.0
            H, g, e2 = reg.calc_H_g_e2(T, src, weights=onehot)
            if not mask[c]:
                assert not H.any() and not g.any() and e2 == 0.0 and reg.last_weight_sum == 0.0, (name, c)
                continue
            assert reg.last_weight_sum == 1.0 and np.array_equal(H, H.T)
            if name in ("plane", "vplane"):
                Jc, rc = J[c, 0], r[c, 0]
                assert np.array_equal(H, Jc[:, None] * Jc[None, :]), (name, c)
                assert np.array_equal(g, Jc * rc) and e2 == rc * rc, (name, c)
                continue
            A, d = J[c, :, 3:], r[c]
            assert np.array_equal(J[c, :, :3], np.eye(3))
            if name == "icp":
                assert np.array_equal(H[:3, :3], np.eye(3)) and np.array_equal(H[:3, 3:], A), (name, c)
                AtA = (A[0][:, None] * A[0][None, :] + A[1][:, None] * A[1][None, :]) + A[2][:, None] * A[2][None, :]
                assert np.array_equal(H[3:, 3:], AtA), (name, c)
                assert e2 == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] and np.array_equal(g[:3], d), (name, c)
                continue
            C = ws[c]
            CA = (C[:, 0, None] * A[0][None, :] + C[:, 1, None] * A[1][None, :]) + C[:, 2, None] * A[2][None, :]
            assert np.array_equal(H[:3, :3], C) and np.array_equal(H[:3, 3:], CA), (name, c)
            # everything else: test_values' bound, 4 * 2^-53 * sum |products|, against acc_ndt's expressions over the row
            Cd = (C[:, 0] * d[0] + C[:, 1] * d[1]) + C[:, 2] * d[2]
            aC, aA, ad = np.abs(C), np.abs(A), np.abs(d)
            AtCA = (A[0][:, None] * CA[0][None, :] + A[1][:, None] * CA[1][None, :]) + A[2][:, None] * CA[2][None, :]
            want = (AtCA[np.triu_indices(3)], Cd, (A[0] * Cd[0] + A[1] * Cd[1]) + A[2] * Cd[2], (d[0] * Cd[0] + d[1] * Cd[1]) + d[2] * Cd[2])
            mags = ((aA.T @ (aC @ aA))[np.triu_indices(3)], aC @ ad, aA.T @ (aC @ ad), ad @ (aC @ ad))
            for got, w, m in zip((H[3:, 3:][np.triu_indices(3)], g[:3], g[3:], e2), want, mags):
                assert np.all(np.abs(got - w) <= 4 * EPS * m), (name, c)
    finally:
        if name == "icp":
            reg._target = None                          # (borrowed handle)


# ----------------------------------------------------------------------------- 4. order and edges
def bits_equal(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                                              y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_order_and_edges(capi, regs, g2, name):
    reg, T, src = regs[name], g2["T"], g2["source"]
    ctx = capi.get_context(0)
    rng = np.random.default_rng(7)
    m = 1 if name in ("plane", "vplane") else 3
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        cut = np.ascontiguousarray(src[:n])
        base = reg.linearize(T, cut, return_index=True)
        assert base[0].shape == (n, m, 6) and base[1].shape == (n, m) and base[3].shape == (n,)
        assert base[2].shape == ((n, 3, 3) if name == "ndt" else (n,))
        perm = rng.permutation(n)
        moved = reg.linearize(T, np.ascontiguousarray(cut[perm]), return_index=True)
        assert bits_equal(moved, [a[perm] for a in base]), (name, n, "permutation")
        # a KEEP_ORDER scan and a NO_SCAN_SORT scan give identical rows
        kind = reg.KIND
        a = capi.linearize_rows(reg._target, capi.Scan(ctx, cut, flags=capi.FLAG_KEEP_ORDER), kind, T, reg.max_dist, reg._flags, True)
        b = capi.linearize_rows(reg._target, capi.Scan(ctx, cut, flags=capi.FLAG_NO_SCAN_SORT), kind, T, reg.max_dist, reg._flags, True)
        keep = [k for k in range(5) if a[k] is not None]
        assert bits_equal([a[k] for k in keep], [b[k] for k in keep]), (name, n, "KEEP_ORDER vs NO_SCAN_SORT")
    # every point gated out
    J, r, w, W, idx = capi.linearize_rows(reg._target, capi.Scan(ctx, np.ascontiguousarray(src[:257]), flags=capi.FLAG_KEEP_ORDER), reg.KIND,
                                          T, 1e-6, reg._flags, True)
    assert not J.any() and not r.any() and not w.any() and np.all(idx == -1) and (W is None or not W.any())


# ----------------------------------------------------------------------------- 5. weighted evaluation
@pytest.mark.parametrize("name", NAMES)
def test_weighted_evaluation(regs, rows, g2, name):
    import point_cloud_registration_amd as pcr
    T, src = g2["T"], g2["source"]
    J, r, ws, idx = rows[name]
    n = len(src)
    mask = idx >= 0
    # the weighted sums are the rows' sums (for ICP: the flag-0 sums of the rows; the quirk changes g[3:] only)
    reg = regs[name]
    if name == "icp":
        reg = pcr.ICP(max_dist=float(g2["max_dist"]), compat_flags=0)
        reg._set_target_handle(regs[name]._target)
    try:
        (H1, g1, e1), mags = row_sums(J, r, ws)
        got = reg.calc_H_g_e2(T, src, weights=np.ones(n))
        assert_sums(got, (H1, g1, e1), mags, n, f"{name} ones vs rows")
        assert_sums(got, reg.calc_H_g_e2(T, src), mags, n, f"{name} ones vs unweighted")
        assert reg.last_weight_sum == float(mask.sum())
        rng = np.random.default_rng(11)
        w01 = (rng.random(n) < 0.6).astype(np.float64)
        got = reg.calc_H_g_e2(T, src, weights=w01)
        (Hs, gs, es), ms = row_sums(J, r, ws, w01)
        assert_sums(got, reg.calc_H_g_e2(T, np.ascontiguousarray(src[w01 > 0])), ms, n, f"{name} 0/1 vs subset")
        assert reg.last_weight_sum == float((w01 * mask).sum())
        wr = rng.uniform(0.5, 2.0, n)
        got = reg.calc_H_g_e2(T, src, weights=wr)
        want, mw = row_sums(J, r, ws, wr)
        assert_sums(got, want, mw, n, f"{name} random weights")
        assert abs(reg.last_weight_sum - math.fsum(wr[mask])) <= n * EPS * wr[mask].sum()
    finally:
        if name == "icp":
            reg._target = None


def test_weighted_icp_quirk(regs, rows, g2):
    """Under the default compat flag the weighted g[3:] is sum w p x (R r); H, g[:3] and e2 are the rows' sums."""
    T, src = g2["T"], g2["source"]
    J, r, ws, idx = rows["icp"]
    n = len(src)
    wr = np.random.default_rng(12).uniform(0.5, 2.0, n)
    H, g, e2 = regs["icp"].calc_H_g_e2(T, src, weights=wr)
    (Hw, gw, ew), (mH, mg, me) = row_sums(J, r, ws, wr)
    p, rr = src.astype(np.float64), r @ T[:3, :3].T
    terms = np.cross(p, rr) * (ws * wr)[:, None]
    gw[3:], _ = fsum_cols(terms)
    ap, ar = np.abs(p), np.abs(r) @ np.abs(T[:3, :3]).T
    mg[3:] = ((ap[:, [1, 2, 0]] * ar[:, [2, 0, 1]] + ap[:, [2, 0, 1]] * ar[:, [1, 2, 0]]) * (ws * wr)[:, None]).sum(0)
    assert_sums((H, g, e2), (Hw, gw, ew), (mH, mg, me), n, "icp quirk weighted")


# ----------------------------------------------------------------------------- 6. coreset
G15 = load_golden("g15_coreset_cases.npz")
CORESET_BOUND = 10.0 * float(np.max(G15["row_rel"][G15["M"] == 28]))


def terms_matrix(J, r, ws):
    """P (28, N) of the rows: triu(J^T W J), J^T W r, r^T W r per point."""
    if ws.ndim == 1:
        WJ, Wr = ws[:, None, None] * J, ws[:, None] * r
    else:
        WJ, Wr = np.einsum("nik,nkl->nil", ws, J), np.einsum("nik,nk->ni", ws, r)
    tH = np.einsum("nij,nil->njl", J, WJ)[:, TRIU[0], TRIU[1]]
    return np.ascontiguousarray(np.hstack([tH, np.einsum("nij,ni->nj", J, Wr), np.einsum("ni,ni->n", r, Wr)[:, None]]).T)


def check_coreset(reg, T, src, P_full, mask, tag):
    count = int(mask.sum())
    ind, w = reg.coreset(T, src, N_target=64, k=64)
    print(f"{tag}: {count} gated in -> {len(ind)} points, min w {w.min():.3g}, |sum w - count| / count {abs(w.sum() - count) / count:.2e}")
    assert ind.dtype == np.int64 and w.dtype == np.float64 and len(ind) == len(w) <= 64
    assert np.all(np.diff(ind) > 0) and np.all(mask[ind])
    assert np.all(w > 0)
    assert abs(math.fsum(w) - count) <= 1e-12 * count
    # the reduced scan reproduces the full sums (same pose, every point finds its own neighbour again): the per-row relative
    # error of coreset_cases.per_row_error over the 28 sums, through calc_H_g_e2 and from the rows themselves
    full = reg.calc_H_g_e2(T, src)
    Hc, gc, ec = reg.calc_H_g_e2(T, np.ascontiguousarray(src[ind]), weights=w)
    P = P_full[:, mask]
    den = np.array([math.fsum(np.abs(row)) for row in P])
    got = np.concatenate([Hc[TRIU], gc, [ec]])
    want = np.concatenate([full[0][TRIU], full[1], [full[2]]])
    live = den > 0
    rel = np.max(np.abs(got - want)[live] / den[live])
    assert np.all(got[~live] == want[~live])
    rel_rows, exact = cc.per_row_error(P, np.ones(count), w, np.searchsorted(np.flatnonzero(mask), ind))
    print(f"{tag}: per-row error through calc_H_g_e2 {rel:.2e}, from the rows {rel_rows:.2e} (bound {CORESET_BOUND:.2e})")
    assert exact and rel_rows <= CORESET_BOUND and rel <= CORESET_BOUND
    # N_target >= count: every gated-in point, weight 1
    ind_all, w_all = reg.coreset(T, src, N_target=count, k=64)
    assert np.array_equal(ind_all, np.flatnonzero(mask)) and np.all(w_all == 1.0)
    # deterministic
    ind2, w2 = reg.coreset(T, src, N_target=64, k=64)
    assert np.array_equal(ind, ind2) and np.array_equal(w.view(np.uint64), w2.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_coreset(regs, rows, g2, name):
    import point_cloud_registration_amd as pcr
    T, src = g2["T"], g2["source"]
    J, r, ws, idx = rows[name]
    mask = idx >= 0
    P = terms_matrix(J, r, ws)
    if name != "icp":
        check_coreset(regs[name], T, src, P, mask, name)
        return
    # ICP under the default compat flag (quirk Q1): its g[3:] terms are p x (R r), from the rows
    Pq = P.copy()
    Pq[24:27] = (np.cross(src.astype(np.float64), r @ T[:3, :3].T) * ws[:, None]).T
    check_coreset(regs[name], T, src, Pq, mask, "icp quirk")
    plain = pcr.ICP(max_dist=float(g2["max_dist"]), compat_flags=0)
    plain._set_target_handle(regs[name]._target)
    try:
        check_coreset(plain, T, src, P, mask, "icp flags 0")
    finally:
        plain._target = None                    # (borrowed handle)


# ----------------------------------------------------------------------------- 7. nothing else moved
@pytest.mark.parametrize("pipe", ["default", "reuse"])
@pytest.mark.parametrize("name", NAMES)
def test_rows_leave_the_scan_alone(capi, regs, g2, name, pipe):
    """pcr_linearize / pcr_align over a scan: the same bits before and after pcr_linearize_rows / pcr_scan_coreset on it."""
    ctx = capi.get_context(0)
    reg, T, src, md = regs[name], g2["T"], g2["source"], float(g2["max_dist"])
    T2 = T.copy(); T2[:3, 3] += 0.003

    def run(with_rows):
        sc = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
        out = [capi.linearize(reg._target, sc, reg.KIND, T, md).copy()]
        if with_rows:
            capi.linearize_rows(reg._target, sc, reg.KIND, T2, md, reg._flags, True)
            capi.scan_coreset(reg._target, sc, reg.KIND, T2, md, 64, 64, reg._flags)
            capi.linearize_weighted(reg._target, sc, reg.KIND, T2, md, np.ones(len(src)), reg._flags)
        out.append(capi.linearize(reg._target, sc, reg.KIND, T2, md).copy())
        out.append(capi.linearize(reg._target, sc, reg.KIND, T, md).copy())
        Ta, it = capi.align(reg._target, sc, reg.KIND, T, 5, 1e-3, md)
        out += [Ta, np.array([float(it)])]
        if with_rows:
            capi.linearize_rows(reg._target, sc, reg.KIND, T, md, reg._flags, False)
        out.append(capi.linearize(reg._target, sc, reg.KIND, Ta, md).copy())
        return out

    with ctx.pipeline(**PIPELINES[pipe]):
        a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64)), (name, pipe)


def test_fast_caratheodory_after_the_refactor(capi, regs, g2):
    """pcr_coreset is now a host-upload front over the device-resident core it shares with pcr_scan_coreset.  On g14's first
    case: the selection has the properties g14's own test pins, and it is bit-identical before and after a pcr_scan_coreset
    ran on the same context (the two routes share the core, the context's stream and its block cache).  g14 stores no
    selection, so bit-identity to the library BEFORE the refactor is not asserted here, and it has NOT been verified anywhere
    else either: it is argued from the code alone (the core issues the same launches in the same order with the same
    arguments as the old pcr_coreset did)."""
    from point_cloud_registration_amd import create_gn_set, fast_caratheodory
    g14 = load_golden("g14_coreset.npz")
    P = create_gn_set(g14["gn0_J"], g14["gn0_r"])
    assert np.array_equal(P, g14["gn0_P"])
    u = np.ones(P.shape[1])
    a = fast_caratheodory(P, u, 64, 128)
    reg = regs["plane"]
    sc = capi.Scan(capi.get_context(0), g2["source"], flags=capi.FLAG_KEEP_ORDER)
    ind, _ = capi.scan_coreset(reg._target, sc, reg.KIND, g2["T"], float(g2["max_dist"]), 64, 64, reg._flags)
    assert 0 < len(ind) <= 64
    b = fast_caratheodory(P, u, 64, 128)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                     y.view(np.uint64) if y.dtype == np.float64 else y)
    P_sel, w, idx = a
    assert np.array_equal(P_sel, P[:, idx]) and np.all(np.diff(idx) > 0) and np.all(w > 0) and len(w) <= 128
    rel, exact = cc.per_row_error(P, u, w, idx)
    assert exact and rel <= CORESET_BOUND


def test_one_upload_serves_rows_and_plain_calls(capi, regs, g2):
    """linearize / weights / coreset alternating with plain calc_H_g_e2 on the same array (the README workflow) upload and
    sort the scan once: the cached order-keeping scan serves the plain call, with the bits a plain scan gives."""
    import point_cloud_registration_amd as pcr
    T, src = g2["T"], g2["source"]
    fresh = pcr.PlaneICP(max_dist=float(g2["max_dist"]))
    fresh._set_target_handle(regs["plane"]._target)
    try:
        want = fresh.calc_H_g_e2(T, src)                # a plain scan ...
        plain_scan = fresh._scan
        fresh.linearize(T, src)                         # ... cannot serve rows: uploaded again, order kept
        kept = fresh._scan
        assert kept is not plain_scan and kept.flags & capi.FLAG_KEEP_ORDER
        got = fresh.calc_H_g_e2(T, src)
        assert fresh._scan is kept
        fresh.calc_H_g_e2(T, src, weights=np.ones(len(src)))
        fresh.coreset(T, src, N_target=64, k=64)
        assert fresh._scan is kept
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    finally:
        fresh._target = None                            # (borrowed handle)


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals_and_memory(capi, regs, g2, g9):
    import gc
    import torch
    import point_cloud_registration_amd as pcr
    ctx = capi.get_context(0)
    reg, T, src, md = regs["plane"], g2["T"], g2["source"], float(g2["max_dist"])
    good = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
    before = capi.linearize_rows(reg._target, good, reg.KIND, T, md, reg._flags, True)
    calls = (lambda t, s: capi.linearize_rows(t, s, capi.PLANE, T, md),
             lambda t, s: capi.linearize_weighted(t, s, capi.PLANE, T, md, np.ones(s.n)),
             lambda t, s: capi.scan_coreset(t, s, capi.PLANE, T, md, 64, 64))
    # a sorted scan without KEEP_ORDER
    plain = capi.Scan(ctx, src)
    for call in calls:
        with pytest.raises(ValueError, match="PCR_FLAG_KEEP_ORDER"):           # PCR_ERR_INVALID
            call(reg._target, plain)
    # a float64 PlaneICP target (quirk Q6)
    q6 = pcr.PlaneICP(max_dist=float(g9["max_dist"]), k=int(g9["k"]))
    q6.set_target(g9["target"], kdree=object(), norm=g9["plane_normals"])
    s9 = capi.Scan(ctx, g9["source"], flags=capi.FLAG_KEEP_ORDER)
    for call in calls:
        with pytest.raises(capi.PcrError, match=f"status {capi.PCR_ERR_UNSUPPORTED}: .*float64 point target"):
            call(q6._target, s9)
    H9 = q6.calc_H_g_e2(g9["T"], g9["source"])
    assert np.all(np.isfinite(H9[0]))
    # a bad k / n_target at the C boundary
    with pytest.raises(ValueError):
        capi.scan_coreset(reg._target, good, capi.PLANE, T, md, 29, 64)
    with pytest.raises(ValueError):
        capi.scan_coreset(reg._target, good, capi.PLANE, T, md, 64, 28)
    after = capi.linearize_rows(reg._target, good, reg.KIND, T, md, reg._flags, True)
    keep = [k for k in range(5) if before[k] is not None]
    assert bits_equal([before[k] for k in keep], [after[k] for k in keep])

    # device memory does not grow over 20 calls of each entry point
    def cycle():
        sc = capi.Scan(ctx, src, flags=capi.FLAG_KEEP_ORDER)
        return [c(reg._target, sc) for c in calls]

    cycle(); gc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    gc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
