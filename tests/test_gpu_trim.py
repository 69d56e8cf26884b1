"""The adaptive pass of GICP, VGICP, SymmetricICP and ColoredICP on the GPU (include/pcr.h: "adaptive pass"): the selection
inside the pass, the sums of a trim, a trim at quantile 1, the M-estimators at the scale the pass found, align, and isolation.
It mirrors tests/test_gpu_robust.py over the same fixtures (tests/trim_sides.py); tests/trim_cases.py restates the rule.

What the threshold is compared with is the GPU's OWN squared residuals (pcr_*_residuals, turned into keys by trim_cases.key):
tau must be their k-th smallest bit for bit, n_le their count <= tau, and the kept set of a trim {kappa_gpu <= tau} -- so the
rounding of a GICP / VGICP residual cannot flip a membership and nothing needs to be excluded as fragile.

The bound on the sums of a trim, per entry: the plain pass's own bound (symm_cases.sum_bound, color_cases.sum_bound,
gicp_cases.sum_bound) on the magnitudes of the KEPT terms.  A weight of exactly 0 or 1 adds no error term of its own, so the
factor 1.5 that tests/test_gpu_robust.py derives for a weight computed from a rounded s is not needed here."""

import ctypes

import numpy as np
import pytest

import dist_cases as dc
import gicp_cases as gc
import robust_cases as rc
import trim_cases as tc
import trim_sides as ts

pytestmark = pytest.mark.gpu

ALIGNERS = ts.ALIGNERS
SMALL = (1, 2, 255, 256, 257)
# quantiles that give k = 1, a k in the middle and k = m
QUANTILES = (1e-9, 0.5, 1.0)


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


@pytest.fixture(scope="module")
def sides(capi, ctx, orc, g2):
    return ts.build(capi, ctx, orc, g2)


def _check_selection(side, s, kind, q, factor, what):
    """stats and out[28] of one adaptive pass against the GPU's own keys -> (out, stats, kappa)."""
    out, stats = side.adaptive(s, kind, q, factor)
    kappa = side.keys(s)
    tau, k, m, n_le = tc.threshold(kappa, q)
    assert out[28] == m == side.plain(s)[28], (what, out[28], m)
    if m == 0:
        assert np.array_equal(stats, [np.inf, 0.0, 0.0, 0.0]) and not out.any(), (what, stats)
        return out, stats, kappa
    assert stats[0] == tau and np.float64(stats[0]).tobytes() == np.float64(tau).tobytes(), (what, stats[0], tau)
    assert stats[2] == n_le and stats[3] == k == tc.rank(q, m), (what, stats, n_le, k)
    c = 0.0 if kind == "trim" else tc.scale(tau, factor)[0]
    print(f"{what} {kind} q {q}: m {m}, k {k}, kept {n_le}, tau {tau:.6e}, c {stats[1]:.17g} (restated {c:.17g})")
    assert stats[1] == c, (what, stats[1], c)
    return out, stats, kappa


def _check_trim(side, s, rows, q, what):
    """A trim over the scan of base rows ``rows``: the selection, then the sums against math.fsum over {kappa_gpu <= tau}."""
    out, stats, kappa = _check_selection(side, s, "trim", q, 1.0, what)
    kept = (kappa <= stats[0]) & (kappa < np.inf)
    mult = np.bincount(np.asarray(rows)[kept], minlength=len(side.scan))
    assert np.all(side.keep[mult > 0])                                  # (every kept row is one the restatement keeps)
    ref, mag = side.sums_over(mult)
    count = int(kept.sum())
    assert count == stats[2]
    bound = side.bound(count, mag)
    err = np.abs(out[:28] - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{what} trim q {q}: kept {count} of {int(out[28])}, max error / bound {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3e}")
    assert np.all(np.isfinite(out)) and np.all(err <= bound), (what, q, np.nonzero(err > bound)[0].tolist())
    out2, stats2 = side.adaptive(s, "trim", q)
    assert np.array_equal(out2, out) and np.array_equal(stats2, stats), (what, q, "second call")
    return out, stats


# ----------------------------------------------------------------------------- 1. the selection inside the pass, 2. trim sums
@pytest.mark.parametrize("n", SMALL + (2000,))
@pytest.mark.parametrize("name", ALIGNERS)
def test_trim(sides, name, n):
    side = sides[name]
    rows = np.arange(n)
    s = side.upload(rows)
    for q in QUANTILES:
        _check_trim(side, s, rows, q, (name, n))


@pytest.mark.parametrize("name", ["symm", "gicp", "vgicp"])
def test_no_caller_order_needed(sides, name):
    """A Morton-sorted scan that does not know the caller's order, its payload estimated on it: pcr_*_residuals refuses it, the
    adaptive pass runs -- its keys are in device order -- and counts what the plain pass counts."""
    side = sides[name]
    bare = side.capi.Scan(side.ctx, side.scan)
    bare.estimate_normals(10, want=False) if name == "symm" else bare.estimate_covariances(10, want=False)
    with pytest.raises(ValueError, match="order"):
        side.entry("residuals")(side.tgt, bare, side.T, side.md, *side.extra)
    plain = side.plain(bare)
    for kind, q in (("trim", 0.5), ("trim", 1.0), ("cauchy", 0.5)):
        out, stats = side.adaptive(bare, kind, q, 3.0)
        assert out[28] == plain[28] > 0 and stats[3] == tc.rank(q, int(plain[28])) and stats[2] >= stats[3] and np.isfinite(stats[0])
        assert np.array_equal(side.adaptive(bare, kind, q, 3.0)[0], out)


@pytest.mark.parametrize("name", ALIGNERS)
def test_ties_at_tau_are_all_kept(sides, name):
    """The first 100 of 300 rows twice: every key of those appears twice.  A rank that lands on the first of such a pair keeps
    both: kept > k, and the sums are those of the larger set."""
    side = sides[name]
    rows = np.concatenate([np.arange(300), np.arange(100)])
    s = side.upload(rows)
    kappa = side.keys(s)
    f = np.sort(kappa[kappa < np.inf])
    m = len(f)
    tied = np.nonzero(f[:-1] == f[1:])[0]
    tied = tied[(tied == 0) | (f[np.maximum(tied, 1) - 1] < f[tied])]   # the FIRST of a run
    assert len(tied) > 20
    k = int(tied[len(tied) // 2]) + 1
    q = (k + 0.5) / m
    assert tc.rank(q, m) == k
    out, stats = _check_trim(side, s, rows, q, (name, "ties"))
    assert stats[3] == k and stats[2] >= k + 1


def test_grid_rule_on_this_device(cus):
    """The sizes below make slots and trips live only while the reduce grid is 8 blocks per CU."""
    assert dc.stride_points(cus) == 524288, cus


@pytest.mark.parametrize("name, slot", [(a, k) for a in ALIGNERS for k in range(ts.ROBUST_W[a])])
def test_trim_live_slots(sides, cus, name, slot):
    """dist_cases.big_sizes with the adaptive reduce's W (the robust kernel's): slot 1 (.. W - 1), then the second trip carry
    live points -- and the selection runs past its own first stride (262144 keys)."""
    side = sides[name]
    n = dc.big_sizes(cus, ts.ROBUST_W[name])[slot]
    rows = np.arange(n) % len(side.scan)
    s = side.upload(rows)
    try:
        out, stats = _check_trim(side, s, rows, 0.6, (name, n))
        assert 0 < stats[2] < out[28] < n
    finally:
        s.close()


# ----------------------------------------------------------------------------- 3. quantile 1
@pytest.mark.parametrize("name", ALIGNERS)
def test_quantile_one(sides, name):
    """The rule of test_gpu_robust.test_weights_of_one: a trim at quantile 1 keeps everything at weight exactly 1, so where the
    adaptive reduce keeps the plain kernel's W it adds the same numbers in the same order -- the plain entry point's 29 values
    bit for bit (color, gicp, vgicp); k_symm_adaptive carries 2 points per lane where k_symm_reduce carries 3: within the bound."""
    side = sides[name]
    N0 = len(side.scan)
    s = side.upload(np.arange(N0))
    plain = side.plain(s)
    out, stats = side.adaptive(s, "trim", 1.0)
    assert stats[2] == stats[3] == out[28] == plain[28] == side.keep.sum()
    if ts.ROBUST_W[name] == ts.PLAIN_W[name]:
        assert np.array_equal(out, plain), name
    else:
        ref, mag = side.sums_over(np.ones(N0))
        bound = side.bound(int(side.keep.sum()), mag)
        assert np.all(np.abs(out[:28] - ref) <= bound) and np.all(np.abs(out[:28] - plain[:28]) <= bound), name


# ----------------------------------------------------------------------------- 4. M-estimators
@pytest.mark.parametrize("n", (257, 2000))
@pytest.mark.parametrize("name", ALIGNERS)
def test_m_estimators_at_the_scale_of_the_pass(sides, name, n):
    """linearize_adaptive(kind, q, factor) == linearize_robust(kind, scale = stats[1]) bit for bit, at q = 0.25, 0.5 and 1."""
    side = sides[name]
    s = side.upload(np.arange(n))
    for kind in rc.KINDS:
        for q in (0.25, 0.5, 1.0):
            out, stats, _ = _check_selection(side, s, kind, q, 3.0, (name, n))
            assert stats[1] > 0.0
            want = side.robust(s, kind, stats[1])
            assert np.array_equal(out, want), (name, n, kind, q)
    out, stats = side.adaptive(s, "tukey", 0.5, 3.0)
    again = side.adaptive(s, "tukey", 0.5, 3.0)
    assert np.array_equal(out, again[0]) and np.array_equal(stats, again[1])
    assert not np.array_equal(out[:28], side.plain(s)[:28])                    # (the kernel did weigh)


@pytest.mark.parametrize("name", ALIGNERS)
def test_scale_zero_is_the_limit(sides, name):
    """A scan that is a subset of the target at the identity, plus a quarter of points moved off it by 0.05: more than half of
    the keys are exactly 0, so tau = 0 and c = 0 at q = 0.5.  Every kernel then takes w = (s == 0 ? 1 : 0): finite sums, no NaN,
    only the s == 0 terms counted -- which is the trim at the same rank (kept: kappa <= 0), bit for bit; out[28] stays m."""
    side = sides[name]
    pts, payload = side.subset
    s = side.upload_points(pts, payload)
    I = np.eye(4)
    kappa = side.keys(s, I)
    m, zeros = int(np.sum(kappa < np.inf)), int(np.sum(kappa == 0.0))
    print(f"{name}: {len(pts)} points, m {m}, keys == 0: {zeros}, > 0: {int(np.sum((kappa > 0) & (kappa < np.inf)))}")
    assert zeros > m / 2 and np.sum((kappa > 0) & (kappa < np.inf)) > 0                     # (conditions on the input)
    trim, tstats = side.adaptive(s, "trim", 0.5, T=I)
    assert np.array_equal(tstats, [0.0, 0.0, zeros, tc.rank(0.5, m)]) and trim[28] == m
    assert np.any(trim[:21] != 0.0) and not trim[21:28].any()                               # J^T J of the kept; r = 0 there
    for kind in rc.KINDS:
        out, stats = side.adaptive(s, kind, 0.5, 3.0, T=I)
        assert np.array_equal(stats, tstats), (name, kind, stats)
        assert np.all(np.isfinite(out)) and out[28] == m
        assert np.array_equal(out, trim), (name, kind)
    # and a scale above 0 again one rank past the zeros
    out, stats = side.adaptive(s, "tukey", (zeros + 1.5) / m, 3.0, T=I)
    assert stats[0] > 0.0 and stats[1] > 0.0 and np.all(np.isfinite(out)) and np.array_equal(out, side.robust(s, "tukey", stats[1], T=I))


# ----------------------------------------------------------------------------- 5. align
@pytest.mark.parametrize("setting", [tc.E2E_TRIM, tc.E2E_TUKEY], ids=["trim", "tukey"])
@pytest.mark.parametrize("name", ALIGNERS)
def test_align(capi, ctx, case, name, setting):
    """What test_gpu_robust.test_align asserts, under the adaptive pass: the native loop equals the Python loop over calc_H_g_e2
    within 1e-10 with the same iteration count, every trace row and stats row is *_linearize_adaptive at that row's pose bit for
    bit -- and the pose is closer to the truth than the plain aligner's on the same data, within twice the error the
    restatement recorded (trim_cases.ADAPTIVE_ERRORS; the factor 2 is test_gpu_robust.test_align's margin)."""
    from point_cloud_registration_amd.math_tools import plus
    kind, q, factor = setting
    scan = case["scan"]
    kw_reg = dict(trim=q) if kind == "trim" else dict(robust=kind, robust_scale=("quantile", q, factor))
    reg, kw = ts.e2e_reg(name, capi, ctx, case, **kw_reg)
    T = reg.align(scan, **kw)
    iters = reg.last_iterations
    assert reg.last_adaptive_trace.shape == (iters, 4) and list(reg.last_adaptive) == ["tau", "scale", "kept", "k"]
    assert list(reg.last_adaptive.values()) == reg.last_adaptive_trace[-1].tolist()
    cur, it = np.eye(4), 0
    for it in range(reg.max_iter):
        H, g, _ = reg.calc_H_g_e2(cur, scan, **kw)
        if it == 0:                                    # (the same pose, so the same bits; later poses agree within 1e-10 only)
            assert list(reg.last_adaptive.values()) == reg.last_adaptive_trace[0].tolist()
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < reg.tol:
            break
        cur = plus(cur, dx)
    assert iters == it + 1 and iters < reg.max_iter
    assert np.max(np.abs(T - cur)) <= 1e-10
    dev = reg._pass_scan(scan, **kw)
    params = reg._pass_params()
    ad = (tc.KIND_ID[kind], q, factor)
    T2, iters2, stats, trace = getattr(capi, f"{name}_align_adaptive")(reg._target, dev, np.eye(4), reg.max_iter, reg.tol, rc.E2E_MAX_DIST,
                                                                       *params, adaptive=ad, want_trace=True)
    assert iters2 == iters and np.array_equal(T2, T) and trace.shape == (iters, 45) and stats.shape == (iters, 4)
    assert np.array_equal(stats, reg.last_adaptive_trace)
    for row, st in zip(trace, stats):
        out, st1 = getattr(capi, f"{name}_linearize_adaptive")(reg._target, dev, row[:16], rc.E2E_MAX_DIST, *params, adaptive=ad)
        assert np.array_equal(out, row[16:]) and np.array_equal(st1, st)
    plain, kwp = ts.e2e_reg(name, capi, ctx, case)
    Tp = plain.align(scan, **kwp)
    ep, er = rc.t_err(Tp, case), rc.t_err(T, case)
    rec = tc.ADAPTIVE_ERRORS[name][0 if kind == "trim" else 1]
    print(f"{name}: plain |dt| {ep:.4e} ({plain.last_iterations} iterations), {kind} q {q} factor {factor}: |dt| {er:.4e} "
          f"({iters}; restated {rec:.4e}); last pass {reg.last_adaptive}")
    assert er < ep
    assert er <= 2.0 * rec


# ----------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("name", ALIGNERS)
def test_plain_and_fixed_scale_calls_are_what_they_were(capi, ctx, case, name):
    """robust=None, trim=None and a float robust_scale: the class returns the plain and the robust entry point's bits, before
    and after an adaptive call on the same cached scan."""
    scan = case["scan"]
    plain, kw = ts.e2e_reg(name, capi, ctx, case)
    fixed, _ = ts.e2e_reg(name, capi, ctx, case, robust="cauchy", robust_scale=rc.E2E_SCALE[name])
    trim, _ = ts.e2e_reg(name, capi, ctx, case, trim=0.6)
    T = np.eye(4)
    dev = plain._pass_scan(scan, **kw)
    params = plain._pass_params()
    want_p = getattr(capi, f"{name}_linearize")(plain._target, dev, T, rc.E2E_MAX_DIST, *params)
    for reg, extra in ((plain, {}), (fixed, dict(robust=(2, rc.E2E_SCALE[name])))):
        dev_r = reg._pass_scan(scan, **kw)
        want = getattr(capi, f"{name}_linearize_robust")(reg._target, dev_r, T, rc.E2E_MAX_DIST, *params, **extra)
        for _ in range(2):
            H, g, e2 = reg.calc_H_g_e2(T, scan, **kw)
            assert np.array_equal(H[gc.TRIU], want[:21]) and np.array_equal(g, want[21:27]) and e2 == want[27]
            assert reg.last_adaptive is None and reg.last_adaptive_trace is None
            trim.calc_H_g_e2(T, scan, **kw)                                     # (an adaptive call in between)
    assert np.array_equal(plain.calc_H_g_e2(T, scan, **kw)[0][gc.TRIU], want_p[:21])
    assert trim.last_adaptive["kept"] >= trim.last_adaptive["k"] > 0


def test_setting_belongs_to_the_aligner(g2, sides):
    """Aligners with different settings over ONE cached device scan: each returns what it returns alone, in any order."""
    import point_cloud_registration_amd as pcr
    side = sides["symm"]
    T, src = side.T, side.scan
    regs = {}
    c = 3.0 * float(np.sqrt(tc.threshold(np.where(side.keep, side.t[:, 27], np.inf), 0.5)[0]))
    for key, kw in (("none", {}), ("trim", dict(trim=0.6)), ("trim9", dict(trim=0.9)), ("fixed", dict(robust="tukey", robust_scale=c)),
                    ("quantile", dict(robust="tukey", robust_scale=("quantile", 0.5, 3.0))), ("huberq", dict(robust="huber", robust_scale=("quantile", 0.5, 3.0)))):
        regs[key] = pcr.SymmetricICP(max_dist=side.md, **kw)
        regs[key].set_target(g2["target"], norm=g2["plane_normals"])
    scan = regs["none"].upload(src, keep_order=True)
    alone = {k: r.calc_H_g_e2(T, scan, source_normals=side.payload) for k, r in regs.items()}
    for order in (("trim", "none", "quantile", "fixed"), ("huberq", "trim9", "trim", "none", "trim9", "quantile")):
        for k in order:
            got = regs[k].calc_H_g_e2(T, scan, source_normals=side.payload)
            assert all(np.array_equal(a, b) for a, b in zip(got, alone[k])), (order, k)
    keys = list(alone)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            # (the fixed scale IS the one the quantile rule finds at this pose: SymmetricICP's residuals are the restated bits)
            assert np.array_equal(alone[a][0], alone[b][0]) == ({a, b} == {"fixed", "quantile"}), (a, b)
    # the class returns the entry point's sums and stats
    s = side.upload(np.arange(len(src)))
    out, stats = side.adaptive(s, "trim", 0.6)
    H, g, e2 = alone["trim"]
    assert np.array_equal(H[gc.TRIU], out[:21]) and np.array_equal(g, out[21:27]) and e2 == out[27]
    regs["trim"].calc_H_g_e2(T, scan, source_normals=side.payload)
    assert list(regs["trim"].last_adaptive.values()) == stats.tolist() and regs["trim"].last_correspondences == out[28]
    assert np.array_equal(alone["none"][0][gc.TRIU], side.plain(s)[:21])


# ----------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("name", ALIGNERS)
def test_refusals(sides, name):
    """A kind outside 1 .. 5, a quantile outside (0, 1] or NaN, (M-estimators) a factor that is not finite and > 0, a NULL
    pcr_adaptive: PCR_ERR_INVALID with out, stats, T_out, trace and iterations untouched.  A trim does not read the factor."""
    side, capi = sides[name], sides[name].capi
    s = side.upload(np.arange(257))
    L = capi.lib()
    T = np.ascontiguousarray(side.T, dtype=np.float64).reshape(16)
    extra = [float(v) for v in side.extra]
    bad = [(0, 0.5, 1.0), (6, 0.5, 1.0), (-1, 0.5, 1.0), (5, 0.0, 1.0), (5, -0.5, 1.0), (5, 1.0000001, 1.0), (5, float("nan"), 1.0),
           (3, float("inf"), 1.0), (1, 0.5, 0.0), (2, 0.5, -1.0), (3, 0.5, float("nan")), (4, 0.5, float("inf")), None]
    for ad in bad:
        p, keep = (None, None) if ad is None else capi._ad(ad)
        out, stats = np.full(29, 7.25), np.full(4, 7.25)
        st = getattr(L, f"pcr_{name}_linearize_adaptive")(side.tgt.handle, s.handle, T, side.md, *extra, p, 0, out, stats)
        assert st == capi.PCR_ERR_INVALID and np.all(out == 7.25) and np.all(stats == 7.25), (ad, st)
        T_out, iters, trace, rows = np.full(16, 7.25), ctypes.c_int(-3), np.full((2, 45), 7.25), np.full((2, 4), 7.25)
        st = getattr(L, f"pcr_{name}_align_adaptive")(side.tgt.handle, s.handle, T, 2, 1e-3, side.md, *extra, p, 0, T_out, ctypes.byref(iters),
                                                     trace.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p))
        assert st == capi.PCR_ERR_INVALID and np.all(T_out == 7.25) and np.all(trace == 7.25) and np.all(rows == 7.25) and iters.value == -3, (ad, st)
        if ad is not None:
            with pytest.raises(ValueError):
                side.entry("linearize_adaptive")(side.tgt, s, side.T, side.md, *side.extra, adaptive=ad)
    # the unit's own parameter is refused first, and names itself
    if side.extra:
        p, keep = capi._ad((6, 0.5, 1.0))
        out, stats = np.full(29, 7.25), np.full(4, 7.25)
        st = getattr(L, f"pcr_{name}_linearize_adaptive")(side.tgt.handle, s.handle, T, side.md, 1.5, p, 0, out, stats)
        msg = L.pcr_last_error().decode()
        assert st == capi.PCR_ERR_INVALID and "adaptive" not in msg and ("min_cos" in msg or "lambda_geometric" in msg) and np.all(out == 7.25)
    # a trim does not read the factor; the plain call's refusals stay: a scan without its payload
    for f in (0.0, -1.0, float("nan")):
        assert np.array_equal(side.adaptive(s, "trim", 0.5, f)[0], side.adaptive(s, "trim", 0.5)[0])
    bare = capi.Scan(side.ctx, side.scan, flags=capi.FLAG_KEEP_ORDER)
    with pytest.raises(ValueError):
        side.adaptive(bare, "trim", 0.5)
    # the robust entry points keep refusing kind 5
    with pytest.raises(ValueError):
        side.entry("linearize_robust")(side.tgt, s, side.T, side.md, *side.extra, robust=(5, 1.0))
