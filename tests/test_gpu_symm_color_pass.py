"""The passes of SymmetricICP and ColoredICP (csrc/symm.hip, color.hip over csrc/match_pass.h) at the gate boundary and across the
pose space (tests/normal_pass_cases.py on the clouds of tests/pass_cases.py / g16) -- what tests/test_gpu_dist_pass.py holds
for GICP and VGICP, for the two units whose own tests stay at g2's pose and away from every boundary.

  a  the exact lattices, both forms of the index: 9 exact poses x 13 gates, scan normals whose c = n_q . R n_p is exactly one of
     -1, -0.5, 0, 0.5, S, 1, the normal gate ON, one ulp below and one ulp above 0.5 and S; the sign decision AT c == 0; a dyadic
     colour payload whose gradients are not tangent, at lambda 0, 0.5, 0.968, 1.  Counts compare with the written-out tables.  At
     one gate per pose the same bits from a second call, the class, trace row 0 of the align loop and the trim at quantile 1,
     and the residuals finite on exactly the restated kept rows
  b  the 12 general poses (one rotation of pi - 1e-4, |t| in 0 / 50 / 1e4 m) with random unit normals and gradients, and with
     normals and gradients estimated on the GPU and read back
  c  the robust pass at weights of one on the gate

Where the restated quantities come from: transformed points from oracle.transform (bit-identical to the kernels' xform:
pass_cases.exact_poses asserts it), matches and float32 distances from oracle.nn_brute.

Bars (none is new): counts compare exactly; every one of the 28 sums lies within symm_cases.sum_bound / color_cases.sum_bound of
math.fsum of the restated terms; conftest.step_err <= 1e-10 wherever at least 6 pairs are kept and cond(H_ref) <= 1e6 (the rule
of tests/test_gpu_dist_pass.py); all 29 outputs exactly zero where nothing is kept; equal bits between the routes; under a
robust kernel 1.5 x the plain bound (derived in tests/test_gpu_robust.py).

The trim at quantile 1 returns the plain BITS here for both units, also for SymmetricICP whose adaptive reduce carries 2 points
per lane where the plain one carries 3: a 280-point scan lies inside one stride of the grid (at least 8 blocks of 256), so every
lane holds at most one point whatever its width, its weight is exactly 1, and the folds are the same."""

import numpy as np
import pytest

import color_cases as cc
import gicp_cases as gc
import normal_pass_cases as npc
import pass_cases as pc
import symm_cases as sc
from conftest import load_golden, step_err

pytestmark = pytest.mark.gpu

INF = float("inf")
ROUTE_GATES = (0, 1, 2, 5, 7, 8, 10, 11, 12)       # pose k takes its routes at gate ROUTE_GATES[k] (tests/test_gpu_dist_pass.py)
REGULAR = 1e6
TRIM_ALL = (5, 1.0, 1.0)                           # PCR_ROBUST_TRIM at quantile 1 (tests/test_gpu_trim.py: test_quantile_one)
HUBER_ONE = (1, 1e30)                              # PCR_ROBUST_HUBER with c2 = 1e60: every weight is exactly 1


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
def built():
    return pc.build_all(load_golden("g16_pass_cases.npz"))


@pytest.fixture(scope="module")
def lattices(built):
    """normal_pass_cases.lattice_case of both forms, once: it asserts the tables against the rule and the oracle."""
    return {"default": npc.lattice_case(built["pt"]), "heavy": npc.lattice_case(built["heavy"])}


# ----------------------------------------------------------------------------- bars
def _inside(dist, md):
    with np.errstate(over="ignore"):
        return dist < np.float32(md)


def _against(out, ref, bound, kept, what):
    """Count, sums within their bound, zeros where nothing is kept, the step -> (worst error / bound, step checked?)."""
    assert np.all(np.isfinite(out)), what
    assert out[28] == kept, (what, out[28], kept)
    if kept == 0:
        assert not np.any(out), what
        return 0.0, False
    err = np.abs(out[:28] - ref)
    ok = err <= bound
    assert np.all(ok), (what, "entries", np.nonzero(~ok)[0].tolist(), "error / bound", (err[~ok] / bound[~ok]).tolist())
    Href, gref, _ = gc.unpack28(ref)
    stepped = kept >= 6 and np.linalg.cond(Href) <= REGULAR
    if stepped:
        H, g, _ = gc.unpack28(out[:28])
        se = step_err(H, g, Href, gref)
        assert se <= 1e-10, (what, se)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0))), stepped


def _same_bits(out, H, g, e2, cnt, what):
    assert np.array_equal(H[gc.TRIU], out[:21]) and np.array_equal(g, out[21:27]) and e2 == out[27] and cnt == out[28], what


def _trace_row(align, tgt, s, T, md, p, out, what):
    _, iters, trace = align(tgt, s, T, 1, 1e-3, md, p, want_trace=True)
    assert iters == 1 and trace.shape == (1, 45), what
    assert np.array_equal(trace[0, :16], np.asarray(T, dtype=np.float64).reshape(16)), (what, "trace row 0: pose")
    assert np.array_equal(trace[0, 16:], out), (what, "trace row 0: sums")


def _point_target(capi, ctx, monkeypatch, heavy, t32):
    """A point target in the asked form -- and the assertion that it IS that form."""
    if heavy:
        monkeypatch.setenv("PCR_HEAVY", "1")
    tgt = capi.Target.points(ctx, t32)
    monkeypatch.delenv("PCR_HEAVY", raising=False)
    info = tgt.index_info()
    assert info["n"] == t32.shape[0] and info["heavy"] == heavy, info
    return tgt


def _class_target(monkeypatch, heavy, reg, *args, **kw):
    if heavy:
        monkeypatch.setenv("PCR_HEAVY", "1")
    reg.set_target(*args, **kw)
    monkeypatch.delenv("PCR_HEAVY", raising=False)
    assert reg._target.index_info()["heavy"] == heavy
    return reg


class _Memo:
    """The reference of one pose per (mask, parameter): 13 gates give three masks."""

    def __init__(self, make):
        self.make, self.seen = make, {}

    def __call__(self, mask, p):
        key = (mask.tobytes(), p)
        if key not in self.seen:
            self.seen[key] = self.make(mask, p)
        return self.seen[key]


# ----------------------------------------------------------------------------- a. the exact lattices: SymmetricICP
@pytest.mark.parametrize("form", ["default", "heavy"])
def test_symm_lattice_gates(capi, ctx, lattices, monkeypatch, form):
    import point_cloud_registration_amd as pcr
    heavy = form == "heavy"
    case = lattices[form]
    t32, gates, n_q = case["target32"], case["gates"], case["n_q"]
    tgt = _point_target(capi, ctx, monkeypatch, heavy, t32)
    tgt.set_normals(n_q)
    reg = _class_target(monkeypatch, heavy, pcr.SymmetricICP(), t32, norm=n_q)
    pairs = [(gi, mc) for gi in range(len(gates)) for mc in (0.0, 0.5)]
    pairs += [(gi, mc) for gi in npc.FULL_MIN_COS_GATES for mc in npc.MIN_COS if mc not in (0.0, 0.5)]
    flip = np.random.default_rng(1631).random(len(case["probes"])) < 0.5
    everything = np.ones(len(case["probes"]), dtype=bool)
    worst, steps, calls = 0.0, 0, 0
    for pi, (T, scan, n_p, tp, dist, idx, c) in enumerate(case["poses"]):
        s = capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER)
        s.set_normals(n_p)
        terms_all = {mc: sc.terms(T, scan, tp, t32[idx], n_p, n_q[idx], everything, mc) for mc in npc.MIN_COS}
        kept_all = {mc: sc.kept(T, n_p, n_q[idx], everything, mc) for mc in npc.MIN_COS}

        def restate(mask, mc):
            keep = kept_all[mc] & mask
            return sc.reference(terms_all[mc] * keep[:, None], keep) + (keep,)

        memo = _Memo(restate)
        for gi, mc in pairs:
            md, what = gates[gi], ("symm", form, pi, gates[gi], mc)
            ref, bound, kept, keep = memo(_inside(dist, md), mc)
            assert kept == npc.SYMM_COUNTS[gi][npc.MIN_COS.index(mc)], (what, "the oracle's mask against the table", kept)
            out = capi.symm_linearize(tgt, s, T, md, mc)
            w, st = _against(out, ref, bound, kept, what)
            worst, steps, calls = max(worst, w), steps + st, calls + 1
            if gi != ROUTE_GATES[pi] or mc not in (0.0, 0.5):
                continue
            assert np.array_equal(capi.symm_linearize(tgt, s, T, md, mc), out), (what, "second call")
            reg.max_dist, reg.min_normal_cos = md, mc
            H, g, e2 = reg.calc_H_g_e2(T, scan, source_normals=n_p)
            _same_bits(out, H, g, e2, reg.last_correspondences, (what, "class"))
            _trace_row(capi.symm_align, tgt, s, T, md, mc, out, what)
            trim, stats = capi.symm_linearize_adaptive(tgt, s, T, md, mc, adaptive=TRIM_ALL)
            assert np.array_equal(trim, out), (what, "trim at quantile 1")
            assert stats[3] == stats[2] == kept, (what, stats)
            res = capi.symm_residuals(tgt, s, T, md, mc)
            assert res.shape == (len(scan),) and np.array_equal(np.isfinite(res), keep), (what, "residuals: kept rows")
            assert np.array_equal(res[keep], terms_all[mc][keep, 27]) and np.all(np.isposinf(res[~keep])), (what, "residuals")
            if mc > 0.0:
                # no pair with c == 0 is left: negated scan normals return the same bits (tests/test_normal_pass_cases.py)
                s2 = capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER)
                s2.set_normals(np.where(flip[:, None], -n_p, n_p))
                assert np.array_equal(capi.symm_linearize(tgt, s2, T, md, mc), out), (what, "negated normals")
    print(f"symm lattice {form}: worst error / bound {worst:.3e}, step checked at {steps} of {calls}")
    assert steps >= 9


# ----------------------------------------------------------------------------- a. the exact lattices: ColoredICP
@pytest.mark.parametrize("form", ["default", "heavy"])
def test_color_lattice_gates(capi, ctx, lattices, monkeypatch, form):
    import point_cloud_registration_amd as pcr
    heavy = form == "heavy"
    case = lattices[form]
    t32, gates, n_q, I_q, I_p, G = (case[k] for k in ("target32", "gates", "n_q", "I_q", "I_p", "G"))
    n = len(case["probes"])
    tgt = _point_target(capi, ctx, monkeypatch, heavy, t32)
    tgt.set_normals(n_q)
    tgt.set_intensity(I_q, G)
    # lambda = 1 reads neither gradients nor intensities: a target with zero gradients and other intensities, and another scan payload
    other = _point_target(capi, ctx, monkeypatch, heavy, t32)
    other.set_normals(n_q)
    other.set_intensity(np.ascontiguousarray(I_q[::-1]))
    assert not other.get_color()[1].any()
    reg = _class_target(monkeypatch, heavy, pcr.ColoredICP(), t32, I_q, norm=n_q, gradient=G)
    everything = np.ones(n, dtype=bool)
    worst, steps, calls = 0.0, 0, 0
    for pi, (T, scan, n_p, tp, dist, idx, c) in enumerate(case["poses"]):
        s = capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER)
        s.set_intensity(I_p)
        s_other = capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER)
        s_other.set_intensity(np.ascontiguousarray(I_p[::-1]))
        terms_all = {lam: cc.terms(T, scan, tp, t32[idx], n_q[idx], I_q[idx], G[idx], I_p, everything, lam) for lam in npc.LAMBDAS}

        def restate(mask, lam):
            return cc.reference(terms_all[lam] * np.tile(mask, 2)[:, None], mask)

        memo = _Memo(restate)
        for gi, md in enumerate(gates):
            mask = _inside(dist, md)
            for lam in npc.LAMBDAS:
                what = ("color", form, pi, md, lam)
                ref, bound, kept = memo(mask, lam)
                assert kept == pc.POINT_COUNTS_F32[gi], (what, "the oracle's mask against the table", kept)
                out = capi.color_linearize(tgt, s, T, md, lam)
                w, st = _against(out, ref, bound, kept, what)
                worst, steps, calls = max(worst, w), steps + st, calls + 1
                if lam == 1.0:
                    assert np.array_equal(capi.color_linearize(other, s_other, T, md, 1.0), out), (what, "zero gradients, other intensities")
                if gi != ROUTE_GATES[pi]:
                    continue
                assert np.array_equal(capi.color_linearize(tgt, s, T, md, lam), out), (what, "second call")
                reg.max_dist, reg.lambda_geometric = md, lam
                H, g, e2 = reg.calc_H_g_e2(T, scan, I_p)
                _same_bits(out, H, g, e2, reg.last_correspondences, (what, "class"))
                _trace_row(capi.color_align, tgt, s, T, md, lam, out, what)
                trim, stats = capi.color_linearize_adaptive(tgt, s, T, md, lam, adaptive=TRIM_ALL)
                assert np.array_equal(trim, out), (what, "trim at quantile 1")
                assert stats[3] == stats[2] == kept, (what, stats)
                res = capi.color_residuals(tgt, s, T, md, lam)
                assert res.shape == (n, 2), what
                assert np.array_equal(np.isfinite(res[:, 0]), mask) and np.array_equal(np.isfinite(res[:, 1]), mask), (what, "residuals: kept rows")
                t = terms_all[lam]
                assert np.array_equal(res[mask, 0], t[:n][mask, 27]) and np.array_equal(res[mask, 1], t[n:][mask, 27]), (what, "residuals")
                assert np.all(np.isposinf(res[~mask])), (what, "residuals")
    print(f"color lattice {form}: worst error / bound {worst:.3e}, step checked at {steps} of {calls}")
    assert steps >= 9


# ----------------------------------------------------------------------------- b. general poses
def _general_scans(capi, ctx, orc, target, cases):
    """Per case: the scan in the caller's order behind a Morton sort and unsorted, its transformed points and brute-force matches."""
    runs = []
    for name, _, T, scan in cases:
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute(target, tp)
        runs.append((name, T, scan, capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER), capi.Scan(ctx, scan, flags=capi.FLAG_NO_SCAN_SORT),
                     tp, idx, _inside(dist, pc.GENERAL_MAX_DIST)))
    return runs


def _step_rule(norm, st, what, passed):
    """|t| <= 50: the step is checked in every case; |t| = 1e4: where cond(H_ref) <= 1e6 -- which cases those are is printed."""
    if norm <= 50.0:
        assert st, (what, "H_ref is not regular")
    elif st:
        passed.append(what)


@pytest.mark.parametrize("norm", pc.GENERAL_NORMS)
def test_symm_general_poses(capi, ctx, orc, built, norm):
    """min_cos 0 and 0.5.  That no pair inside the distance gate has ||c| - 0.5| < 1e-9 is a condition on the inputs, asserted on
    the restated c; it holds for the random and for the device-estimated normals of all twelve cases, so min_cos stays at 0.5."""
    target, md = built["gen_targets"][norm], pc.GENERAL_MAX_DIST
    cases = [c for c in built["gen"] if c[1] == norm]
    assert len(cases) == 4
    tgt = capi.Target.points(ctx, target)
    runs = _general_scans(capi, ctx, orc, target, cases)
    nq_random, np_random = npc.general_normals(len(target))
    nq_estimated = tgt.estimate_normals(npc.GENERAL_K, compat=False)           # estimated on the device and read back
    np_estimated = [s.estimate_normals(npc.GENERAL_K) for _, _, _, s, _, _, _, _ in runs]
    worst, passed = 0.0, []
    for label, n_q in (("estimated", nq_estimated), ("random", nq_random)):
        if label == "random":
            tgt.set_normals(n_q)
        for k, (name, T, scan, s, s_plain, tp, idx, mask) in enumerate(runs):
            n_p = np_estimated[k] if label == "estimated" else np_random
            s.set_normals(n_p)
            s_plain.set_normals(n_p)
            c = sc.dots(T, n_p, n_q[idx])
            for mc in npc.GENERAL_MIN_COS:
                what = ("symm", label, name, mc)
                assert npc.away_from_gate(c, mask, mc), (what, "a pair within 1e-9 of the normal gate: a condition on the inputs")
                keep = sc.kept(T, n_p, n_q[idx], mask, mc)
                ref, bound, kept = sc.reference(sc.terms(T, scan, tp, target[idx], n_p, n_q[idx], mask, mc), keep)
                out = capi.symm_linearize(tgt, s, T, md, mc)
                w, st = _against(out, ref, bound, kept, what)
                worst = max(worst, w)
                print(f"symm {label} {name} min_cos {mc}: kept {kept} of {int(mask.sum())} inside the gate, c < 0 on "
                      f"{np.mean(c[keep] < 0):.3f}, error / bound {w:.3e}, step checked {st}")
                assert 0 < kept < 1500
                _step_rule(norm, st, what, passed)
                assert np.array_equal(capi.symm_linearize(tgt, s, T, md, mc), out), (what, "second call")
                plain = capi.symm_linearize(tgt, s_plain, T, md, mc)
                assert plain[28] == kept and np.all(np.abs(plain[:28] - ref) <= bound) and np.all(np.abs(plain[:28] - out[:28]) <= bound), what
    print(f"symm general |t| {norm:g}: worst error / bound {worst:.3e}" + (f"; step checked at {passed}" if norm > 50.0 else ""))


@pytest.mark.parametrize("norm", pc.GENERAL_NORMS)
def test_color_general_poses(capi, ctx, orc, built, norm):
    target, md = built["gen_targets"][norm], pc.GENERAL_MAX_DIST
    cases = [c for c in built["gen"] if c[1] == norm]
    assert len(cases) == 4
    tgt = capi.Target.points(ctx, target)
    runs = _general_scans(capi, ctx, orc, target, cases)
    nq_random, _ = npc.general_normals(len(target))
    G_random = npc.general_gradients(len(target))
    I_q = npc.general_intensities(norm, target, target[:1])[0]
    nq_estimated = tgt.estimate_normals(npc.GENERAL_K, compat=False)           # estimated on the device and read back, and the
    tgt.set_intensity(I_q)                                                     # gradients on those normals
    G_estimated = tgt.estimate_color_gradients(npc.GENERAL_K)
    assert G_estimated.any() and np.all(np.isfinite(G_estimated))
    worst, passed = 0.0, []
    for label, n_q, G in (("estimated", nq_estimated, G_estimated), ("random", nq_random, G_random)):
        if label == "random":
            tgt.set_normals(n_q)
            tgt.set_intensity(I_q, G)
        for name, T, scan, s, s_plain, tp, idx, mask in runs:
            I_p = npc.general_intensities(norm, target[:1], tp)[1]
            assert 0.0 <= I_p.min() and I_p.max() <= 1.0
            s.set_intensity(I_p)
            s_plain.set_intensity(I_p)
            for lam in npc.GENERAL_LAMBDAS:
                what = ("color", label, name, lam)
                ref, bound, kept = cc.reference(cc.terms(T, scan, tp, target[idx], n_q[idx], I_q[idx], G[idx], I_p, mask, lam), mask)
                out = capi.color_linearize(tgt, s, T, md, lam)
                w, st = _against(out, ref, bound, kept, what)
                worst = max(worst, w)
                print(f"color {label} {name} lambda {lam}: kept {kept}, error / bound {w:.3e}, step checked {st}")
                assert 0 < kept < 1500
                _step_rule(norm, st, what, passed)
                assert np.array_equal(capi.color_linearize(tgt, s, T, md, lam), out), (what, "second call")
                plain = capi.color_linearize(tgt, s_plain, T, md, lam)
                assert plain[28] == kept and np.all(np.abs(plain[:28] - ref) <= bound) and np.all(np.abs(plain[:28] - out[:28]) <= bound), what
    print(f"color general |t| {norm:g}: worst error / bound {worst:.3e}" + (f"; step checked at {passed}" if norm > 50.0 else ""))


# ----------------------------------------------------------------------------- c. the robust pass on the gate
def test_robust_follows_the_plain_gate(capi, ctx, lattices, monkeypatch):
    """Huber at scale 1e30 weighs every pair by exactly 1: the robust kernels take the decisions of the plain ones on the gate d
    (min_cos 0.5 ON |c| = 0.5) -- the table's counts -- and their sums lie within 1.5 x the plain bound."""
    for form, pi in (("default", 4), ("heavy", 7)):
        heavy = form == "heavy"
        case = lattices[form]
        t32, n_q, I_q, I_p, G = (case[k] for k in ("target32", "n_q", "I_q", "I_p", "G"))
        md = case["gates"][0]
        T, scan, n_p, tp, dist, idx, c = case["poses"][pi]
        mask = _inside(dist, md)
        tgt = _point_target(capi, ctx, monkeypatch, heavy, t32)
        tgt.set_normals(n_q)
        tgt.set_intensity(I_q, G)
        s = capi.Scan(ctx, scan, flags=capi.FLAG_KEEP_ORDER)
        s.set_normals(n_p)
        s.set_intensity(I_p)
        keep = sc.kept(T, n_p, n_q[idx], mask, 0.5)
        ref, bound, kept = sc.reference(sc.terms(T, scan, tp, t32[idx], n_p, n_q[idx], mask, 0.5), keep)
        assert kept == npc.SYMM_COUNTS[0][npc.MIN_COS.index(0.5)]
        out = capi.symm_linearize_robust(tgt, s, T, md, 0.5, robust=HUBER_ONE)
        w_s, _ = _against(out, ref, 1.5 * bound, kept, ("symm robust", form))
        ref, bound, kept = cc.reference(cc.terms(T, scan, tp, t32[idx], n_q[idx], I_q[idx], G[idx], I_p, mask, 0.968), mask)
        assert kept == pc.POINT_COUNTS_F32[0]
        out = capi.color_linearize_robust(tgt, s, T, md, 0.968, robust=HUBER_ONE)
        w_c, _ = _against(out, ref, 1.5 * bound, kept, ("color robust", form))
        print(f"robust at weights of one, {form}, pose {pi}: error / (1.5 bound) symm {w_s:.3e}, color {w_c:.3e}")
