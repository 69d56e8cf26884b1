"""The distribution pass behind GICP and VGICP (csrc/match_pass.h, gicp_weight.h) at the gate boundary, across the pose space,
on singular sums, and over scans of more than one stride (tests/dist_cases.py, the clouds of tests/pass_cases.py / g16).

  a  the exact lattices: probes ON the gate, gates one ulp either side in float32 and float64, gates whose float32 square
     underflows or overflows, no gate; 9 exact poses x 13 gates; the counts are the written-out tables of pass_cases.py; at
     one gate per pose the same bits from pcr_*_linearize, the class's calc_H_g_e2 and trace row 0 of pcr_*_align
  b  the 12 general poses (4 rotations, one of pi - 1e-4, |t| in 0 / 50 / 1e4 m), covariances estimated on the GPU and
     read back, and random ones of condition up to 1e6
  c  det == 0 of Cq + R Cp R^T: zero covariances and diag(1, 1, 0) on both sides, one-point neighbourhoods
  d  scans of one, two and three strides of the reduce grid plus a ragged tail: slots 1 and 2 of every lane and the second
     trip of its loop carry live points

Where the restated quantities come from: transformed points from oracle.transform (bit-identical to the kernels' xform:
pass_cases.exact_poses asserts it), matches and float32 distances from oracle.nn_brute, float64 centroid matches from
oracle.nn_brute_f64 over the centroids read back; voxel centroids and covariances are the ones read back from the GPU target.

Bars (none is new): counts compare exactly; every one of the 28 sums lies within gicp_cases.sum_bound, (n_kept + 16 / eps_min)
2^-53 sum |term|, of math.fsum of the restated terms (on the exact degenerate sets the weight is exact: eps_min -> 1);
conftest.step_err <= 1e-10 wherever at least 6 points are kept and H is regular; all 29 outputs exactly zero where nothing is
kept; equal bits between two calls.  "Regular": cond(H_ref) <= 1e6 -- beyond that the rounding of H's own float64 entries
moves a unit step by more than 1e-10, and the bar says nothing about the sums.

What the gate cases hold: the strict comparison of the pass as a whole.  The full search behind pcr_gicp_* / pcr_vgicp_* already
stores "no match" unless sqrt(best) < max_dist on the very distance phase C gates again, so gate_f32 / gate_f64 alone turned
into <= change nothing here (tried: every test passes); with the search's comparison turned as well, the lattice tables fail."""

import numpy as np
import pytest

import dist_cases as dc
import gicp_cases as gc
import pass_cases as pc
from conftest import load_golden, step_err

pytestmark = pytest.mark.gpu

EPS = 1e-3
INF = float("inf")
ROUTE_GATES = (0, 1, 2, 5, 7, 8, 10, 11, 12)       # pose k takes its three routes at gate ROUTE_GATES[k] of pass_cases.gates
REGULAR = 1e6


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
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ----------------------------------------------------------------------------- bars
def _inside(dist, md):
    """The gate in the type of ``dist``: float32 distances against (float)max_dist, float64 ones against max_dist."""
    with np.errstate(over="ignore"):
        return dist < (np.float32(md) if dist.dtype == np.float32 else md)


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


def _check(out, terms, lmin, mask, what, expect=None, exact=False):
    ref, bound, kept = dc.reference(terms, lmin, mask, exact)
    if expect is not None:
        assert kept == expect, (what, "the oracle's mask against the table", kept, expect)
    return _against(out, ref, bound, kept, what)


def _same_bits(out, H, g, e2, cnt, what):
    assert np.array_equal(H[gc.TRIU], out[:21]) and np.array_equal(g, out[21:27]) and e2 == out[27] and cnt == out[28], what


def _routes(linearize, align, reg, tgt, s, T, scan, Cp, md, out, what):
    """The same bits from a second call, from the class and from trace row 0 of the align loop."""
    assert np.array_equal(linearize(tgt, s, T, md), out), (what, "second call")
    reg.max_dist = md
    H, g, e2 = reg.calc_H_g_e2(T, scan, source_cov=Cp)
    _same_bits(out, H, g, e2, reg.last_correspondences, (what, "class"))
    _, iters, trace = align(tgt, s, T, 1, 1e-3, md, want_trace=True)
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


def _gicp_class(monkeypatch, heavy, t32, Cq):
    import point_cloud_registration_amd as pcr
    reg = pcr.GICP()
    if heavy:
        monkeypatch.setenv("PCR_HEAVY", "1")
    reg.set_target(t32, cov=Cq)
    monkeypatch.delenv("PCR_HEAVY", raising=False)
    assert reg._target.index_info()["heavy"] == heavy
    return reg


def _scan(capi, ctx, pts, Cp, flags=None):
    s = capi.Scan(ctx, pts, flags=capi.FLAG_KEEP_ORDER if flags is None else flags)
    if Cp is not None:
        s.set_covariances(Cp)
    return s


def _voxel_side(t):
    """(centroids, covariances) read back from a voxel target, key order: what the pass uses."""
    return t.voxel_stats(("mean",))["mean"], t.get_voxel_covariances()


# ----------------------------------------------------------------------------- a. the gate boundary on the exact lattices
@pytest.mark.parametrize("form", ["default", "heavy"])
def test_gicp_lattice_gates(capi, ctx, orc, built, monkeypatch, form):
    heavy = form == "heavy"
    lat = built["heavy" if heavy else "pt"]
    t32, probes, gates, table = lat["target32"], lat["probes"], pc.gates(lat["d"]), pc.POINT_COUNTS_F32
    Cp, Cq = dc.spd_pair(len(probes), len(t32), seed=21)
    tgt = _point_target(capi, ctx, monkeypatch, heavy, t32)
    tgt.set_covariances(Cq)
    reg = _gicp_class(monkeypatch, heavy, t32, Cq)
    worst, steps = 0.0, 0
    for pi, (T, scan) in enumerate(pc.exact_poses(probes)):
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute(t32, tp)
        terms, lmin = dc.terms_all(T, scan, tp, t32[idx], Cp, Cq[idx], "f32")
        s = _scan(capi, ctx, scan, Cp)
        for gi, md in enumerate(gates):
            what = ("gicp", form, pi, md)
            out = capi.gicp_linearize(tgt, s, T, md)
            w, st = _check(out, terms, lmin, _inside(dist, md), what, expect=table[gi])
            worst, steps = max(worst, w), steps + st
            if gi == ROUTE_GATES[pi]:
                _routes(capi.gicp_linearize, capi.gicp_align, reg, tgt, s, T, scan, Cp, md, out, what)
    print(f"gicp lattice {form}: worst error / bound {worst:.3e}, step checked at {steps} of {9 * len(gates)}")
    assert steps >= 9


@pytest.mark.parametrize("name", ["spd", "raw", "plane"])
def test_vgicp_lattice_gates(capi, ctx, orc, built, name):
    import point_cloud_registration_amd as pcr
    vox = built["vox"]
    probes, gates, table = vox["probes"], pc.gates(vox["d"]), pc.VOXEL_COUNTS
    Cp, cv = dc.spd_pair(len(probes), 64, seed=22)
    cv = cv.astype(np.float64)
    tgt = capi.Target.voxels(ctx, vox["target64"], vox["voxel_size"])
    reg = pcr.VGICP(voxel_size=vox["voxel_size"], eps=EPS, regularization="raw" if name == "raw" else "plane")
    reg.set_target(vox["target64"])
    if name == "spd":
        tgt.set_voxel_covariances(cov=cv)
        reg.set_covariance(cv)
    else:
        tgt.set_voxel_covariances(capi.COV_RAW if name == "raw" else capi.COV_PLANE, EPS)
    mean, Cv = _voxel_side(tgt)
    assert mean.shape == (64, 3) and np.array_equal(mean % 1.0, np.full((64, 3), 0.5))          # every mean IS its centre
    assert np.array_equal(reg.covariance, Cv) and np.array_equal(reg.voxels.mean, mean)
    worst, steps = 0.0, 0
    for pi, (T, scan) in enumerate(pc.exact_poses(probes)):
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute_f64(mean, tp)
        terms, lmin = dc.terms_all(T, scan, tp, mean[idx], Cp, Cv[idx], "f64")
        s = _scan(capi, ctx, scan, Cp)
        for gi, md in enumerate(gates):
            what = ("vgicp", name, pi, md)
            out = capi.vgicp_linearize(tgt, s, T, md)
            w, st = _check(out, terms, lmin, _inside(dist, md), what, expect=table[gi])
            worst, steps = max(worst, w), steps + st
            if gi == ROUTE_GATES[pi]:
                _routes(capi.vgicp_linearize, capi.vgicp_align, reg, tgt, s, T, scan, Cp, md, out, what)
    print(f"vgicp lattice {name}: eps_min {lmin.min():.3e}, worst error / bound {worst:.3e}, step checked at {steps} of {9 * len(gates)}")
    assert steps >= 9


# ----------------------------------------------------------------------------- b. general poses
@pytest.mark.parametrize("norm", pc.GENERAL_NORMS)
def test_gicp_general_poses(capi, ctx, orc, built, norm):
    target, md = built["gen_targets"][norm], pc.GENERAL_MAX_DIST
    cases = [c for c in built["gen"] if c[1] == norm]
    assert len(cases) == 4
    tgt = capi.Target.points(ctx, target)
    Cq_plane = tgt.estimate_covariances(10, capi.COV_PLANE, EPS)
    runs = []
    for name, _, T, scan in cases:
        s = _scan(capi, ctx, scan, None)
        Cp_plane = s.estimate_covariances(10, capi.COV_PLANE, EPS)
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute(target, tp)
        runs.append((name, T, scan, s, Cp_plane, tp, dist, idx))
    Cp_spd, Cq_spd = dc.spd_pair(1500, len(target), seed=23, cond=1e6)
    for label, Cq in (("plane", Cq_plane), ("spd1e6", Cq_spd)):
        if label == "spd1e6":
            tgt.set_covariances(Cq)
        for name, T, scan, s, Cp_plane, tp, dist, idx in runs:
            Cp = Cp_plane
            if label == "spd1e6":
                Cp = Cp_spd
                s.set_covariances(Cp)
            mask = _inside(dist, md)
            terms, lmin = dc.terms_all(T, scan, tp, target[idx], Cp, Cq[idx], "f32")
            out = capi.gicp_linearize(tgt, s, T, md)
            w, st = _check(out, terms, lmin, mask, ("gicp", label, name))
            print(f"gicp {label} {name}: kept {int(mask.sum())}, eps_min {lmin[mask].min():.3e}, error / bound {w:.3e}, step checked {st}")
            assert 0 < mask.sum() <= 1500 and st
            assert np.array_equal(capi.gicp_linearize(tgt, s, T, md), out)


@pytest.mark.parametrize("norm", pc.GENERAL_NORMS)
def test_vgicp_general_poses(capi, ctx, orc, built, norm):
    target, md = built["gen_targets"][norm], pc.GENERAL_MAX_DIST
    cases = [c for c in built["gen"] if c[1] == norm]
    tgt = capi.Target.voxels(ctx, target, pc.GENERAL_VOXEL)
    scans = []
    for name, _, T, scan in cases:
        s = _scan(capi, ctx, scan, None)
        scans.append((s, s.estimate_covariances(10, capi.COV_PLANE, EPS), orc.transform(T, scan)))
    for label, mode in (("raw", capi.COV_RAW), ("plane", capi.COV_PLANE)):
        tgt.set_voxel_covariances(mode, EPS)
        mean, Cv = _voxel_side(tgt)
        for (name, _, T, scan), (s, Cp, tp) in zip(cases, scans):
            dist, idx = orc.nn_brute_f64(mean, tp)
            mask = _inside(dist, md)
            terms, lmin = dc.terms_all(T, scan, tp, mean[idx], Cp, Cv[idx], "f64")
            out = capi.vgicp_linearize(tgt, s, T, md)
            w, st = _check(out, terms, lmin, mask, ("vgicp", label, name))
            print(f"vgicp {label} {name}: kept {int(mask.sum())}, eps_min {lmin[mask].min():.3e}, error / bound {w:.3e}, step checked {st}")
            assert 0 < mask.sum() < 1500 and st
            assert np.array_equal(capi.vgicp_linearize(tgt, s, T, md), out)


# ----------------------------------------------------------------------------- c. the det == 0 rule
def _z_poses(orc, probes):
    """Identity and 90 degrees about z, translation zero: -> [(T, scan)], every scan transformed back to the probes exactly."""
    out = []
    for R in pc.EXACT_ROTATIONS[:2]:
        T = pc.make_T(R, (0.0, 0.0, 0.0))
        scan = pc.sensor_frame(T, probes)
        assert np.array_equal(orc.transform(T, scan), probes)
        out.append((T, scan))
    return out


def test_gicp_singular_sums(capi, ctx, orc, built, monkeypatch):
    import point_cloud_registration_amd as pcr
    lat = built["pt"]
    t32, probes = lat["target32"], lat["probes"]
    n = len(probes)
    tgt = _point_target(capi, ctx, monkeypatch, False, t32)
    for T, scan in _z_poses(orc, probes):
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute(t32, tp)
        everything = np.ones(n, dtype=bool)
        # zero covariances on both sides: every pair is kept and weighs nothing
        Cp, Cq = dc.degenerate_pair(n, len(t32), "zero")
        tgt.set_covariances(Cq)
        s = _scan(capi, ctx, scan, Cp)
        out = capi.gicp_linearize(tgt, s, T, INF)
        assert np.all(np.isfinite(out)) and out[28] == n and not np.any(out[:28]), out
        # diag(1, 1, 0) on both sides: the weight is diag(0, 0, 4e-6), exactly
        Cp, Cq = dc.degenerate_pair(n, len(t32), "disc")
        tgt.set_covariances(Cq)
        s.set_covariances(Cp)
        terms, lmin = dc.terms_all(T, scan, tp, t32[idx], Cp, Cq[idx], "f32")
        assert np.all(lmin == 0.0) and np.any(terms[:, 27] > 0)
        for md in (INF, lat["d"]):
            out = capi.gicp_linearize(tgt, s, T, md)
            w, _ = _check(out, terms, lmin, _inside(dist, md) if md != INF else everything, ("gicp disc", md), exact=True)
            assert out[11] > 0                                # (H[2, 2]: the zz weight of every kept pair)
            print(f"gicp disc, gate {md}: kept {int(out[28])}, error / bound {w:.3e}")
        # one-point neighbourhoods: RAW covariances of k = 1 are exact zeros on both sides
        Cq1 = tgt.estimate_covariances(1, capi.COV_RAW)
        Cp1 = s.estimate_covariances(1, capi.COV_RAW)
        assert Cq1.shape == (len(t32), 6) and Cp1.shape == (n, 6) and not np.any(Cq1) and not np.any(Cp1)
        for gi, md in ((0, lat["d"]), (12, INF)):
            out = capi.gicp_linearize(tgt, s, T, md)
            assert np.all(np.isfinite(out)) and out[28] == pc.POINT_COUNTS_F32[gi] and not np.any(out[:28]), out
    # H = 0: the first solve of the loop is singular, as in test_nothing_inside_the_gate
    Cp, Cq = dc.degenerate_pair(n, len(t32), "zero")
    reg = pcr.GICP(max_dist=INF)
    reg.set_target(t32, cov=Cq)
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(probes, source_cov=Cp)


def test_vgicp_singular_sums(capi, ctx, orc, built):
    import point_cloud_registration_amd as pcr
    vox = built["vox"]
    probes = vox["probes"]
    n = len(probes)
    tgt = capi.Target.voxels(ctx, vox["target64"], vox["voxel_size"])
    for T, scan in _z_poses(orc, probes):
        tp = orc.transform(T, scan)
        Cp, cv = dc.degenerate_pair(n, 64, "zero")
        tgt.set_voxel_covariances(cov=cv.astype(np.float64))
        s = _scan(capi, ctx, scan, Cp)
        out = capi.vgicp_linearize(tgt, s, T, INF)
        assert np.all(np.isfinite(out)) and out[28] == n and not np.any(out[:28]), out
        Cp, cv = dc.degenerate_pair(n, 64, "disc")
        tgt.set_voxel_covariances(cov=cv.astype(np.float64))
        s.set_covariances(Cp)
        mean, Cv = _voxel_side(tgt)
        dist, idx = orc.nn_brute_f64(mean, tp)
        terms, lmin = dc.terms_all(T, scan, tp, mean[idx], Cp, Cv[idx], "f64")
        assert np.all(lmin == 0.0) and np.any(terms[:, 27] > 0)
        for md in (INF, vox["d"]):
            out = capi.vgicp_linearize(tgt, s, T, md)
            w, _ = _check(out, terms, lmin, _inside(dist, md), ("vgicp disc", md), exact=True)
            assert out[11] > 0
            print(f"vgicp disc, gate {md}: kept {int(out[28])}, error / bound {w:.3e}")
    reg = pcr.VGICP(voxel_size=vox["voxel_size"], max_dist=INF)
    reg.set_target(vox["target64"])
    reg.set_covariance(np.zeros((64, 6)))
    with pytest.raises(np.linalg.LinAlgError):
        reg.align(probes, source_cov=np.zeros((n, 6), np.float32))


# ----------------------------------------------------------------------------- d. live slots and the second trip
def test_grid_rule_on_this_device(cus):
    """The sizes below make slots and trips live only while the reduce grid is 8 blocks per CU: a change of the rule shows here."""
    assert dc.stride_points(cus) == 524288, cus


def _tiled_pass(capi, ctx, linearize, tgt, base, n, flags, what):
    """One uploaded scan of ``n`` points repeating the base, at BASE_GATE and at no gate, against ``tiled``."""
    T, scan, Cp, dist, terms, lmin = base
    n0 = len(scan)
    s = _scan(capi, ctx, dc.tile_rows(scan, n), dc.tile_rows(Cp, n), flags)
    try:
        for md in (dc.BASE_GATE, INF):
            mask = _inside(dist, md)
            ref, bound, count = dc.tiled(terms * mask[:, None], mask, n, n0, float(lmin[mask].min()))
            out = linearize(tgt, s, T, md)
            w, st = _against(out, ref, bound, count, what + (md,))
            print(f"{what} gate {md}: kept {count} of {n}, error / bound {w:.3e}, bound / max|H| "
                  f"{bound[:21].max() / np.abs(ref[:21]).max():.3e}, step checked {st}")
            # (no gate: the far tenth of the scan, 500 m out, takes cond(H) past what the step bar covers)
            assert (st or md == INF) and 0 < count and (count < n) == (md != INF)
            if md != INF:
                assert np.array_equal(linearize(tgt, s, T, md), out), (what, "second call")
    finally:
        s.close()


@pytest.fixture(scope="module")
def gicp_base(capi, ctx, orc, built):
    """The point lattice with random covariances and the restated base scan, once."""
    t32 = built["pt"]["target32"]
    T, scan, cls = dc.base_scan("pt")
    Cp, Cq = dc.spd_pair(len(scan), len(t32), seed=24)
    tgt = capi.Target.points(ctx, t32)
    tgt.set_covariances(Cq)
    tp = orc.transform(T, scan)
    dist, idx = orc.nn_brute(t32, tp)
    assert np.array_equal(_inside(dist, dc.BASE_GATE), cls == 0)
    terms, lmin = dc.terms_all(T, scan, tp, t32[idx], Cp, Cq[idx], "f32")
    for a in (scan, Cp, dist, terms, lmin):
        a.setflags(write=False)
    return tgt, (T, scan, Cp, dist, terms, lmin)


@pytest.fixture(scope="module")
def vgicp_base(capi, ctx, orc, built):
    vox = built["vox"]
    T, scan, cls = dc.base_scan("vox")
    Cp, cv = dc.spd_pair(len(scan), 64, seed=25)
    tgt = capi.Target.voxels(ctx, vox["target64"], vox["voxel_size"])
    tgt.set_voxel_covariances(cov=cv.astype(np.float64))
    mean, Cv = _voxel_side(tgt)
    tp = orc.transform(T, scan)
    dist, idx = orc.nn_brute_f64(mean, tp)
    assert np.array_equal(_inside(dist, dc.BASE_GATE), cls == 0)
    terms, lmin = dc.terms_all(T, scan, tp, mean[idx], Cp, Cv[idx], "f64")
    for a in (scan, Cp, dist, terms, lmin):
        a.setflags(write=False)
    return tgt, (T, scan, Cp, dist, terms, lmin)


@pytest.mark.parametrize("order", ["keep_order", "no_scan_sort"])
@pytest.mark.parametrize("k", range(dc.GICP_W))
def test_gicp_live_slots(capi, ctx, cus, gicp_base, k, order):
    """Sizes stride + 257, 2 stride + 257, 3 stride + 513: slot 1, slot 2, then the second trip carry live points."""
    tgt, base = gicp_base
    n = dc.big_sizes(cus, dc.GICP_W)[k]
    flags = capi.FLAG_KEEP_ORDER if order == "keep_order" else capi.FLAG_NO_SCAN_SORT
    _tiled_pass(capi, ctx, capi.gicp_linearize, tgt, base, n, flags, ("gicp", n, order))


@pytest.mark.parametrize("order", ["keep_order", "no_scan_sort"])
@pytest.mark.parametrize("k", range(dc.VGICP_W))
def test_vgicp_live_slots(capi, ctx, cus, vgicp_base, k, order):
    """Sizes stride + 257, 2 stride + 513: slot 1, then the second trip carry live points."""
    tgt, base = vgicp_base
    n = dc.big_sizes(cus, dc.VGICP_W)[k]
    flags = capi.FLAG_KEEP_ORDER if order == "keep_order" else capi.FLAG_NO_SCAN_SORT
    _tiled_pass(capi, ctx, capi.vgicp_linearize, tgt, base, n, flags, ("vgicp", n, order))
