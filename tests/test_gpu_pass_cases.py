"""One pass of the hot path at the gate boundary and across the pose space (tests/pass_cases.py, g16).

The cases: exact lattices whose probes lie ON the gate (distance exactly 1.25 / 0.3125), on an inner class and on target
records, with gates one ulp either side in float32 and float64, gates whose float32 square underflows or overflows, at nine
exact poses up to |t| = 8192 m; sensor-frame scans at start poses with large rotations and |t| up to 1e4 m; gates placed on the
oracle's own distances.  Every case runs through every launch path on every target form:

  forms   point target as built, without extended lists (PCR_HALO=0), heavy-cell form (PCR_HEAVY=1), PlaneICP over the float64
          array (quirk Q6), voxel target before and after its float32 filter index exists -- asserted through index_info()
  paths   1 fused single launch, 2 search + reduce (voxel targets: float64 search and filter search, equal bits), 3 certified
          reuse forced on one scan handle (same pose, the gate switching from pass to pass), 4 linearize_batch / align_batch,
          5 trace row 0 of pcr_align's device-resident and host-driven loops, 6 the query seam: nn_query of the form's target and, for point forms, KDTree.query of a
          tree built in that form, on the lattice probes at every gate and on the transformed scan of every general pose

Bars (none is new): counts equal to the written-out table and to the oracle; against the oracle rel_H < 1e-9, g within 1e-9 of
max(|H|, |g|), e2 within 1e-9, zero sums where nothing is kept (test_fuzz_against_oracle); equal bits between batch and fused
single, trace row 0 and linearize, reuse passes and search + reduce, nn_mode 0 and 3; fused against search + reduce rtol 1e-11,
atol 1e-9 max|.| (test_tile_handout_covers_every_point_once); against the reference (g16) rel_H < 1e-5, and on the general
poses e2 within 5e-5 and the Gauss-Newton step within 5e-5 (test_gpu_fullsize.py)."""

import ctypes as C

import numpy as np
import pytest

import pass_cases as pc
from conftest import load_golden, rel_H, step_err

pytestmark = pytest.mark.gpu

TOL_REF = 1e-5
INF_GATE = float("inf")
FUSED = dict(variant=0, fuse_finalize=1, nn_mode=0, reuse=0)
SPLIT = dict(variant=1, fuse_finalize=1, nn_mode=0, reuse=0)
SPLIT_F64 = dict(variant=1, fuse_finalize=1, nn_mode=3, reuse=0)
POINT_FORMS = [("default", "icp"), ("default", "plane"), ("halo0", "icp"), ("halo0", "plane"), ("heavy", "icp"), ("heavy", "plane"),
               ("q6", "plane")]
VOXEL_FORMS = [("nofilter", "vplane"), ("nofilter", "ndt"), ("filter", "vplane"), ("filter", "ndt")]
FORMS = POINT_FORMS + VOXEL_FORMS
FORM_IDS = [f"{form}-{kind}" for form, kind in FORMS]


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


@pytest.fixture(scope="module")
def g16():
    g = load_golden("g16_pass_cases.npz")
    return g, pc.build_all(g)


@pytest.fixture
def profiled(ctx):
    """Launch accounting around a test: which kernels of the hot path ran (-> {name: launches})."""
    before = ctx.get_pipeline()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        yield lambda: {k: v[0] for k, v in ctx.profile_read().items()}
    finally:
        ctx.profile_enable(False)
    assert ctx.get_pipeline() == before                    # the shipped selection is back


def _kind(capi, name):
    return {"icp": capi.ICP, "plane": capi.PLANE, "vplane": capi.VPLANE, "ndt": capi.NDT}[name]


# ----------------------------------------------------------------------------- target forms
def _point_target(capi, ctx, monkeypatch, form, t32, t64, normals):
    """A point target in the asked form -- and the assertion that it IS that form."""
    if form == "halo0":
        monkeypatch.setenv("PCR_HALO", "0")
    if form == "heavy":
        monkeypatch.setenv("PCR_HEAVY", "1")
    tgt = capi.Target.points(ctx, t32, normals)
    monkeypatch.delenv("PCR_HALO", raising=False)
    monkeypatch.delenv("PCR_HEAVY", raising=False)
    info = tgt.index_info()
    assert info["n"] == t32.shape[0]
    assert info["heavy"] == (form == "heavy"), (form, info)
    assert (info["halo_records"] == 0) == (form == "halo0"), (form, info)
    if form == "q6":
        assert tgt.set_points_f64(t64) and tgt.has_f64
    return tgt


class _Voxels:
    """The voxel target of a form: ``nofilter`` hands out a fresh target for every use (a search + reduce pass with the filter
    enabled, or the ninth fused pass, would build the float32 filter index) and checks afterwards that none was built;
    ``filter`` is one target whose filter index one search + reduce pass has built."""

    def __init__(self, capi, ctx, form, o_vox, vs, T, scan, kind):
        self.capi, self.ctx, self.form, self.o_vox, self.vs = capi, ctx, form, o_vox, vs
        self.handed = []
        self.shared = None
        if form == "filter":
            self.shared = self._new()
            assert self.shared.index_info()["filter_band"] == 0
            with ctx.pipeline(**SPLIT):
                capi.linearize(self.shared, capi.Scan(ctx, scan), kind, T, 1.0)
            assert self.shared.index_info()["filter_band"] > 0

    def _new(self):
        return self.capi.Target.voxels_from_stats(self.ctx, self.o_vox.mean, self.o_vox.norm, self.o_vox.icov, self.vs)

    def __call__(self):
        if self.shared is not None:
            return self.shared
        self.handed.append(self._new())
        return self.handed[-1]

    def check(self):
        if self.shared is not None:
            assert self.shared.index_info()["filter_band"] > 0
        for t in self.handed:
            assert t.index_info()["filter_band"] == 0
            t.close()
        self.handed = []


# ----------------------------------------------------------------------------- bars
def _vs_oracle(capi, out, oracle, what):
    """The bars of test_fuzz_against_oracle."""
    H, g, e2, cnt = capi.unpack29(out)
    Ho, go, e2o, cnto = oracle
    assert cnt == cnto, (what, cnt, cnto)
    if cnto == 0:
        assert not np.any(out[:28]), what
        return 0.0
    assert rel_H(H, Ho) < 1e-9, (what, rel_H(H, Ho))
    assert np.max(np.abs(g - go)) <= 1e-9 * max(np.max(np.abs(H)), np.max(np.abs(go)), 1e-300), (what, np.max(np.abs(g - go)))
    assert abs(e2 - e2o) <= 1e-9 * max(abs(e2o), 1e-300), (what, e2, e2o)
    return rel_H(H, Ho)


def _vs_reference(capi, out, ref, what, lattice):
    """Against g16: H alone on the lattices (the reference's float32 e2 and g are not pinned there), the bars of
    test_gpu_fullsize.py on the general poses."""
    H, g, e2, cnt = capi.unpack29(out)
    Href, gref, e2ref = ref
    if not Href.any():
        assert cnt == 0 and not np.any(out[:28]), what
        return
    assert rel_H(H, Href) < TOL_REF, (what, rel_H(H, Href))
    if not lattice:
        assert abs(e2 - e2ref) <= 5 * TOL_REF * abs(e2ref), (what, e2, e2ref)
        assert step_err(H, g, Href, gref) <= 5e-5, (what, step_err(H, g, Href, gref))


def _row0(capi, target, scan, kind, T, md, loop):
    """Sums of trace row 0 of pcr_align(max_iter = 1); a singular first solve (nothing kept) is that item's own business."""
    T0 = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    Tout, iters, trace = np.zeros(16), C.c_int(0), np.zeros((1, 45))
    st = capi.lib().pcr_align(target.handle, scan.handle, int(kind), T0, 1, 1e-3, float(md), capi.FLAG_ICP_RR_QUIRK | loop,
                              Tout, C.byref(iters), trace.ctypes.data_as(C.c_void_p))
    assert st in (capi.PCR_OK, capi.PCR_ERR_SINGULAR), capi.lib().pcr_last_error()
    assert iters.value == 1 and np.array_equal(trace[0, :16], T0)
    return trace[0, 16:].copy()


class _Case:
    """What the paths of one (form, kind) share: tgt_for() -> the GPU target, ot the oracle's, tag for messages."""

    def __init__(self, capi, orc, ctx, form, name, tgt_for, ot, tag):
        self.capi, self.orc, self.ctx, self.form, self.name, self.tgt_for, self.ot, self.tag = capi, orc, ctx, form, name, tgt_for, ot, tag
        self.kind = _kind(capi, name)
        # (a voxel target without its filter index keeps it only while no search + reduce pass runs with the filter enabled)
        self.nn_mode = 3 if form == "nofilter" else 0

    def what(self, *more):
        return (self.tag, self.form, self.name) + more


def _single_passes(c, poses, scans, gate_list, expect, ref, lattice):
    """Paths 1, 2 and 5 for every pose x gate -> (fused[(pi, gi)], split[(pi, gi)], worst rel_H against the oracle).
    (Voxel forms: gates of 3 voxels and more -- here 1e19 and above -- make a float64 search walk the row-occupancy bitmap
    instead of the rings (pass_enqueue: md / h + 2 >= 5).  Which traversal ran is not observable in the shipped library: the
    work counters, pcr_nn_counters, exist in the developer build only.  What is pinned is the outcome: nn_mode 3 == nn_mode 0
    == the oracle at those gates.)"""
    capi, ctx = c.capi, c.ctx
    split_pipe = dict(SPLIT, nn_mode=c.nn_mode)
    loops = (capi.FLAG_DEVICE_LOOP, capi.FLAG_HOST_LOOP)
    fused_of, split_of, worst = {}, {}, 0.0
    for gi, md in enumerate(gate_list):
        for pi, (T, scan) in enumerate(poses):
            what = c.what(pi, md)
            tgt = c.tgt_for()
            oracle = c.orc.calc_H_g_e2(c.kind, c.ot, T, scan, md, with_count=True)
            if expect is not None:
                assert oracle[3] == expect[gi], (what, oracle[3], expect[gi])
            with ctx.pipeline(**FUSED):                                           # path 1
                fused = capi.linearize(tgt, scans[pi], c.kind, T, md).copy()
                rows = [_row0(capi, tgt, scans[pi], c.kind, T, md, loop) for loop in loops]
            assert all(np.array_equal(r, fused) for r in rows), (what, "fused: trace row 0 != linearize")         # path 5
            with ctx.pipeline(**split_pipe):                                      # path 2
                split = capi.linearize(tgt, scans[pi], c.kind, T, md).copy()
                rows = [_row0(capi, tgt, scans[pi], c.kind, T, md, loop) for loop in loops]
            assert all(np.array_equal(r, split) for r in rows), (what, "search + reduce: trace row 0 != linearize")
            if c.form == "filter":
                with ctx.pipeline(**SPLIT_F64):
                    assert np.array_equal(split, capi.linearize(tgt, scans[pi], c.kind, T, md)), (what, "nn_mode 0 != nn_mode 3")
            worst = max(worst, _vs_oracle(capi, fused, oracle, what + ("fused",)), _vs_oracle(capi, split, oracle, what + ("split",)))
            assert np.allclose(fused, split, rtol=1e-11, atol=1e-9 * max(np.max(np.abs(split)), 1e-300)), (what, "fused != split")
            if ref is not None:
                _vs_reference(capi, fused, ref(pi, gi), what, lattice)
                _vs_reference(capi, split, ref(pi, gi), what, lattice)
            fused_of[(pi, gi)], split_of[(pi, gi)] = fused, split
    return fused_of, split_of, worst


def _batch_path(c, poses, gate_list, fused_of):
    """Path 4: the poses over one ScanBatch, a 1-point scan among the items; refused on the Q6 form."""
    capi, ctx = c.capi, c.ctx
    one_pt = np.ascontiguousarray(poses[0][1][:1])
    one_scan = capi.Scan(ctx, one_pt)
    batch = capi.ScanBatch(ctx, [scan for _, scan in poses] + [one_pt])
    Ts = np.array([T for T, _ in poses] + [poses[0][0]])
    for gi, md in enumerate(gate_list):
        tgt = c.tgt_for()
        with ctx.pipeline(**FUSED):
            if c.form == "q6":
                with pytest.raises(capi.PcrError, match="float64"):
                    capi.linearize_batch(tgt, batch, c.kind, Ts, md)
                with pytest.raises(capi.PcrError, match="float64"):
                    capi.align_batch(tgt, batch, c.kind, Ts, 1, 1e-3, md)
                continue
            out = capi.linearize_batch(tgt, batch, c.kind, Ts, md)
            for pi in range(len(poses)):
                assert np.array_equal(out[pi], fused_of[(pi, gi)]), c.what(pi, md, "batch != fused single")
            assert np.array_equal(out[-1], capi.linearize(tgt, one_scan, c.kind, Ts[-1], md)), c.what(md, "1-point item")
            _, itb, _, trb = capi.align_batch(tgt, batch, c.kind, Ts, 1, 1e-3, md, want_trace=True)
            assert np.all(itb == 1) and np.array_equal(trb[:, 0, 16:], out), c.what(md, "align_batch row 0")
    batch.close()


def _reuse_path(c, poses, gate_list, split_of):
    """Path 3: certified reuse forced, one scan handle per pose: three passes per gate, then the gate switching between d and
    its successor (and to gates far from the previous one) from pass to pass -- every pass equal to path 2, bit for bit."""
    capi, ctx = c.capi, c.ctx
    seq = [gi for gi in range(len(gate_list)) for _ in range(3)]
    if len(gate_list) == 13:                                 # (d, its float32 successor, d / 2, inf, 1e-30, 1e20, below d)
        seq += [0, 1, 0, 1, 1, 0, 5, 12, 7, 0, 10, 2, 1]
    elif len(gate_list) > 1:                                 # (data-dependent gates come as pairs d_k, successor)
        seq += [0, 1, 0, 1] + list(range(len(gate_list)))[::-1]
    for pi, (T, scan) in enumerate(poses):
        tgt = c.tgt_for()
        sc = capi.Scan(ctx, scan)
        with ctx.pipeline(variant=1, fuse_finalize=1, nn_mode=c.nn_mode, reuse=2):
            for k, gi in enumerate(seq):
                out = capi.linearize(tgt, sc, c.kind, T, gate_list[gi])
                assert np.array_equal(out, split_of[(pi, gi)]), c.what(pi, k, gate_list[gi], "reuse pass != search + reduce",
                                                                        out[28], split_of[(pi, gi)][28], sc.reuse_stats())
            st = sc.reuse_stats()
        if c.form == "q6":                                   # (a float64 search is always a full search)
            assert st["passes_full"] == len(seq) and st["passes_track"] == 0 and st["passes_list"] == 0, st
        else:
            assert st["passes_full"] == 1 and st["passes_track"] == 1 and st["passes_list"] == len(seq) - 2, st


def _run_paths(c, poses, gate_list, expect=None, ref=None, lattice=True):
    """Paths 1-5 for every pose x gate.  expect[gi]: the written-out count or None; ref(pi, gi) -> the reference's (H, g, e2)
    or None.  -> (counts[gi][pi], worst rel_H against the oracle)."""
    scans = [c.capi.Scan(c.ctx, scan) for _, scan in poses]
    fused_of, split_of, worst = _single_passes(c, poses, scans, gate_list, expect, ref, lattice)
    _batch_path(c, poses, gate_list, fused_of)
    _reuse_path(c, poses, gate_list, split_of)
    counts = [[int(round(fused_of[(pi, gi)][28])) for pi in range(len(poses))] for gi in range(len(gate_list))]
    return counts, worst


def _seam(query, pts, do, io, md, f32, what):
    """Path 6: query(pts, md) -> (dist, idx) must give index -1 and distance inf exactly where the oracle's distance is not
    < max_dist (in the type the tree compares in), the oracle's index and distance bit for bit elsewhere."""
    with np.errstate(over="ignore"):
        keep = (do.astype(np.float32) < np.float32(md)) if f32 else (do < md)
    d, i = (np.asarray(x) for x in query(pts, md))
    assert np.array_equal(i[keep], io[keep]) and np.array_equal(d[keep].astype(np.float64), do[keep]), what
    assert np.all(i[~keep] == -1) and np.all(np.isinf(d[~keep])), (what, int(keep.sum()), int((i >= 0).sum()))


def _seam_queries(capi, monkeypatch, form, tgt_for, t32, t64):
    """The doors of the query seam on a form -> [(name, query(pts, md))]: nn_query of the form's own target and, for point
    forms, ``KDTree.query`` of a tree built in that form (a voxel target's centroid index is not built through KDTree)."""
    import point_cloud_registration_amd as pcr
    doors = [("nn_query", lambda pts, md: tgt_for().nn_query(pts, r_max=md))]
    if form in ("default", "halo0", "heavy", "q6"):
        if form == "halo0":
            monkeypatch.setenv("PCR_HALO", "0")
        if form == "heavy":
            monkeypatch.setenv("PCR_HEAVY", "1")
        tree = pcr.KDTree(t64 if form == "q6" else t32)
        monkeypatch.delenv("PCR_HALO", raising=False)
        monkeypatch.delenv("PCR_HEAVY", raising=False)
        info = tree._target.index_info()
        assert info["heavy"] == (form == "heavy") and (info["halo_records"] == 0) == (form == "halo0"), (form, info)
        assert bool(getattr(tree._target, "has_f64", False)) == (form == "q6")
        doors.append(("KDTree.query", lambda pts, md: tree.query(pts, distance_upper_bound=md)))
    return doors


# ----------------------------------------------------------------------------- exact lattices
@pytest.mark.parametrize("form,name", FORMS, ids=FORM_IDS)
def test_lattice_gates(capi, orc, ctx, g16, monkeypatch, profiled, form, name):
    """Every exact pose x gate x path on one target form: the count is the one written out in tests/pass_cases.py."""
    g, built = g16
    if (form, name) in POINT_FORMS:
        lat = built["heavy"] if form == "heavy" else built["pt"]
        case = {"heavy": "heavy", "q6": "pt64"}.get(form, "pt")
        normals = g[f"normals_{case}"]
        tgt = _point_target(capi, ctx, monkeypatch, form, lat["target32"], lat["target64"], normals)
        ot = orc.TargetPoints(lat["target64"] if form == "q6" else lat["target32"], normals=normals, tree_f64=form == "q6")
        table = pc.POINT_COUNTS_F64 if form == "q6" else pc.POINT_COUNTS_F32
        tgt_for, finish = (lambda: tgt), (lambda: None)
    else:
        lat, case, table = built["vox"], "vox", pc.VOXEL_COUNTS
        ot = orc.TargetVoxels(lat["target64"], lat["voxel_size"])
        poses0 = pc.exact_poses(lat["probes"])
        tgt_for = _Voxels(capi, ctx, form, ot, lat["voxel_size"], poses0[0][0], poses0[0][1], _kind(capi, name))
        finish = tgt_for.check
    gates, probes = pc.gates(lat["d"]), lat["probes"]
    poses = pc.exact_poses(probes)
    Href, gref, e2ref = (g[f"lat_{case}_{name}_{k}"] for k in ("H", "g", "e2"))
    c = _Case(capi, orc, ctx, form, name, tgt_for, ot, "lattice")
    counts, worst = _run_paths(c, poses, gates, expect=table, ref=lambda pi, gi: (Href[pi, gi], gref[pi, gi], e2ref[pi, gi]))
    assert all(n == table[gi] for gi, row in enumerate(counts) for n in row)
    # path 6: the query seam (the probes are what every exact pose transforms its scan to)
    f32 = form != "q6" and name in ("icp", "plane")
    do, io = ot.query(probes)
    for door, query in _seam_queries(capi, monkeypatch, form, tgt_for, lat.get("target32"), lat["target64"]):
        for md in gates:
            _seam(query, probes, do, io, md, f32, (form, name, md, door))
    finish()
    prof = profiled()
    if form == "q6":                                         # never the fused kernel, never a certify launch
        assert prof["linearize"] == 0 and prof["nn"] > 0 and prof["reduce"] > 0 and prof["certify"] == 0, prof
    else:
        assert prof["linearize"] > 0 and prof["nn"] > 0 and prof["reduce"] > 0 and prof["certify"] > 0, prof
    print(f"lattice {form}-{name}: worst rel_H against the oracle {worst:.2e}")


# ----------------------------------------------------------------------------- general poses, data-dependent gates
@pytest.mark.parametrize("form,name", FORMS, ids=FORM_IDS)
def test_general_poses(capi, orc, ctx, g16, monkeypatch, profiled, form, name):
    """Sensor-frame scans at start poses with large rotations and |t| in (0, 50, 1e4) m through every path, against the oracle and
    the reference; on one of them, gates placed ON the oracle's own distances: the count at d_k and at its successor is the
    oracle's, and the two differ by the number of scan points at exactly d_k."""
    g, built = g16
    md, vs = pc.GENERAL_MAX_DIST, pc.GENERAL_VOXEL
    worst = 0.0
    for norm, target in built["gen_targets"].items():
        cases = [(ci, c) for ci, c in enumerate(built["gen"]) if c[1] == norm]
        poses = [(T, scan) for _, (_, _, T, scan) in cases]
        if (form, name) in POINT_FORMS:
            normals = g[f"normals_t{norm:g}"]
            t64 = target.astype(np.float64)
            tgt = _point_target(capi, ctx, monkeypatch, form, target, t64, normals)
            ot = orc.TargetPoints(t64 if form == "q6" else target, normals=normals, tree_f64=form == "q6")
            tgt_for, finish = (lambda tgt=tgt: tgt), (lambda: None)
        else:
            ot = orc.TargetVoxels(target, vs)
            tgt_for = _Voxels(capi, ctx, form, ot, vs, poses[0][0], poses[0][1], _kind(capi, name))
            finish = tgt_for.check
        # (the reference ran PlaneICP on the float32 target: its figures pin the float32 forms only)
        ref = None if form == "q6" else (lambda pi, gi: tuple(g[f"gen_{name}_{k}"][cases[pi][0]] for k in ("H", "g", "e2")))
        c = _Case(capi, orc, ctx, form, name, tgt_for, ot, f"general t{norm:g}")
        counts, w = _run_paths(c, poses, [md], ref=ref, lattice=False)
        assert all(0 < n < 1500 for n in counts[0]), counts
        worst = max(worst, w)
        f32 = form != "q6" and name in ("icp", "plane")
        # path 6: the query seam on what each pose transforms its scan to (inexact distances, |q| up to 1e4 m, a grid-searched map)
        doors = _seam_queries(capi, monkeypatch, form, tgt_for, target, target.astype(np.float64))
        for ci, (cname, _, T, scan) in cases:
            st = orc.transform(T, scan)
            do, io = ot.query(st)
            for door, query in doors:
                for r in (md, INF_GATE):
                    _seam(query, st, do, io, r, f32, (form, name, cname, r, door))
            if cname != pc.DATA_GATE_CASE:
                continue
            dg = pc.data_gates(do, f32)
            for door, query in doors:                        # ... and with r_max ON a distance and one ulp above it
                for r, _ in dg:
                    _seam(query, st, do, io, r, f32, (form, name, cname, r, door))
            c = _Case(capi, orc, ctx, form, name, tgt_for, ot, "data gates")
            cnt, w = _run_paths(c, [(T, scan)], [m for m, _ in dg], expect=[n for _, n in dg])
            dd = do.astype(np.float32) if f32 else do
            for k in range(0, len(dg), 2):
                at = int((dd == (np.float32(dg[k][0]) if f32 else dg[k][0])).sum())
                assert at >= 1 and cnt[k + 1][0] - cnt[k][0] == at, (form, name, k, at, cnt[k], cnt[k + 1])
        finish()
    prof = profiled()
    if form == "q6":
        assert prof["linearize"] == 0 and prof["nn"] > 0 and prof["reduce"] > 0 and prof["certify"] == 0, prof
    else:
        assert prof["linearize"] > 0 and prof["nn"] > 0 and prof["reduce"] > 0 and prof["certify"] > 0, prof
    print(f"general {form}-{name}: worst rel_H against the oracle {worst:.2e}")
