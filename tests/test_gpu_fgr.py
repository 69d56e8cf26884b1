"""Fast global registration on the GPU (csrc/fgr.hip) against the NumPy restatement of tests/fgr_cases.py: the weights bit
for bit, the 29 sums within the bound of a pass's own summation, sums that do not depend on the grid, the loop as the chain
of its passes and host steps bit for bit, the ends, and the public calls."""
import contextlib
import os

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import fgr_cases as fc
from test_fgr_cases import PUBLIC
from test_gpu_parity import capi, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TILE, W = _capi.FGR_TILE, _capi.FGR_WIDTH
MU_MIN = fc.MAX_DIST ** 2
EPS = 2.0 ** -53


@contextlib.contextmanager
def env(**kv):
    """Environment switches the library reads at every call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def groups(m):
    return -(-(-(-m // TILE)) // W)


def first_k(pred):
    k = 1
    while not pred(TILE * k + 1):
        k += 1
    return k


def blocks_rule(m, cap=1024):
    """The launch rule of the pass (csrc/fgr.hip: fgr_blocks), restated: one block per group of W tiles, at most `cap`."""
    return min(max(groups(m), 1), cap)


def pass_sizes():
    """(m, grid cap or None): the ragged ends of one tile, then 256 k + 1 for the k at which a second block and then a second
    trip of a block's loop first carry live matches -- from the launch rule, which the tests hold against pcr_fgr_blocks.
    Under the default cap a second trip needs more than 2^20 matches; the pass honours PCR_FGR_BLOCKS at every call, so the
    cap is lowered to 2 blocks and the same loop makes its second trip at a size a test can afford."""
    k_block = first_k(lambda m: blocks_rule(m) >= 2)
    k_trip = first_k(lambda m: groups(m) > blocks_rule(m, 2))
    assert (k_block, k_trip) == (W, 2 * W)
    return [(m, None) for m in (1, 2, 3, TILE - 1, TILE, TILE + 1, TILE * k_block + 1)] + [(TILE * k_trip + 1, 2)]


def pairs(m, seed):
    """m matches of the kind of the shared cases (half of them outliers) and a pose of 1 rad to evaluate them at."""
    from point_cloud_registration_amd.math_tools import expSO3
    rng = np.random.default_rng([seed, m])
    src = rng.uniform(-20, 20, (m, 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = expSO3(np.array([0.6, -0.5, 0.62])), [3.0, -4.0, 2.0]
    dst = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, (m, 3))
    out = rng.random(m) < 0.5
    dst[out] = rng.uniform(-20, 20, (int(out.sum()), 3))
    Te = np.eye(4)
    Te[:3, :3], Te[:3, 3] = expSO3(np.array([0.6, -0.5, 0.62]) * 0.9), [2.5, -4.2, 2.2]
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32), Te, rng.integers(0, 5, m).astype(np.int32)


# ---- 1. one pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, cap", pass_sizes())
def test_one_pass_equals_the_restatement(ctx, m, cap):
    src, dst, T, mult = pairs(m, 1)
    worst = 0.0
    with env(PCR_FGR_BLOCKS=cap) if cap else contextlib.nullcontext():
        assert _capi.fgr_blocks(m) == blocks_rule(m, cap or 1024)
        if cap:
            assert groups(m) > _capi.fgr_blocks(m) and groups(m - TILE) <= _capi.fgr_blocks(m - TILE)      # the first size of a second trip
        elif m > TILE * W:
            assert _capi.fgr_blocks(m) == 2 and _capi.fgr_blocks(m - TILE) == 1                           # ... of a second block
        for mu in (fc.mu0_of(src, dst) or 4800.0, 1.0, MU_MIN):                                         # D^2 (one match has no extent: the box's)
            for c in (None, mult):
                out, weight = _capi.fgr_linearize(ctx, src, dst, T, mu, mult=c, want_weight=True)
                assert same_bits(weight, fc.weights(src, dst, T, mu))
                ref, mags = fc.sums(src, dst, T, mu, c)
                bound = m * EPS * mags
                assert np.all(np.abs(out - ref) <= bound), (mu, c is not None, np.abs(out - ref) / np.maximum(bound, 1e-300))
                assert abs(out[28] - ref[0]) <= bound[0] and out[0] == out[6] == out[11] == out[28]
                assert np.all(out[[1, 2, 3, 7, 9, 14]] == 0)
                worst = max(worst, float(np.max(np.abs(out - ref) / np.maximum(bound, 1e-300))))
    print(f"m {m}: largest |sum - fsum| / (m 2^-53 sum|term|) = {worst:.3g}")


# ---- 2. grid independence and determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [TILE * 2 * W + 1, 3000])
def test_sums_do_not_depend_on_the_grid(ctx, m):
    src, dst, T, mult = pairs(m, 2)
    first = _capi.fgr_linearize(ctx, src, dst, T, 1.0, mult=mult)
    assert same_bits(first, _capi.fgr_linearize(ctx, src, dst, T, 1.0, mult=mult))                      # the same call twice
    assert _capi.fgr_blocks(m) == groups(m) > 2
    for cap in (1, 2, 3):
        with env(PCR_FGR_BLOCKS=cap):
            assert _capi.fgr_blocks(m) == cap
            assert same_bits(first, _capi.fgr_linearize(ctx, src, dst, T, 1.0, mult=mult)), cap
            r = _capi.fgr_pose(ctx, src, dst, T, 1.0, 1.0, 1.4, 4, 1, mult=mult, want_trace=True)        # one iteration of the loop
            assert same_bits(first, r["trace"][0, 16:45])


def test_pose_twice_returns_the_same_bits(ctx):
    c = fc.case("B", 1)
    a = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, want_trace=True, **fc.SCHEDULE)
    b = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, want_trace=True, **fc.SCHEDULE)
    with env(PCR_FGR_BLOCKS=1):
        d = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, want_trace=True, **fc.SCHEDULE)
    for o in (b, d):
        assert same_bits(a["T"], o["T"]) and same_bits(a["trace"], o["trace"]) and same_bits(a["weights"], o["weights"])
        assert (a["iterations"], a["status"], a["mu"]) == (o["iterations"], o["status"], o["mu"])


@pytest.mark.parametrize("m, n_tuples, scale, min_edge", [(3, 300, 0.9, 0.0), (40, 4097, 0.9, 0.0), (1000, 4097, 0.95, 2.0), (2, 10, 0.9, 0.0)])
def test_tuples_equal_the_restatement(ctx, m, n_tuples, scale, min_edge):
    import ransac_cases as rc
    src, dst = rc.random_pairs(m, seed=40 + m, inlier_share=0.7)
    want = fc.tuple_mult(src, dst, n_tuples, 3, scale, min_edge)
    got = _capi.fgr_tuples(ctx, src, dst, n_tuples, 3, scale, min_edge)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and got[1] == want[1]
    with env(PCR_FGR_CHUNK=1000):                                                                        # chunks smaller than n_tuples
        again = _capi.fgr_tuples(ctx, src, dst, n_tuples, 3, scale, min_edge)
    assert np.array_equal(again[0], want[0]) and again[1] == want[1]
    if m == 40:
        assert 0 < want[1] < n_tuples


# ---- 3. the loop is its passes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced(ctx):
    c = fc.case("A", 0)
    return c, _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, want_trace=True, **fc.SCHEDULE)


def test_the_loop_is_its_passes(ctx, traced):
    c, r = traced
    n = fc.SCHEDULE["max_iter"]
    assert r["iterations"] == n and r["status"] == 0
    mu = c["mu0"]
    for i in range(n):
        T_i = r["trace"][i, :16].reshape(4, 4)
        assert r["trace"][i, 45] == mu
        assert same_bits(r["trace"][i, 16:45], _capi.fgr_linearize(ctx, c["src"], c["dst"], T_i, mu)), i
        status, T_next = fc.step(r["trace"][i, 16:45], T_i, mu, MU_MIN, 0.0)
        assert status == 0
        assert same_bits(T_next, r["trace"][i + 1, :16].reshape(4, 4) if i + 1 < n else r["T"]), i
        mu = fc.schedule(mu, i, MU_MIN, fc.SCHEDULE["division"], fc.SCHEDULE["period"])
    assert r["mu"] == mu
    assert same_bits(r["weights"], fc.weights(c["src"], c["dst"], r["T"], r["mu"]))


def test_host_loop_equals_the_device_loop(ctx, traced):
    c, r = traced
    h = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, flags=_capi.FLAG_HOST_LOOP, want_trace=True, **fc.SCHEDULE)
    assert same_bits(h["T"], r["T"]) and same_bits(h["weights"], r["weights"]) and same_bits(h["trace"], r["trace"])
    assert (h["iterations"], h["status"], h["mu"]) == (r["iterations"], r["status"], r["mu"])


@pytest.mark.parametrize("flags", [0, _capi.FLAG_HOST_LOOP])
def test_converges_at_the_floor(ctx, flags):
    """tol > 0: once mu has reached mu_min the loop ends at |dx| < tol, the pose of the last step kept.  The restatement
    steps over the device's own sums, so every decision and every bit must agree."""
    c = fc.case("A", 1)
    src, dst = c["src"][c["inlier"]], c["dst"][c["inlier"]]
    args = dict(mu0=4.0, mu_min=1.0, division=2.0, period=1, max_iter=40, tol=1e-9)
    ref = fc.fgr_numpy(src, dst, c["T_true"], gpu_sums=lambda T, mu: _capi.fgr_linearize(ctx, src, dst, T, mu), **args)
    assert ref["status"] == 1 and 2 < ref["iterations"] < 40
    r = _capi.fgr_pose(ctx, src, dst, c["T_true"], args["mu0"], args["mu_min"], args["division"], args["period"], args["max_iter"], tol=args["tol"],
                       flags=flags, want_trace=True)
    assert (r["status"], r["iterations"], r["mu"]) == (1, ref["iterations"], 1.0)
    assert same_bits(r["T"], ref["T"]) and same_bits(r["trace"], ref["trace"]) and same_bits(r["weights"], ref["weights"])
    assert not r["trace"][r["iterations"]:].any()


# ---- 4. ends ----------------------------------------------------------------------------------------------------------------
def test_empty_calls_return_the_start_pose(ctx):
    c = fc.case("A", 0)
    T0 = c["T_true"]
    none = np.zeros((0, 3), np.float32)
    L = _capi.lib()
    for src, dst, max_iter in ((none, none, 10), (c["src"], c["dst"], 0)):
        m = len(src)
        T, it, st, mu = np.full((4, 4), 7.0), _capi.C.c_int(-1), _capi.C.c_int(-1), _capi.C.c_double(-1)
        w, tr = np.full(m, 7.0), np.full((10, 46), 7.0)
        assert L.pcr_fgr_pose(ctx.handle, src, dst, m, None, T0, 9.0, 1.0, 1.4, 4, max_iter, 0.0, 0, T, _capi.C.byref(it), _capi.C.byref(st),
                              _capi.C.byref(mu), _capi._ptr(w), _capi._ptr(tr)) == _capi.PCR_OK
        assert same_bits(T, T0) and (it.value, st.value, mu.value) == (0, 0, 9.0) and np.all(w == 1.0)
        assert not tr[:max_iter].any() and np.all(tr[max_iter:] == 7.0)                     # max_iter rows, none of them written by a pass
    out = np.full(29, 7.0)
    assert L.pcr_fgr_linearize(ctx.handle, none, none, 0, None, T0, 1.0, out, None) == _capi.PCR_OK and not out.any()


@pytest.mark.parametrize("flags", [0, _capi.FLAG_HOST_LOOP])
def test_rank_deficient_systems_are_reported(ctx, flags):
    """One and two matches: integer coordinates, q = p and T = I make every weight 1 and the elimination exact, so the pivot
    is exactly 0 (tests/test_fgr_cases.py confirms it on the restatement): status 2, T_out = T_init."""
    pts = np.float32([[1, 2, 3], [4, -1, 2]])
    for m in (1, 2):
        assert fc.fgr_numpy(pts[:m], pts[:m], np.eye(4), 100.0, 0.01, 1.4, 4, 8)["status"] == 2
        r = _capi.fgr_pose(ctx, pts[:m], pts[:m], np.eye(4), 100.0, 0.01, 1.4, 4, 8, flags=flags, want_trace=True)
        assert (r["status"], r["iterations"], r["mu"]) == (2, 1, 100.0) and same_bits(r["T"], np.eye(4))
        assert np.all(r["weights"] == 1.0) and r["trace"][0, 16] == m and not r["trace"][1:].any()


def test_refusals_leave_outputs_and_context_alone(ctx):
    c = fc.case("A", 0)
    src, dst = c["src"], c["dst"]
    m = len(src)
    L, Cc = _capi.lib(), _capi.C
    I4 = np.eye(4)
    bad_src = src.copy()
    bad_src[5, 1] = np.nan
    bad_mult = np.ones(m, np.int32)
    bad_mult[7] = -1
    good = dict(src=src, dst=dst, m=m, mult=None, mu0=9.0, mu_min=1.0, division=1.4, period=4, max_iter=8)
    cases = [dict(src=bad_src), dict(dst=np.where(np.arange(3 * m).reshape(m, 3) == 4, np.inf, dst).astype(np.float32)), dict(mu0=0.0),
             dict(mu0=np.nan), dict(mu0=np.inf), dict(mu_min=0.0), dict(mu_min=-1.0), dict(division=1.0), dict(division=np.nan), dict(period=0),
             dict(max_iter=-1), dict(mult=bad_mult), dict(m=(1 << 24) + 1)]
    for change in cases:
        a = dict(good, **change)
        T, it, st, mu = np.full((4, 4), 7.0), Cc.c_int(-1), Cc.c_int(-1), Cc.c_double(-1)
        w, tr = np.full(m, 7.0), np.full((8, 46), 7.0)
        rc_ = L.pcr_fgr_pose(ctx.handle, a["src"], a["dst"], a["m"], _capi._ptr(a["mult"]), I4, a["mu0"], a["mu_min"], a["division"], a["period"],
                             a["max_iter"], 0.0, 0, T, Cc.byref(it), Cc.byref(st), Cc.byref(mu), _capi._ptr(w), _capi._ptr(tr))
        assert rc_ == _capi.PCR_ERR_INVALID, change
        assert np.all(T == 7) and np.all(w == 7) and np.all(tr == 7) and (it.value, st.value, mu.value) == (-1, -1, -1), change
    for change in (dict(src=bad_src), dict(mu0=0.0), dict(mu0=np.nan), dict(mult=bad_mult), dict(m=(1 << 24) + 1)):
        a = dict(good, **change)
        out, w = np.full(29, 7.0), np.full(m, 7.0)
        assert L.pcr_fgr_linearize(ctx.handle, a["src"], a["dst"], a["m"], _capi._ptr(a["mult"]), I4, a["mu0"], out, _capi._ptr(w)) == _capi.PCR_ERR_INVALID
        assert np.all(out == 7) and np.all(w == 7), change
    for args in ((bad_src, dst, m, 100, 0.9, 0.0), (src, dst, m, -1, 0.9, 0.0), (src, dst, m, (1 << 26) + 1, 0.9, 0.0), (src, dst, m, 100, 1.5, 0.0),
                 (src, dst, m, 100, 0.9, -1.0)):
        mult, nv = np.full(m, 7, np.int32), Cc.c_int64(-1)
        assert L.pcr_fgr_tuples(ctx.handle, args[0], args[1], args[2], args[3], 0, args[4], args[5], _capi._ptr(mult), Cc.byref(nv)) == _capi.PCR_ERR_INVALID
        assert np.all(mult == 7) and nv.value == -1
    # the next valid call succeeds
    r = _capi.fgr_pose(ctx, src, dst, I4, c["mu0"], MU_MIN, **fc.SCHEDULE)
    assert same_bits(r["T"], _capi.fgr_pose(ctx, src, dst, I4, c["mu0"], MU_MIN, **fc.SCHEDULE)["T"]) and r["iterations"] == 64


# ---- 5. against the restatement end to end ----------------------------------------------------------------------------------
# max |T_gpu - T_numpy| over the eight cases, measured on an MI355X and recorded in docs/EXPERIMENTS.md: POSE_DIFF_MEASURED.
# The bound is 1000 x that and at most 1e-6 -- four orders below the 0.01 m noise of the cases: a difference above it is a
# defect to explain, not a tolerance to widen.
POSE_DIFF_MEASURED = 1.776e-15
POSE_BOUND = min(1000 * POSE_DIFF_MEASURED, 1e-6)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_cases_against_the_restatement(ctx, name, seed):
    c, ref = fc.case(name, seed), fc.reference(name, seed)
    r = _capi.fgr_pose(ctx, c["src"], c["dst"], np.eye(4), c["mu0"], MU_MIN, **fc.SCHEDULE)
    diff = float(np.abs(r["T"] - ref["T"]).max())
    print(f"case {name} seed {seed}: max |T_gpu - T_numpy| = {diff:.3e}, max |w_gpu - w_numpy| = {np.abs(r['weights'] - ref['weights']).max():.3e}")
    assert (r["status"], r["iterations"]) == (ref["status"], ref["iterations"]) and r["mu"] == ref["mu"]
    assert np.array_equal(r["weights"] > 0.5, ref["weights"] > 0.5)
    assert diff <= POSE_BOUND


# ---- 6. through the public call ---------------------------------------------------------------------------------------------
def test_fgr_pose_recovers_case_b():
    c = fc.case("B", PUBLIC["seed"])
    rows = np.arange(len(c["src"]))
    T, info = pcr.fgr_pose(c["src"], c["dst"], rows, rows, fc.MAX_DIST, n_tuples=PUBLIC["n_tuples"], seed=PUBLIC["seed"], return_info=True)
    ang, dt = fc.pose_error(T, c["T_true"])
    print(f"{info['n_valid']} valid tuples, {np.count_nonzero(info['mult'])} rows kept, {ang:.2e} deg, {dt:.4f} m, fitness {info['fitness']:.4f}")
    assert ang <= 0.05 and dt <= 0.1 and info["fitness"] >= 0.19
    assert not (c["inlier"] & ~info["inliers"]).any()                                 # (the restatement leaves none out either: test_fgr_cases.py)
    want = fc.tuple_mult(c["src"], c["dst"], PUBLIC["n_tuples"], PUBLIC["seed"], 0.95, 0.0)
    assert np.array_equal(info["mult"], want[0]) and info["n_valid"] == want[1]
    assert (info["iterations"], info["status"]) == (64, 0) and info["weights"].shape == (len(rows),) and info["count"] == info["inliers"].sum()
    assert np.array_equal(pcr.fgr_pose(c["src"], c["dst"], rows, rows, fc.MAX_DIST, n_tuples=PUBLIC["n_tuples"], seed=PUBLIC["seed"]), T)
    # the filter off: the loop of section 5 behind the same refinement
    T2, info2 = pcr.fgr_pose(c["src"], c["dst"], rows, rows, fc.MAX_DIST, tuple_scale=None, return_info=True)
    assert fc.pose_error(T2, c["T_true"])[0] <= 0.05 and fc.pose_error(T2, c["T_true"])[1] <= 0.1 and np.all(info2["mult"] == 1)


def test_register_global_by_fgr():
    from test_gpu_ransac import E2E, e2e_case
    target, nt, scan, ns, _ = e2e_case()
    kw = dict(normals=(ns, nt), return_info=True)
    Tr, ir = pcr.register_global(scan, target, E2E["radius"], E2E["max_dist"], n_hypotheses=E2E["n_hypotheses"], min_edge=E2E["min_edge"], **kw)
    Tf, inf = pcr.register_global(scan, target, E2E["radius"], E2E["max_dist"], method="fgr", min_edge=E2E["min_edge"], **kw)
    p = scan.astype(np.float64)
    moved = np.linalg.norm((p @ Tf[:3, :3].T + Tf[:3, 3]) - (p @ Tr[:3, :3].T + Tr[:3, 3]), axis=1)
    print(f"register_global: {len(ir['inliers'])} matches; ransac {ir['count']} inliers, fgr {inf['count']} inliers ({inf['n_valid']} valid tuples, "
          f"{np.count_nonzero(inf['mult'])} rows kept); largest displacement between the two {moved.max():.4g}")
    assert moved.max() < E2E["max_dist"]
    # the default method returns what it returned: the same bits without `method` and with method="ransac"
    T1, i1 = pcr.register_global(scan, target, E2E["radius"], E2E["max_dist"], n_hypotheses=E2E["n_hypotheses"], min_edge=E2E["min_edge"],
                                 method="ransac", **kw)
    assert same_bits(T1, Tr) and np.array_equal(i1["inliers"], ir["inliers"]) and i1["hypothesis"] == ir["hypothesis"]
    assert same_bits(i1["pose"].astype(np.float64), ir["pose"].astype(np.float64))
