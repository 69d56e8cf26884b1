"""Gauss-Newton coresets beyond well-conditioned D = 6 input: every instantiation of k_gn_set (D = 1..12 x four type pairs)
and of k_chunk_sums (D = 1..12), float32 products that overflow, underflow or are -0.0, rank-deficient, repeated, ill-scaled
and planar sets, the refusals of the C entry point, and device memory over repeated calls.

Expected values: ``coreset_cases.gn_set_numpy`` (a plain NumPy restatement of create_gn_set, tied here to the reference's P
of g14 and g15 bit for bit) and, for fast_caratheodory, the checks of test_gpu_coreset.check_coreset plus a per-row error
(``coreset_cases.per_row_error``): each row of P against its own magnitude, summed with math.fsum.  The global metric of
test_gpu_coreset.sums_error divides by the largest of |H|, |g|, e2, which checks a row a million times smaller than the
largest a million times more loosely.  g15 (tests/golden/make_golden_coreset.py) holds the reference's figure on every case."""

import numpy as np
import pytest

import coreset_cases as cc
from conftest import load_golden
from test_gpu_coreset import check_coreset

gpu = pytest.mark.gpu

G15 = load_golden("g15_coreset_cases.npz")
# Bound of a family = 10 x the reference's worst per-row figure over the family's cases (g15: row_rel), the margin of
# test_gpu_coreset.REL_BOUND and for the same reason: the two eliminations choose different null vectors (SVD there, pivoted
# QR here) and sum in another order.  The reference's worst figures when g15 was made:
#   every_D 4.5e-16   structure 5.8e-16   weights 5.8e-16   rank_deficient 5.5e-16   repeated_rows 6.0e-16
#   planar_exact 1.3e-15   float32 2.5e-16
#   ill_scaled 6.7e-11      (columns of J differ by 1e3, r by 1e-2: rows of P span ten decades)
#   planar_offset 4.2e-9    (p offset by (1000, -2000, 50): rows of P span twelve decades)
MARGIN = 10.0
ROW_BOUND = {fam: MARGIN * max(float(G15["row_rel"][i]) for i, c in enumerate(cc.CASES) if c[0] == fam) for fam in cc.FAMILIES}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def cast(J, r, tj, tr):
    return np.ascontiguousarray(J.astype(tj)), np.ascontiguousarray(r.astype(tr))


def pair_id(p):
    return f"J{np.dtype(p[0]).name}-r{np.dtype(p[1]).name}"


# ----------------------------------------------------------------------------- A. create_gn_set
def test_restatement_is_the_reference():
    """The NumPy restatement reproduces the reference's P bit for bit: the nine cases of g14 and the special values of g15
    (overflow, underflow, -0.0) in all four type pairs.  Needs no GPU."""
    g14 = load_golden("g14_coreset.npz")
    assert int(g14["gn_count"]) == 9
    for i in range(9):
        P = cc.gn_set_numpy(g14[f"gn{i}_J"], g14[f"gn{i}_r"])
        assert P.shape == g14[f"gn{i}_P"].shape and np.array_equal(bits(P), bits(g14[f"gn{i}_P"])), i
    J32, r32 = cc.special_values()
    for i, (tj, tr) in enumerate(cc.TYPE_PAIRS):
        P = cc.gn_set_numpy(*cast(J32, r32, tj, tr))
        assert np.array_equal(bits(P), bits(G15[f"sv{i}_P"])), pair_id((tj, tr))


def test_g15_matches_the_case_table():
    """The fixture was made from the case table the tests draw from."""
    assert len(G15["seed"]) == len(cc.CASES) and np.array_equal(G15["seed"], [s for _, _, s in cc.CASES])
    assert np.all(G15["row_rel"] > 0) and np.all(G15["size"] <= G15["target"]) and np.all(G15["wmin"] > 0)


@gpu
@pytest.mark.parametrize("pair", cc.TYPE_PAIRS, ids=pair_id)
@pytest.mark.parametrize("d", range(1, 13))
def test_gn_set_every_d_and_type_pair(d, pair):
    """N = 257: one block plus one lane."""
    from point_cloud_registration_amd import create_gn_set
    rng = np.random.default_rng(1000 + d)
    J, r = cast(rng.standard_normal((257, d)), rng.standard_normal(257), *pair)
    P = create_gn_set(J, r)
    assert P.dtype == np.float64 and P.shape == (cc.rows_of(d), 257) and P.flags.c_contiguous
    assert np.array_equal(bits(P), bits(cc.gn_set_numpy(J, r)))


@gpu
@pytest.mark.parametrize("pair", cc.TYPE_PAIRS, ids=pair_id)
@pytest.mark.parametrize("n", [1, 255, 256])
def test_gn_set_block_edges(n, pair):
    from point_cloud_registration_amd import create_gn_set
    rng = np.random.default_rng(1100 + n)
    J, r = cast(rng.standard_normal((n, 6)), rng.standard_normal(n), *pair)
    P = create_gn_set(J, r)
    assert P.shape == (28, n) and np.array_equal(bits(P), bits(cc.gn_set_numpy(J, r)))


@gpu
def test_gn_set_past_the_grid():
    """The grid is capped at 8 blocks of 256 per CU: N = CUs * 8 * 256 + 257 sends the grid-stride loop on a second trip
    with a partial tail."""
    import torch
    from point_cloud_registration_amd import create_gn_set
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = num_cu * 8 * 256 + 257
    rng = np.random.default_rng(1200)
    J, r = cast(rng.standard_normal((n, 2)), rng.standard_normal(n), np.float32, np.float32)
    P = create_gn_set(J, r)
    print(f"{num_cu} CUs, N = {n}")
    assert P.shape == (6, n) and np.array_equal(bits(P), bits(cc.gn_set_numpy(J, r)))


@gpu
@pytest.mark.parametrize("i", range(4), ids=[pair_id(p) for p in cc.TYPE_PAIRS])
def test_gn_set_rounds_once_in_the_input_type(i):
    """float32 x float32 is rounded in float32: +-inf where the product overflows, a subnormal or +-0.0 where it
    underflows; any product with a float64 factor is taken in float64 and stays finite.  A kernel that computed wider and
    rounded afterwards gives other bits on these values."""
    from point_cloud_registration_amd import create_gn_set
    tj, tr = cc.TYPE_PAIRS[i]
    J, r = cast(*cc.special_values(), tj, tr)
    want = cc.gn_set_numpy(J, r)
    nh = 21
    assert not np.isnan(want).any()
    if tj == np.float32:                                  # the inputs do what they are here for
        hh = want[:nh]
        tiny = np.finfo(np.float32).tiny
        assert np.isinf(hh).any() and ((hh != 0) & (np.abs(hh) < tiny)).any() and (hh == 0).any()
        wide = cc.gn_set_numpy(J.astype(np.float64), r.astype(np.float64))
        assert np.mean(bits(want[:nh]) != bits(wide[:nh])) > 0.3
    else:
        assert np.isfinite(want[:nh]).all()
    if tj == np.float64 or tr == np.float64:
        assert np.isfinite(want[nh:nh + 6]).all()
    else:
        assert np.isinf(want[nh:]).any() and (np.signbit(want[nh:]) & (want[nh:] == 0)).any()     # -0.0 in J r
    if tr == np.float64:
        assert np.isfinite(want[-1]).all()
    P = create_gn_set(J, r)
    differ = bits(P) != bits(want)
    print(f"{pair_id((tj, tr))}: inf {int(np.isinf(want).sum())}, -0.0 {int((np.signbit(want) & (want == 0)).sum())}, "
          f"entries that differ {int(differ.sum())} of {differ.size}")
    assert not differ.any(), np.argwhere(differ)[:5]


# ----------------------------------------------------------------------------- B, C. fast_caratheodory
@gpu
@pytest.mark.parametrize("case", range(len(cc.CASES)), ids=cc.CASE_IDS)
def test_fast_caratheodory_case(case):
    from point_cloud_registration_amd import create_gn_set, fast_caratheodory
    fam, name, seed = cc.CASES[case]
    J, r, u, k, nt = cc.build(name, seed)
    P = create_gn_set(J, r)
    assert np.array_equal(bits(P), bits(cc.gn_set_numpy(J, r)))
    assert P.shape == (int(G15["M"][case]), int(G15["N"][case])) and (k, nt) == (int(G15["k"][case]), int(G15["target"][case]))
    P_sel, w, idx = fast_caratheodory(P, u, k, nt)
    check_coreset(P, u, P_sel, w, idx, nt, f"{name} seed {seed}")
    rel, exact = cc.per_row_error(P, u, w, idx)
    print(f"{name} seed {seed}: per-row error {rel:.2e} (reference {float(G15['row_rel'][case]):.2e}, bound of family {fam} "
          f"{ROW_BOUND[fam]:.2e}), size {len(w)} (reference {int(G15['size'][case])}), min w {w.min():.3g} "
          f"(reference {float(G15['wmin'][case]):.3g})")
    assert exact, "a row of P that is zero throughout must be reproduced exactly"
    assert rel <= ROW_BOUND[fam]
    if name == "k_above_level":
        assert len(w) == 128 == int(G15["size"][case])       # the reference returns 128 points here


# ----------------------------------------------------------------------------- E. the entry point itself
@pytest.fixture(scope="module")
def valid():
    """(ctx, P, u, the coreset of (P, u)): M = 28, N = 3000 > N_target = 128, so the call reaches the device."""
    from point_cloud_registration_amd import _capi
    ctx = _capi.get_context()
    rng = np.random.default_rng(1300)
    P = cc.gn_set_numpy(rng.standard_normal((3000, 6)), rng.standard_normal(3000))
    u = rng.uniform(0.5, 2.0, 3000)
    return ctx, P, u, _capi.coreset(ctx, P, u, 64, 128)


def _same_as_before(valid):
    from point_cloud_registration_amd import _capi
    ctx, P, u, before = valid
    after = _capi.coreset(ctx, P, u, 64, 128)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float64 else a,
                                                                            bits(b) if b.dtype == np.float64 else b)


@gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_entry_point_refuses_non_finite_P(valid, bad):
    """Past caratheodory.py's own check: the chunk sums of the first level come back non-finite and the library refuses;
    the next call on the same context returns what it returned before."""
    from point_cloud_registration_amd import _capi
    ctx, P, u, _ = valid
    P = P.copy()
    P[5, 777] = bad
    with pytest.raises(ValueError, match="non-finite"):
        _capi.coreset(ctx, P, u, 64, 128)
    _same_as_before(valid)


@gpu
@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan])
def test_entry_point_refuses_bad_weights(valid, bad):
    from point_cloud_registration_amd import _capi
    ctx, P, u, _ = valid
    u = u.copy()
    u[2999] = bad
    with pytest.raises(ValueError, match="u must be finite and positive"):
        _capi.coreset(ctx, P, u, 64, 128)
    _same_as_before(valid)


@gpu
@pytest.mark.parametrize("k, n_target, m, what", [(29, 128, 28, "k must exceed"), (64, 28, 28, "n_target"), (64, 128, 27, "m must be")])
def test_entry_point_refuses_sizes(valid, k, n_target, m, what):
    from point_cloud_registration_amd import _capi
    ctx, P, u, _ = valid
    with pytest.raises(ValueError, match=what):
        _capi.coreset(ctx, np.ascontiguousarray(P[:m]), u, k, n_target)
    _same_as_before(valid)


@gpu
def test_no_device_memory_growth_over_coreset_calls():
    """create_gn_set + fast_caratheodory twenty times: the pattern and the allowance of
    test_gpu_parity.test_no_device_memory_growth."""
    import gc
    import torch
    from point_cloud_registration_amd import _capi, create_gn_set, fast_caratheodory
    ctx = _capi.get_context(0)
    rng = np.random.default_rng(1400)
    J, r, u = rng.standard_normal((30_000, 6)), rng.standard_normal(30_000), np.ones(30_000)

    def cycle():
        return fast_caratheodory(create_gn_set(J, r), u, 64, 128)

    first = cycle(); gc.collect(); ctx.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        last = cycle()
    gc.collect(); ctx.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 8 * 2 ** 20, (free0 - free1) / 2 ** 20
    for a, b in zip(first, last):
        assert np.array_equal(a, b)
