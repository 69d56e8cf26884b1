"""The NumPy restatement of the compatibility rules (tests/compat_cases.py) against its own invariants, the presence of the
three entry points in the binding, and the argument errors of the Python layer that need no GPU."""
import re

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import compat_cases as cc
from conftest import REPO

SMALL = [n for n in cc.CASE_NAMES if len(cc.cases()[n]["src"]) <= 65] + ["lattice_on", "nan_row", "duplicates"]


def test_case_list_is_complete():
    assert tuple(cc.cases()) == cc.CASE_NAMES
    sizes = {len(c["src"]) for c in cc.cases().values()}
    assert {0, 1, 2, 3, 63, 64, 65, 127, 129, 1000, 2500} <= sizes and max(sizes) > 4096


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_restatement_invariants(name):
    c, ref = cc.cases()[name], cc.reference(name)
    m = len(c["src"])
    C, bits = ref["C"], ref["bits"]
    assert C.shape == (m, m) and bits.shape == (m, (m + 63) // 64) and bits.dtype == np.uint64
    assert np.array_equal(C, C.T) and not C.diagonal().any()
    assert np.array_equal(cc.unpack(bits, m), C)
    if m % 64:                                                  # the padding bits of the last word
        assert not (bits[:, -1] >> np.uint64(m % 64)).any()
    assert np.array_equal(ref["deg1"], cc.popcount(bits)) and ref["deg1"].dtype == ref["deg2"].dtype == np.int64
    rows = np.arange(m) if m <= 130 else np.arange(0, m, 97)
    assert np.array_equal(ref["deg2"][rows], cc.deg2_of_rows(bits, rows))
    s = min(c["n_seeds"], m)
    assert ref["seeds"].shape == (s,) and ref["members"].shape == ref["scores"].shape == (s, c["k"])
    assert len(set(ref["seeds"].tolist())) == s
    key = list(zip((-ref["deg2"][ref["seeds"]]).tolist(), ref["seeds"].tolist()))
    assert key == sorted(key) and (s == m or max(key) <= min((-ref["deg2"][i], i) for i in set(range(m)) - set(ref["seeds"].tolist())))
    for e, row in enumerate(ref["seeds"]):
        mem, sc = ref["members"][e], ref["scores"][e]
        n = int((mem >= 0).sum())
        assert mem[0] == row and sc[0] == ref["deg1"][row] and n == min(c["k"], 1 + ref["deg1"][row])
        assert (mem[n:] == -1).all() and (sc[n:] == -1).all() and (sc[:n] >= 0).all()
        assert C[row, mem[1:n]].all() and len(set(mem[:n].tolist())) == n
        order = list(zip((-sc[1:n]).tolist(), mem[1:n].tolist()))
        assert order == sorted(order)                           # by score descending, ties to the smaller row


@pytest.mark.parametrize("name", SMALL)
def test_deg2_is_the_triple_loop(name):
    ref = cc.reference(name)
    if len(ref["C"]) <= 65:
        assert np.array_equal(ref["deg2"], cc.deg2_brute(ref["C"]))
    else:
        rows = slice(0, 12)
        C = ref["C"]
        assert np.array_equal(ref["deg2"][rows], [sum(int((C[i] & C[j]).sum()) for j in np.flatnonzero(C[i])) for i in range(12)])


def test_lattice_sits_on_the_threshold():
    src, dst, t, s, u = cc.lattice()
    on, below = cc.reference("lattice_on")["C"], cc.reference("lattice_below")["C"]
    dt, ds = np.abs(t[:, None] - t[None, :]), np.abs(s[:, None] - s[None, :])
    plain = (u[:, None] == 0) & (u[None, :] == 0) & ~np.eye(len(t), dtype=bool)
    la, lb = cc.lengths(src), cc.lengths(dst)
    assert np.array_equal(la[plain], 5.0 * dt[plain]) and np.array_equal(lb, 5.0 * ds)          # exact lengths
    edge = plain & (np.abs(dt - ds) == 1)
    assert edge.sum() > 100
    assert on[edge].all() and not below[edge].any()             # <=, and one ulp of d decides
    exact = (np.abs(la - lb) == 5.0) & ~np.eye(len(t), dtype=bool)                            # (some pairs off the line land there too)
    assert (below <= on).all() and np.array_equal(on & ~below, exact) and (edge <= exact).all()
    assert np.array_equal(on[plain], (np.abs(dt - ds) <= 1)[plain])


def test_special_cases_are_what_they_claim():
    nan = cc.reference("nan_row")
    assert not nan["C"][7].any() and not nan["C"][:, 7].any() and nan["deg1"][7] == 0 and nan["deg2"][7] == 0
    assert nan["deg1"].max() > 30
    dup = cc.reference("duplicates")
    assert dup["C"][30:50, 30:50].sum() == 20 * 19                                            # a2 = b2 = 0: compatible
    outside = np.r_[0:30, 50:100]
    assert len(set(dup["deg2"][30:50].tolist())) == 1 and (dup["C"][30:50][:, outside] == dup["C"][30, outside]).all()
    ties = sum(len(sc[sc >= 0]) - len(set(sc[sc >= 0].tolist())) for sc in dup["scores"])
    assert ties > 100                                                                         # both tie rules have work to do
    dense = cc.reference("dense_200")
    assert dense["deg1"].mean() > 150 and dense["deg2"].mean() > 0.5 * 199 * 198 and (dense["members"] >= 0).all()
    more = cc.reference("more_seeds_than_rows")
    assert more["seeds"].shape == (65,) and sorted(more["seeds"].tolist()) == list(range(65))
    short = cc.reference("k_beyond_the_sets")
    assert ((short["members"] >= 0).sum(axis=1) < cc.K_MAX).all() and (short["members"][:, -1] == -1).all()


@pytest.mark.parametrize("seed", cc.E2E["seeds"])
def test_restatement_recovers_the_planted_pose(seed):
    """What the GPU test of sc2_pose is measured against: the restatement alone finds all 30 planted matches of the 2 000,
    the translation within 0.014."""
    src, dst, planted, T_true, (T, info) = cc.e2e_case(seed)
    dt = float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
    print(f"seed {seed}: count {info['count']}, planted found {int((info['inliers'] & planted).sum())}, |dt| {dt:.4g}, "
          f"|dR| {np.linalg.norm(T[:3, :3] - T_true[:3, :3]):.4g}, planted seeds {int(planted[info['seeds']].sum())} of {len(info['seeds'])}")
    assert planted.sum() == 30 and (info["inliers"] & planted).sum() == 30
    assert dt <= 0.014


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_prototypes_and_abi():
    header = open(f"{REPO}/include/pcr.h").read()
    for name in ("pcr_compat_bits", "pcr_compat_degrees", "pcr_compat_consensus"):
        assert name in _capi.PROTOTYPES and re.search(r"PCR_API\s+pcr_status\s+%s\s*\(" % name, header)
    assert _capi.ABI_VERSION == 5 and re.search(r"#define\s+PCR_ABI_VERSION\s+5\b", header)
    assert int(re.search(r"#define\s+PCR_COMPAT_M_MAX\s+(\d+)", header).group(1)) == _capi.COMPAT_M_MAX == cc.M_MAX
    assert int(re.search(r"#define\s+PCR_COMPAT_K_MAX\s+(\d+)", header).group(1)) == _capi.COMPAT_K_MAX == cc.K_MAX
    for name in ("match_compatibility", "sc2_pose"):
        assert name in pcr.__all__ and callable(getattr(pcr, name))


def test_argument_errors_need_no_gpu():
    rng = np.random.default_rng(0)
    P, Q = rng.normal(size=(50, 3)).astype(np.float32), rng.normal(size=(50, 3)).astype(np.float32)
    rows = np.arange(50)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            pcr.match_compatibility(P, Q, rows, rows, bad)
        with pytest.raises(ValueError):
            pcr.sc2_pose(P, Q, rows, rows, 0.1, compat_dist=bad)
    for kw in (dict(k=1), dict(k=65), dict(k=2.5), dict(n_seeds=0), dict(n_seeds=-3), dict(refine_rounds=-1)):
        with pytest.raises(ValueError):
            pcr.sc2_pose(P, Q, rows, rows, 0.1, **kw)
    with pytest.raises(ValueError):
        pcr.sc2_pose(P, Q, rows, rows[:-1], 0.1)
    with pytest.raises(ValueError):
        pcr.sc2_pose(P, Q, rows, rows + 1, 0.1)
    with pytest.raises(ValueError):
        pcr.sc2_pose(P, Q, rows, rows, -0.1)
    many = np.zeros(_capi.COMPAT_M_MAX + 1, np.int64)
    for fn in (pcr.sc2_pose, pcr.match_compatibility):
        with pytest.raises(ValueError) as e:
            fn(P, Q, many, many, 0.1)
        for word in ("32768", 'keypoints="iss"', "mutual=True", "ratio="):
            assert word in str(e.value)
    with pytest.raises(ValueError):
        _capi.compat_bits(None, np.zeros((_capi.COMPAT_M_MAX + 1, 3), np.float32), np.zeros((_capi.COMPAT_M_MAX + 1, 3), np.float32), 0.1)
    with pytest.raises(ValueError):
        pcr.register_global(P, Q, 1.0, 0.1, method="sc3")
    # no matches: nothing to compute, no GPU needed
    none = np.zeros(0, np.int64)
    d1, d2, bits = pcr.match_compatibility(P, Q, none, none, 0.1, return_bits=True)
    assert d1.shape == d2.shape == (0,) and d1.dtype == d2.dtype == np.int64 and bits.shape == (0, 0) and bits.dtype == np.uint64
