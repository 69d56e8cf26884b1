"""The compatibility graph on the GPU (csrc/compat.hip) against the NumPy restatement of tests/compat_cases.py: the bit matrix,
both degrees, the seeds, the consensus sets and their scores are integers and must be EQUAL, through all three entry points;
then sc2_pose end to end at 1.5 % inliers, register_global(method="sc2"), and the PCR_COMPAT_TIMES lines."""
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

import compat_cases as cc
from test_gpu_parity import capi, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def consensus(ctx, c, **over):
    k = dict(n_seeds=c["n_seeds"], k=c["k"])
    k.update(over)
    return _capi.compat_consensus(ctx, c["src"], c["dst"], c["d"], k["n_seeds"], k["k"])


def assert_consensus(got, ref):
    for key in ("deg1", "deg2", "seeds", "members", "scores"):
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, key
        assert np.array_equal(got[key], ref[key]), key


# ---- every case, every entry point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_equals_the_restatement(ctx, name):
    c, ref = cc.cases()[name], cc.reference(name)
    bits = _capi.compat_bits(ctx, c["src"], c["dst"], c["d"])
    assert bits.dtype == np.uint64 and bits.shape == ref["bits"].shape and np.array_equal(bits, ref["bits"])
    deg1, deg2 = _capi.compat_degrees(ctx, c["src"], c["dst"], c["d"])
    assert deg1.dtype == deg2.dtype == np.int64
    assert np.array_equal(deg1, ref["deg1"]) and np.array_equal(deg2, ref["deg2"])
    got = consensus(ctx, c)
    assert_consensus(got, ref)                                  # and with it: consensus agrees with degrees and with bits
    # two calls return the same bytes
    again = consensus(ctx, c)
    assert all(got[key].tobytes() == again[key].tobytes() for key in got)
    assert _capi.compat_bits(ctx, c["src"], c["dst"], c["d"]).tobytes() == bits.tobytes()
    d1, d2 = _capi.compat_degrees(ctx, c["src"], c["dst"], c["d"])
    assert d1.tobytes() == deg1.tobytes() and d2.tobytes() == deg2.tobytes()


@pytest.mark.parametrize("n_seeds, k", [(1, 2), (3, 3), (64, 64), (5000, 20)])
def test_other_seed_counts_and_set_lengths(ctx, n_seeds, k):
    """n_seeds and k cut the same ordered lists short: one seed and one neighbour, every row a seed, the longest set."""
    c = cc.cases()["planted_1000"]
    ref = cc.compat(c["src"], c["dst"], c["d"], n_seeds, k)
    assert_consensus(consensus(ctx, c, n_seeds=n_seeds, k=k), ref)
    assert len(ref["seeds"]) == min(n_seeds, 1000)


def test_python_layer_returns_the_same(ctx):
    c, ref = cc.cases()["planted_129"], cc.reference("planted_129")
    rows = np.arange(129)
    perm = np.random.default_rng(3).permutation(129)
    d1, d2 = pcr.match_compatibility(c["src"][perm], c["dst"], np.argsort(perm), rows, c["d"])
    assert np.array_equal(d1, ref["deg1"]) and np.array_equal(d2, ref["deg2"])
    d1, d2, bits = pcr.match_compatibility(c["src"], c["dst"], rows, rows, c["d"], return_bits=True)
    assert np.array_equal(d1, ref["deg1"]) and np.array_equal(d2, ref["deg2"]) and np.array_equal(bits, ref["bits"])


def test_257_words_on_sampled_rows(ctx):
    """16 402 matches: 257 words a row, the last one a quarter full: five words per lane in k_compat_degrees and, above 16 384
    rows, its form with four rows per wave (the last wave has two), a fifth group of 64 words in k_compat_bits, index
    arithmetic beyond 2^22 words.  The restatement of the whole matrix would take minutes, so: the rows of a sample equal
    the restatement's rows, the matrix is symmetric with an empty diagonal, deg1 is its population count, and deg2 of the
    sampled rows is recomputed from the matrix itself; the sets of the best seeds against the same matrix."""
    m = 16402
    src, dst = cc.planted(m, 200, seed=13)[:2]
    bits = _capi.compat_bits(ctx, src, dst, cc.D)
    assert bits.shape == (m, 257)
    rows = np.r_[0, 1, 63, 64, 4095, 4096, 8191, 8192, 16383, 16384, m - 3, m - 2, m - 1, np.random.default_rng(1).integers(0, m, 20)]
    assert np.array_equal(bits[rows], cc.pack(cc.compat_rows(src, dst, cc.D, rows)))
    C = cc.unpack(bits, m)
    assert np.array_equal(C, C.T) and not C.diagonal().any() and not (bits[:, -1] >> np.uint64(m % 64)).any()
    deg1, deg2 = _capi.compat_degrees(ctx, src, dst, cc.D)
    assert np.array_equal(deg1, C.sum(axis=1)) and np.array_equal(deg2[rows], cc.deg2_of_rows(bits, rows))
    got = _capi.compat_consensus(ctx, src, dst, cc.D, 4, 20)
    assert np.array_equal(got["deg1"], deg1) and np.array_equal(got["deg2"], deg2)
    assert np.array_equal(got["seeds"], np.lexsort((np.arange(m), -deg2))[:4])
    for e, s in enumerate(got["seeds"]):
        cand = np.flatnonzero(C[s])
        sc = cc.popcount(bits[cand] & bits[s])
        order = np.lexsort((cand, -sc))[:19]
        assert np.array_equal(got["members"][e], np.r_[s, cand[order]]) and np.array_equal(got["scores"][e], np.r_[deg1[s], sc[order]])


# ---- the library's refusals -------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    c, ref = cc.cases()["planted_65"], cc.reference("planted_65")
    L, C = _capi.lib(), _capi.C
    src, dst, m = c["src"], c["dst"], 65
    bits, d1, d2 = np.full((m, 2), 7, np.uint64), np.full(m, 7, np.int64), np.full(m, 7, np.int64)
    seeds, members, scores, n_out = np.full(4, 7, np.int32), np.full((4, 5), 7, np.int32), np.full((4, 5), 7, np.int32), C.c_int(7)
    p = _capi._ptr
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert L.pcr_compat_bits(ctx.handle, src, dst, m, bad, p(bits)) == _capi.PCR_ERR_INVALID
        assert L.pcr_compat_degrees(ctx.handle, src, dst, m, bad, p(d1), p(d2)) == _capi.PCR_ERR_INVALID
        assert L.pcr_compat_consensus(ctx.handle, src, dst, m, bad, 4, 5, None, None, p(seeds), p(members), p(scores), C.byref(n_out)) == _capi.PCR_ERR_INVALID
    assert b"d > 0" in L.pcr_last_error()
    for bad_m in (-1, _capi.COMPAT_M_MAX + 1):
        assert L.pcr_compat_bits(ctx.handle, src, dst, bad_m, 0.1, p(bits)) == _capi.PCR_ERR_INVALID
        assert L.pcr_compat_degrees(ctx.handle, src, dst, bad_m, 0.1, p(d1), p(d2)) == _capi.PCR_ERR_INVALID
        assert L.pcr_compat_consensus(ctx.handle, src, dst, bad_m, 0.1, 4, 5, None, None, p(seeds), p(members), p(scores), C.byref(n_out)) == _capi.PCR_ERR_INVALID
    assert b"PCR_COMPAT_M_MAX" in L.pcr_last_error()
    for n_seeds, k in ((4, 1), (4, 65), (0, 5), (-2, 5)):
        assert L.pcr_compat_consensus(ctx.handle, src, dst, m, 0.1, n_seeds, k, None, None, p(seeds), p(members), p(scores), C.byref(n_out)) == _capi.PCR_ERR_INVALID
        assert L.pcr_last_error()
    # a refused call writes nothing
    assert (bits == 7).all() and (d1 == 7).all() and (d2 == 7).all() and (seeds == 7).all() and (members == 7).all() and n_out.value == 7
    # m == 0: PCR_OK, nothing written but the count
    assert L.pcr_compat_bits(ctx.handle, src, dst, 0, 0.1, None) == 0 and L.pcr_compat_degrees(ctx.handle, src, dst, 0, 0.1, None, None) == 0
    assert L.pcr_compat_consensus(ctx.handle, src, dst, 0, 0.1, 4, 5, None, None, p(seeds), p(members), p(scores), C.byref(n_out)) == 0
    assert n_out.value == 0 and (seeds == 7).all() and (scores == 7).all()
    # n_seeds beyond m: clipped, and only so many rows written; the degrees are optional
    big_seeds, big_members, big_scores = np.full(70, 7, np.int32), np.full((70, 5), 7, np.int32), np.full((70, 5), 7, np.int32)
    assert L.pcr_compat_consensus(ctx.handle, src, dst, m, c["d"], 70, 5, None, p(d2), p(big_seeds), p(big_members), p(big_scores), C.byref(n_out)) == 0
    assert n_out.value == 65 and (big_seeds[65:] == 7).all() and (big_members[65:] == 7).all() and np.array_equal(d2, ref["deg2"])
    assert sorted(big_seeds[:65].tolist()) == list(range(65))
    # the context still works
    assert_consensus(consensus(ctx, c), ref)


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cc.E2E["seeds"])
def test_sc2_pose_at_one_and_a_half_per_cent(ctx, seed):
    src, dst, planted, T_true, (T_ref, ref) = cc.e2e_case(seed)
    md = cc.E2E["max_dist"]
    rows = np.arange(len(src))
    T, info = pcr.sc2_pose(src, dst, rows, rows, md, return_info=True)
    found = int((info["inliers"] & planted).sum())
    dt = float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
    print(f"seed {seed}: count {info['count']}, planted found {found} of 30, |dt| {dt:.4g} (restatement {np.linalg.norm(T_ref[:3, 3] - T_true[:3, 3]):.4g}), "
          f"seed row {info['seed']}, planted among the seeds {int(planted[info['seeds']].sum())}")
    assert found >= 27 and dt < md
    for key in ("deg1", "deg2", "seeds", "members", "scores"):
        assert np.array_equal(info[key], ref[key]), key         # the same sets: only the host SVD's rounding is between the poses
    assert info["seed"] == ref["seed"] and info["hypothesis"] == ref["hypothesis"] and info["seed"] == info["seeds"][info["hypothesis"]]
    assert info["counts"].dtype == np.int32 and info["counts"].shape == (64,)
    assert info["count"] == int(info["inliers"].sum()) and info["fitness"] == info["count"] / len(src) and info["n_valid"] == int((info["counts"] >= 0).sum())
    assert info["pose"].dtype == np.float32 and np.abs(T - np.r_[np.c_[info["pose"][:9].reshape(3, 3), info["pose"][9:]], [[0, 0, 0, 1]]]).max() < 1e-6
    # _proper: U D Vt from a float64 SVD.  Three factors orthonormal to a few eps each (eps = 2^-53), two 3 x 3 products to
    # form R and one more to test it, 3 eps a product: some 20 eps in all, 32 eps as the bound -- against the 1e-8 of the
    # float32 rotation it replaces
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 32 * 2.0 ** -53
    again, mask = pcr.score_poses(src, dst, rows, rows, np.r_[np.c_[info["pose"][:9].reshape(3, 3).astype(np.float64), info["pose"][9:]], [[0, 0, 0, 1]]],
                                  md, return_mask=True)
    assert again == info["count"] and np.array_equal(mask, info["inliers"])
    assert np.array_equal(pcr.sc2_pose(src, dst, rows, rows, md), T)               # the same call twice: the same bits


def test_sc2_pose_without_a_set(ctx):
    rng = np.random.default_rng(4)
    P, Q = rng.uniform(-50, 50, (40, 3)).astype(np.float32), rng.uniform(-50, 50, (40, 3)).astype(np.float32)
    for m in (0, 1, 2, 40):                                     # too few matches; 40 unrelated ones at a tiny threshold: no set of 3
        rows = np.arange(m)
        T, info = pcr.sc2_pose(P, Q, rows, rows, 1e-4, return_info=True)
        assert np.array_equal(T, np.eye(4)) and info["count"] == 0 and not info["inliers"].any() and info["rmse"] == np.inf
        assert info["hypothesis"] == -1 and info["seed"] == -1 and info["n_valid"] == 0 and (info["counts"] == -1).all()
        assert info["pose"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and len(info["seeds"]) == min(64, m)


def test_register_global_methods(ctx):
    """method="sc2" is sc2_pose of register_global's own matches; the default and method="ransac" are the same call."""
    from point_cloud_registration_amd.math_tools import expSO3
    from point_cloud_registration_amd.synthetic import street, street_normals
    target = street(3000, seed=3)
    nt = street_normals(target)
    Tt = np.eye(4)
    Tt[:3, :3], Tt[:3, 3] = expSO3(np.array([0.3, -0.5, 1.2])), [4.0, -7.0, 1.5]
    Ti = np.linalg.inv(Tt)
    scan = np.ascontiguousarray(target.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3], dtype=np.float32)
    ns = np.ascontiguousarray(nt.astype(np.float64) @ Ti[:3, :3].T, dtype=np.float32)
    rows = np.arange(0, 3000, 5)
    radius, md = 6.7, 0.3
    fs = pcr.compute_fpfh_rows(scan, rows, ns, radius=radius)
    ft = pcr.compute_fpfh_rows(target, rows, nt, radius=radius)
    ia, ib, _ = pcr.match_features(fs, ft, mutual=True)
    assert len(ia) >= 3
    want_T, want = pcr.sc2_pose(scan, target, rows[ia], rows[ib], md, k=10, return_info=True)
    T, info = pcr.register_global(scan, target, radius, md, normals=(ns, nt), keypoints=(rows, rows), method="sc2", k=10, return_info=True)
    assert np.array_equal(T, want_T) and sorted(info) == sorted(want)
    for key in want:
        assert np.array_equal(np.asarray(info[key]), np.asarray(want[key])), key
    print(f"register_global sc2: {len(ia)} matches, {info['count']} inliers, |dt| {np.linalg.norm(T[:3, 3] - Tt[:3, 3]):.3g}")
    a = pcr.register_global(scan, target, radius, md, normals=(ns, nt), keypoints=(rows, rows), n_hypotheses=2000)
    b = pcr.register_global(scan, target, radius, md, normals=(ns, nt), keypoints=(rows, rows), n_hypotheses=2000, method="ransac")
    assert np.array_equal(a, b) and np.array_equal(a, pcr.ransac_pose(scan, target, rows[ia], rows[ib], md, n_hypotheses=2000))


# ---- the stage times --------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
from point_cloud_registration_amd import _capi
sys.path.insert(0, sys.argv[1])
import compat_cases as cc

def mark(name):
    sys.stderr.flush()
    print("== " + name, file=sys.stderr, flush=True)

c = cc.cases()["planted_129"]
ctx = _capi.get_context(0)
mark("bits")
_capi.compat_bits(ctx, c["src"], c["dst"], c["d"])
mark("degrees")
_capi.compat_degrees(ctx, c["src"], c["dst"], c["d"])
mark("consensus")
_capi.compat_consensus(ctx, c["src"], c["dst"], c["d"], 7, 5)
mark("end")
"""

MS = r"[0-9]+\.[0-9]{4}"


def test_stage_time_lines():
    spec = importlib.util.spec_from_file_location("pcr_tools_timing", os.path.join(REPO, "tools", "timing.py"))
    timing = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(timing)
    env = dict(os.environ, PCR_COMPAT_TIMES="1", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "tests")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    sections, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
            sections[name] = []
        elif line.startswith("pcr_") and name is not None:
            sections[name].append(line)
    expected = {"bits": ("bits m 129 words 3", ["bits_ms"]), "degrees": ("degrees m 129 words 3", ["bits_ms", "degrees_ms"]),
                "consensus": ("consensus m 129 words 3 seeds 7 k 5", ["bits_ms", "degrees_ms", "consensus_ms"])}
    assert sections["end"] == []
    for call, (middle, phases) in expected.items():
        assert len(sections[call]) == 1, (call, sections[call])
        line = sections[call][0]
        assert re.match("^pcr_compat_times " + middle + "".join(f" {p} {MS}" for p in phases) + "$", line), line
        assert line.split(" ", 1)[0] in timing.PREFIXES
        got = timing.phase_ms(line)
        assert [n for n, _ in got] == phases and all(math.isfinite(v) and v >= 0 for _, v in got), line
