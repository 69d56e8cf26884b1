"""The claims of tests/normal_pass_cases.py, checked with the CPU oracle alone: the exact values of c = n_q . R n_p on the
lattices, the written-out table of kept pairs against the rule and against the oracle's brute-force mask at every exact pose
and for both forms, what the restatement says at c == 0, the colour row of a pair without a tangent gradient, and what negating
a normal does to the restated bits."""
import numpy as np
import pytest

import color_cases as cc
import normal_pass_cases as npc
import pass_cases as pc
import symm_cases as sc


@pytest.fixture(scope="module", params=["default", "heavy"])
def case(request):
    lat = pc.heavy_lattice() if request.param == "heavy" else pc.point_lattice()
    return lat, npc.lattice_case(lat)


def _rank1(J, r):
    return np.concatenate([J[:, sc.TRIU[0]] * J[:, sc.TRIU[1]], J * r[:, None], (r * r)[:, None]], axis=1)


def test_min_cos_sits_on_and_beside_the_values_of_c():
    lo, half, hi = npc.MIN_COS[1:4]
    assert lo < half == 0.5 < hi and np.nextafter(lo, 1.0) == 0.5 and np.nextafter(hi, 0.0) == 0.5
    s, s_hi = npc.MIN_COS[4:6]
    assert s == float(np.float32(0.70710677)) and s < s_hi and np.nextafter(s_hi, 0.0) == s
    assert npc.MIN_COS[0] == 0.0 and npc.MIN_COS[6] == 1.0 and list(npc.MIN_COS) == sorted(npc.MIN_COS)
    assert npc.KINDS.dtype == np.float32 and npc.KINDS.shape == (5, 3)


def test_exact_values_of_c(case):
    """At every exact pose c is one component of a KINDS row, bit for bit: the six values, every one of them taken -- c == 0
    and |c| == 0.5 and |c| == S included -- and the same at every pose."""
    lat, built = case
    first = built["poses"][0][6]
    assert set(first.tolist()) == set(npc.C_VALUES)
    i = np.arange(len(first))
    assert np.array_equal(first, npc.KINDS[i % 5, lat["probe_of"] % 3].astype(np.float64))
    for T, scan, n_p, tp, dist, idx, c in built["poses"]:
        assert np.array_equal(c, first) and n_p.dtype == np.float32
        assert np.array_equal(tp, lat["probes"])
    # each class of distances holds every value of c: the gates and the normal gate cut across each other
    d = npc.probe_classes(lat)
    for dv in (lat["d"], 0.0, lat["d"] / 2):
        assert set(first[d == dv].tolist()) == set(npc.C_VALUES), dv


def test_table_against_rule_and_oracle(case):
    lat, built = case
    assert npc.rule_counts(lat) == npc.SYMM_COUNTS
    assert len(npc.SYMM_COUNTS) == len(built["gates"]) == 13 and all(len(r) == len(npc.MIN_COS) for r in npc.SYMM_COUNTS)
    assert [r[0] for r in npc.SYMM_COUNTS] == pc.POINT_COUNTS_F32
    n_q = built["n_q"]
    for T, scan, n_p, tp, dist, idx, c in built["poses"]:
        assert dist.dtype == np.float32
        with np.errstate(over="ignore"):
            for gi, md in enumerate(built["gates"]):
                mask = dist < np.float32(md)
                got = tuple(int(sc.kept(T, n_p, n_q[idx], mask, mc).sum()) for mc in npc.MIN_COS)
                assert got == npc.SYMM_COUNTS[gi], (gi, got)
    # the counts tell >= from > at 0.5 and at S, and < from <= at the distance gate
    assert npc.SYMM_COUNTS[0][2] > npc.SYMM_COUNTS[0][3] and npc.SYMM_COUNTS[0][4] > npc.SYMM_COUNTS[0][5]
    assert npc.SYMM_COUNTS[0][1] == npc.SYMM_COUNTS[0][2] and npc.SYMM_COUNTS[0] != npc.SYMM_COUNTS[1]


def test_c_zero_takes_the_plus_sign(case):
    """Pairs with c == 0 are kept at min_cos = 0 with s = +1: their restated terms are those of m = 0.5 (n_q + v), and differ from
    those of m = 0.5 (n_q - v) -- so the sums tell c < 0 from c <= 0."""
    lat, built = case
    n_q, t32 = built["n_q"], built["target32"]
    for T, scan, n_p, tp, dist, idx, c in built["poses"][::4]:
        zero = c == 0.0
        assert 0 < zero.sum() < len(c)
        everything = np.ones(len(c), dtype=bool)
        t = sc.terms(T, scan, tp, t32[idx], n_p, n_q[idx], everything, 0.0)
        d = (tp - t32[idx]).astype(np.float64)
        v, nq = sc.rotated(T, n_p), n_q[idx].astype(np.float64)
        plus, minus = (_rank1(*cc.plane_rows(T, scan, 0.5 * (nq + sg * v), d)) for sg in (1.0, -1.0))
        assert np.array_equal(t[zero], plus[zero])
        assert np.all(np.any(plus[zero] != minus[zero], axis=1))


def test_negated_normals_return_the_same_bits(case):
    """Negating any scan or target normal leaves the restated terms of every pair with c != 0 unchanged, bit for bit (s follows
    the sign of c).  At c == 0 there is no sign to follow: c becomes -0, s stays +1 and m becomes 0.5 (n_q - v) -- the one place
    where the objective depends on a normal's sign, which is why those pairs are part of the sums at min_cos = 0 only."""
    lat, built = case
    n_q, t32 = built["n_q"], built["target32"]
    rng = np.random.default_rng(1621)
    flip_p, flip_q = rng.random(len(lat["probes"])) < 0.5, rng.random(len(t32)) < 0.5
    for T, scan, n_p, tp, dist, idx, c in built["poses"]:
        everything = np.ones(len(c), dtype=bool)
        base = sc.terms(T, scan, tp, t32[idx], n_p, n_q[idx], everything, 0.0)
        nonzero = c != 0.0
        for np_, nq_ in ((np.where(flip_p[:, None], -n_p, n_p), n_q), (n_p, np.where(flip_q[:, None], -n_q, n_q)), (-n_p, -n_q)):
            t = sc.terms(T, scan, tp, t32[idx], np_, nq_[idx], everything, 0.0)
            assert np.array_equal(t[nonzero], base[nonzero])
            for mc in npc.MIN_COS[1:]:
                assert np.array_equal(sc.terms(T, scan, tp, t32[idx], np_, nq_[idx], everything, mc),
                                      sc.terms(T, scan, tp, t32[idx], n_p, n_q[idx], everything, mc))
        assert np.array_equal(sc.terms(T, scan, tp, t32[idx], -n_p, -n_q[idx], everything, 0.0), base)     # both: v and n_q flip, m flips, J^T J and J r do not


def test_colour_payload(case):
    lat, built = case
    I_q, I_p, G, n_q = built["I_q"], built["I_p"], built["G"], built["n_q"]
    for a, k in ((I_q, 16), (I_p, 16), (G, 8)):
        assert a.dtype == np.float32 and np.array_equal(a * k, np.round(a * k))
    assert 0.0 <= I_q.min() and I_q.max() < 1.0 and 0.0 <= I_p.min() and I_p.max() < 1.0
    # not tangent: 4 / 5 of the gradients at an x normal and 6 / 7 of those at a z normal have a component along it (at a y
    # normal g_y = ((j % 3) - 1) / 8 = 0), which the pass has to take out
    gn = np.sum(G.astype(np.float64) * n_q, axis=1)
    assert np.mean(gn != 0.0) > 0.5
    idx = built["poses"][0][5]
    assert np.mean(gn[idx] != 0.0) > 0.5


def test_colour_row_without_tangent_gradient(case):
    """A gradient along the normal has no tangent part: m = 0, J_C = 0, r_C = I_q - I_p, and the colour row leaves
    (a_C (I_q - I_p))^2 in e2 alone -- whatever the pose and however far the point is from its match."""
    lat, built = case
    I_q, I_p, n_q, t32 = built["I_q"], built["I_p"], built["n_q"], built["target32"]
    G = (0.375 * n_q).astype(np.float32)
    n = len(lat["probes"])
    for T, scan, n_p, tp, dist, idx, c in built["poses"]:
        for lam in npc.LAMBDAS:
            t = cc.terms(T, scan, tp, t32[idx], n_q[idx], I_q[idx], G[idx], I_p, np.ones(n, dtype=bool), lam)
            colour = t[n:]
            aC = np.sqrt(1.0 - np.float64(lam))
            r = aC * (I_q[idx].astype(np.float64) - I_p.astype(np.float64))
            assert not colour[:, :27].any()
            assert np.array_equal(colour[:, 27], r * r)
            # and the designed gradients, which do have a tangent part, leave more than that
            t2 = cc.terms(T, scan, tp, t32[idx], n_q[idx], I_q[idx], built["G"][idx], I_p, np.ones(n, dtype=bool), lam)
            assert (lam == 1.0) == (not t2[n:, :27].any())


def test_general_inputs():
    n_q, n_p = npc.general_normals(20_000)
    for a in (n_q, n_p):
        assert a.dtype == np.float32 and np.all(np.abs(np.linalg.norm(a.astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22)
    G = npc.general_gradients(20_000)
    assert G.dtype == np.float32 and G.shape == (20_000, 3) and np.all(np.isfinite(G))
    assert np.mean(np.abs(np.sum(G.astype(np.float64) * n_q, axis=1)) > 1e-3) > 0.9             # not tangent
    for norm in pc.GENERAL_NORMS:
        target = pc.general_target(norm)
        I_q, _ = npc.general_intensities(norm, target, target[:10])
        assert I_q.dtype == np.float32 and 0.0 <= I_q.min() and I_q.max() <= 1.0 and I_q.std() > 0.1
    assert npc.away_from_gate(np.array([0.5, 0.2]), [False, True], 0.5) and not npc.away_from_gate(np.array([0.5, 0.2]), [True, True], 0.5)
    assert npc.away_from_gate(np.array([0.0]), [True], 0.0)
