"""The claims of tests/dist_cases.py, checked with the CPU oracle alone: the gate tables of tests/pass_cases.py hold for the
distances the GICP / VGICP restatement takes its masks from, the degenerate covariance sets sum exactly and invert by the
det == 0 rule, the closed-form weight agrees with numpy.linalg.inv on regular sums, ``tiled`` equals the direct restatement of
a materialised scan, the base scans keep their distance from the gate, and the grid rule is restated correctly."""
import numpy as np
import pytest

import dist_cases as dc
import gicp_cases as gc
import pass_cases as pc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _counts(dist, gates, f32):
    with np.errstate(over="ignore"):
        return [int((dist < (np.float32(md) if f32 else md)).sum()) for md in gates]


@pytest.mark.parametrize("which", ["pt", "heavy", "vox"])
def test_gate_tables_at_every_exact_pose(orc, which):
    """The float32 distances of orc.nn_brute (point lattices) and the float64 ones of orc.nn_brute_f64 over the centroids (voxel
    lattice) give the written-out tables at all 9 exact poses."""
    lat = {"pt": pc.point_lattice, "heavy": pc.heavy_lattice, "vox": pc.voxel_lattice}[which]()
    gates = pc.gates(lat["d"])
    for T, scan in pc.exact_poses(lat["probes"]):
        tp = orc.transform(T, scan)
        if which == "vox":
            dist = orc.nn_brute_f64(orc.TargetVoxels(lat["target64"], 1.0).mean, tp)[0]
            assert dist.dtype == np.float64 and _counts(dist, gates, False) == pc.VOXEL_COUNTS
        else:
            dist = orc.nn_brute(lat["target32"], tp)[0]
            assert dist.dtype == np.float32 and _counts(dist, gates, True) == pc.POINT_COUNTS_F32


def test_voxel_lattice_raw_covariances(orc):
    """64 kept voxels, every mean its centre, raw covariance eigenvalues in [0.0142, 0.0199]: RAW sums are regular."""
    vox = orc.TargetVoxels(pc.voxel_lattice()["target64"], 1.0)
    lam = np.linalg.eigvalsh(vox.cov)
    assert vox.mean.shape == (64, 3) and np.array_equal(vox.mean % 1.0, np.full((64, 3), 0.5))
    assert 0.0142 <= lam.min() and lam.max() <= 0.0199, (lam.min(), lam.max())


def test_degenerate_sums_are_exact(orc):
    """Cq + R Cp R^T of the degenerate sets is the same float64 matrix in any order of evaluation at the two rotations about z,
    and oracle.calc_icov applies the det == 0 rule to it."""
    assert np.array_equal(orc.calc_icov(np.diag([2.0, 2.0, 0.0])[None])[0], dc.DISC_WEIGHT)
    assert np.array_equal(orc.calc_icov(np.zeros((1, 3, 3)))[0], np.zeros((3, 3)))
    for R in pc.EXACT_ROTATIONS[:2]:
        for which, total in (("zero", np.zeros((3, 3))), ("disc", np.diag([2.0, 2.0, 0.0]))):
            Cp, Cq = dc.degenerate_pair(1, 1, which)
            P, Q = gc.full3(Cp)[0], gc.full3(Cq)[0]
            for S in (Q + (R @ P) @ R.T, Q + R @ (P @ R.T), (R @ P) @ R.T + Q, Q + np.einsum("ij,jk,lk->il", R, P, R)):
                assert np.array_equal(S, total), (which, R)
            M, lmin = dc.weights_closed(pc.make_T(R, (0, 0, 0)), Cp, Cq)
            assert np.array_equal(M[0], dc.DISC_WEIGHT if which == "disc" else np.zeros((3, 3))) and lmin[0] == 0.0
            assert np.all(np.isfinite(M))


@pytest.mark.parametrize("cond", [100.0, 1e6])
def test_closed_form_weight_is_the_inverse_on_regular_sums(cond):
    """Against numpy.linalg.inv of the same summed matrix.  The determinant is a difference of products of size l_max^3 that
    comes to l_min l_mid l_max: per matrix the closed form may lose (l_max / l_min)^2 roundings, 8 of them allowed each.  At
    condition 100 that is 1e-11; at 1e6 it is what keeps the restatement from using numpy.linalg.inv (measured: 1.3e-8)."""
    Cp, Cq = dc.spd_pair(500, 500, seed=11, cond=cond)
    T = dc.base_pose()
    M, lmin = dc.weights_closed(T, Cp, Cq)
    S = dc.summed(T, Cp, Cq)
    lam = np.linalg.eigvalsh(S)
    assert np.array_equal(S, S.transpose(0, 2, 1)) and np.array_equal(lam[:, 0], lmin) and lmin.min() >= 2e-2 * (1 - 1e-6)
    assert np.max(np.abs(S - (gc.full3(Cq) + np.einsum("ij,njk,lk->nil", T[:3, :3], gc.full3(Cp), T[:3, :3])))) <= 4 * gc.EPS53 * lam.max()
    Minv = np.linalg.inv(S)
    err = np.max(np.abs(M - Minv), axis=(1, 2)) / np.max(np.abs(Minv), axis=(1, 2))
    print(f"cond {cond:g}: max relative difference {err.max():.3e}, largest l_max / l_min {np.max(lam[:, 2] / lam[:, 0]):.3e}")
    assert np.all(err <= 8 * (lam[:, 2] / lam[:, 0]) ** 2 * gc.EPS53)
    if cond == 100.0:
        assert err.max() <= 1e-11


def _base_restated(orc, which):
    T, scan, cls = dc.base_scan(which)
    tp = orc.transform(T, scan)
    if which == "pt":
        tgt = pc.point_lattice()["target32"]
        dist, idx = orc.nn_brute(tgt, tp)
        residual = "f32"
    else:
        tgt = orc.TargetVoxels(pc.voxel_lattice()["target64"], 1.0).mean
        dist, idx = orc.nn_brute_f64(tgt, tp)
        residual = "f64"
    Cp, Cq = dc.spd_pair(len(scan), len(tgt), seed=12)
    return T, scan, cls, tp, tgt, dist, idx, Cp, Cq, residual


@pytest.mark.parametrize("which", ["pt", "vox"])
def test_base_scan_keeps_away_from_the_gate(orc, which):
    T, scan, cls, tp, tgt, dist, idx, Cp, Cq, residual = _base_restated(orc, which)
    rel = np.abs(dist.astype(np.float64) / dc.BASE_GATE - 1.0)
    print(f"{which}: nearest distance to the gate {rel.min():.3f} relative; classes {np.bincount(cls)}")
    assert rel.min() >= 1e-3
    assert np.array_equal(dist < dc.BASE_GATE, cls == 0) and np.bincount(cls).tolist() == [1600, 200, 200]
    assert np.all(dist[cls == 1] < 1.7) and np.all(dist[cls == 2] > 400.0)
    # distinct points with distinct covariances, and 524 288 % 2000 != 0: the slots of a lane hold different base points
    assert len(np.unique(scan, axis=0)) == len(scan) and len(np.unique(Cp, axis=0)) == len(Cp)
    assert dc.stride_points(256) % dc.BASE_N0 == 288


@pytest.mark.parametrize("which", ["pt", "vox"])
def test_tiled_equals_the_direct_restatement(orc, which):
    """A materialised scan of 5000 points (two and a half repeats of the base) restated point by point, against ``tiled``:
    equal counts; sums within the rounding of the products terms * multiplicity, 2^-53 sum |term|, and of the two results."""
    T, scan, cls, tp, tgt, dist, idx, Cp, Cq, residual = _base_restated(orc, which)
    n, n0 = 5000, len(scan)
    for gate in (dc.BASE_GATE, float("inf")):
        mask = dist < gate
        t0, eps_min = dc.terms_closed(T, scan, tp, tgt[idx], Cp, Cq[idx], mask, residual)
        ref, bound, count = dc.tiled(t0, mask, n, n0, eps_min)
        big = dc.tile_rows(scan, n)
        tpb = orc.transform(T, big)
        db, ib = (orc.nn_brute if which == "pt" else orc.nn_brute_f64)(tgt, tpb)
        tb, eps_b = dc.terms_closed(T, big, tpb, tgt[ib], dc.tile_rows(Cp, n), Cq[ib], db < gate, residual)
        direct, mag = gc.fsum_cols(tb)
        assert count == int((db < gate).sum()) == (2 * mask.sum() + mask[:1000].sum()) and eps_b == eps_min
        assert np.all(np.abs(ref - direct) <= 4 * gc.EPS53 * mag)
        assert np.array_equal(bound, gc.sum_bound(count, eps_min, gc.fsum_cols(t0 * np.bincount(np.arange(n) % n0)[:, None])[1]))


def test_grid_rule():
    assert dc.stride_points(256) == 524288
    assert dc.big_sizes(256, dc.GICP_W) == (524288 + 257, 2 * 524288 + 257, 3 * 524288 + 513)
    assert dc.big_sizes(256, dc.VGICP_W) == (524288 + 257, 2 * 524288 + 513)
