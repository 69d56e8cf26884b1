#!/usr/bin/env python3
"""Generate tests/golden/g14_coreset.npz and g15_coreset_cases.npz by RUNNING the reference's ``caratheodory.py`` on the CPU.

Run in the authoring container only (the reference lives at /root/reference and never travels to the GPU box):

    python tests/golden/make_golden_coreset.py

``caratheodory.py`` and ``math_tools.py`` import nothing but NumPy, so they are loaded straight from their files (the
package's ``__init__`` would pull in pykdtree).  The g2 correspondences come from ``scipy.spatial.cKDTree`` queried the
way ``make_golden.py``'s pykdtree shim does it, and are checked against g2's own ``nn_idx``.

Contents (int64 / float32 / float64 arrays only):
  gn{i}_J, gn{i}_r, gn{i}_P  create_gn_set inputs and the reference's P (as a C-contiguous (M, N) array), i < gn_count:
                             (N, D) in (500, 6), (300, 3), (50, 1) x dtypes (J, r) in (f64, f64), (f32, f32), (f32, f64)
  fc_*                       fast_caratheodory cases: seed, N, D, k, N_target, weighted (u ~ U(0.5, 2) instead of ones;
                             default_rng(seed) draws J, then r, then u), and the reference's own figures on that input:
                             err = max |delta| over H, g, e2; rel = err / max(|H|, |g|, e2); size = len(w); wsum_rel =
                             |sum w - sum u| / sum u; wmin = min w
  pl_*                       the same figures for PlaneICP's Gauss-Newton set of g2 at g2's T (k = 64, N_target = 128),
                             pl_count = correspondences, pl_rel_H = rel_H(H from the full set, g2's T_plane_H),
                             pl_rel_H_coreset = the same for H rebuilt from the coreset
  edge_size                  len(w) of the reference at N_target = M + 1 (seed 0, N = 3000, D = 6, k = 64)

g15_coreset_cases.npz: the reference on every case of tests/coreset_cases.py (every D, uneven blocks, k above the level, the
n_sub branch, weights over many decades, ill-scaled / zero / equal columns, repeated rows, planar scenes, float32 input), drawn
there by the same ``default_rng`` calls the GPU test makes -- only seeds and figures are stored:
  seed, N, M, k, target      the case (in the order of coreset_cases.CASES) and its sizes
  row_rel                    the reference's per-row figure (coreset_cases.per_row_error: fsum, each row against its own magnitude)
  size, wmin, wsum_rel       len(w), min w, |sum w - sum u| / sum u of the reference's coreset
  sv{i}_P                    the reference's P on coreset_cases.special_values() (float32 products that overflow, underflow
                             or are -0.0) cast to the i-th of coreset_cases.TYPE_PAIRS
"""

import importlib.util
import os
import sys
import warnings

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import coreset_cases as cc  # noqa: E402
REFERENCE = "/root/reference/point_cloud_registration"


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REFERENCE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


car = load("caratheodory")
mt = load("math_tools")

FC_CASES = [   # seed, N, D, k, N_target, weighted
    (0, 1_060_000, 6, 64, 128, 0),
    (1, 100_000, 6, 64, 128, 0),
    (2, 3_000, 6, 64, 128, 0),
    (3, 129, 6, 64, 128, 0),
    (5, 30_000, 6, 128, 256, 0),
    (6, 30_000, 6, 32, 64, 0),
    (7, 30_000, 6, 64, 128, 1),
    (8, 30_000, 3, 16, 32, 0),
    (9, 20_000, 3, 64, 128, 1),
]


def draw(seed, n, d, weighted):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((n, d))
    r = rng.standard_normal(n)
    u = rng.uniform(0.5, 2.0, n) if weighted else np.ones(n)
    return J, r, u


def figures(J, r, u, w, idx):
    H, g, e2 = J.T @ (u[:, None] * J), J.T @ (u * r), r @ (u * r)
    Js, rs = J[idx], r[idx]
    Ht, gt, e2t = Js.T @ (w[:, None] * Js), Js.T @ (w * rs), rs @ (w * rs)
    err = max(np.max(np.abs(H - Ht)), np.max(np.abs(g - gt)), abs(e2 - e2t))
    rel = err / max(np.max(np.abs(H)), np.max(np.abs(g)), abs(e2))
    return err, rel, abs(w.sum() - u.sum()) / u.sum(), Ht


def plane_gn_set(g2):
    """PlaneICP's per-correspondence J = [n, p x (R^T n)] and r = n . (p_w - q) at g2's T (plane_icp.py:38-54)."""
    T, src, tgt, nrm = g2["T"], g2["source"], g2["target"], g2["plane_normals"]
    p_w = mt.transform_points(T.astype(np.float32), src)
    d, i = cKDTree(tgt.astype(np.float64)).query(p_w.astype(np.float64))
    d = d.astype(np.float32)
    assert np.array_equal(i, g2["nn_idx"])
    mask = d < float(g2["max_dist"])
    n, q = nrm[i[mask]], tgt[i[mask]]
    r = np.einsum("ij,ij->i", n, p_w[mask] - q)
    Jr = mt.skew_time_vector(src[mask], (T[:3, :3].T @ n.T).T)
    J = np.hstack([n, Jr]).astype(np.float64)
    return J, r.astype(np.float64)


def main_cases():
    cols = {k: [] for k in ("seed", "N", "M", "k", "target", "row_rel", "size", "wmin", "wsum_rel")}
    for fam, name, seed in cc.CASES:
        J, r, u, k, nt = cc.build(name, seed)
        P = np.ascontiguousarray(car.create_gn_set(J, r))
        assert np.array_equal(P.view(np.uint64), cc.gn_set_numpy(J, r).view(np.uint64))
        with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
            warnings.simplefilter("ignore", RuntimeWarning)      # (identical rows, exact planar normals: u / v with v == 0)
            P_sel, w, idx = car.fast_caratheodory(P, u, k, nt)
        rel, exact = cc.per_row_error(P, u, w, idx)
        assert exact and np.all(np.diff(idx) > 0) and np.all(w > 0) and len(w) <= nt and np.array_equal(P_sel, P[:, idx])
        wsum = abs(w.sum() - u.sum()) / u.sum()
        for key, v in zip(cols, (seed, P.shape[1], P.shape[0], k, nt, rel, len(w), w.min(), wsum)):
            cols[key].append(v)
        print(f"{fam:15s} {name:16s} seed {seed}: N {P.shape[1]} M {P.shape[0]} k {k} N_target {nt}: size {len(w)} "
              f"row_rel {rel:.2e} wsum {wsum:.1e} wmin {w.min():.3g}")
    out = {key: np.array(v, dtype=np.float64 if key in ("row_rel", "wmin", "wsum_rel") else np.int64) for key, v in cols.items()}
    J32, r32 = cc.special_values()
    for i, (tj, tr) in enumerate(cc.TYPE_PAIRS):
        with np.errstate(over="ignore", under="ignore"):
            out[f"sv{i}_P"] = np.ascontiguousarray(car.create_gn_set(J32.astype(tj), r32.astype(tr)))
        print(f"special values, J {np.dtype(tj)} r {np.dtype(tr)}: inf {int(np.isinf(out[f'sv{i}_P']).sum())}, "
              f"-0.0 {int((np.signbit(out[f'sv{i}_P']) & (out[f'sv{i}_P'] == 0)).sum())}")
    path = os.path.join(HERE, "g15_coreset_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    out = {}
    i = 0
    for n, d, seed in ((500, 6, 100), (300, 3, 101), (50, 1, 102)):
        rng = np.random.default_rng(seed)
        J64, r64 = rng.standard_normal((n, d)), rng.standard_normal(n)
        for tj, tr in ((np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)):
            J, r = J64.astype(tj), r64.astype(tr)
            out[f"gn{i}_J"], out[f"gn{i}_r"] = J, r
            out[f"gn{i}_P"] = np.ascontiguousarray(car.create_gn_set(J, r))
            i += 1
    out["gn_count"] = np.int64(i)

    cols = {k: [] for k in ("seed", "N", "D", "k", "target", "weighted", "err", "rel", "size", "wsum_rel", "wmin")}
    for seed, n, d, k, nt, weighted in FC_CASES:
        J, r, u = draw(seed, n, d, weighted)
        _, w, idx = car.fast_caratheodory(car.create_gn_set(J, r), u, k, nt)
        err, rel, wsum, _ = figures(J, r, u, w, idx)
        assert np.all(np.diff(idx) > 0) and np.all(w > 0) and len(w) <= nt and rel <= 3e-15 * 2
        for key, v in zip(cols, (seed, n, d, k, nt, weighted, err, rel, len(w), wsum, w.min())):
            cols[key].append(v)
        print(f"fc seed {seed} N {n} D {d} k {k} N_target {nt} weighted {weighted}: size {len(w)} err {err:.2e} rel {rel:.2e} "
              f"wsum {wsum:.1e} wmin {w.min():.3g}")
    for key, v in cols.items():
        out["fc_" + key] = np.array(v, dtype=np.float64 if key in ("err", "rel", "wsum_rel", "wmin") else np.int64)

    g2 = dict(np.load(os.path.join(HERE, "g2_mini_street.npz")))
    J, r = plane_gn_set(g2)
    u = np.ones(len(r))
    _, w, idx = car.fast_caratheodory(car.create_gn_set(J, r), u, 64, 128)
    err, rel, wsum, Ht = figures(J, r, u, w, idx)
    H = J.T @ J
    Href = g2["T_plane_H"]
    out.update(pl_count=np.int64(len(r)), pl_size=np.int64(len(w)), pl_err=np.float64(err), pl_rel=np.float64(rel),
               pl_wsum_rel=np.float64(wsum),
               pl_rel_H=np.float64(np.max(np.abs(H - Href)) / np.max(np.abs(Href))),
               pl_rel_H_coreset=np.float64(np.max(np.abs(Ht - Href)) / np.max(np.abs(Href))))
    print(f"g2 PlaneICP set: {len(r)} correspondences, size {len(w)}, rel {rel:.2e}, rel_H full {out['pl_rel_H']:.2e}, "
          f"coreset {out['pl_rel_H_coreset']:.2e}")

    J, r, u = draw(0, 3000, 6, 0)
    _, w, _ = car.fast_caratheodory(car.create_gn_set(J, r), u, 64, 29)
    out["edge_size"] = np.int64(len(w))
    print("N_target = M + 1:", len(w))

    path = os.path.join(HERE, "g14_coreset.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
    main_cases()
