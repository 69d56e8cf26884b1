"""The four aligners over the fixtures of tests/test_gpu_robust.py, for tests/test_gpu_trim.py: g2_mini_street with random unit
scan normals (SymmetricICP) or random gradients and scan intensities (ColoredICP), 1823 of 2000 kept; the point / voxel lattice
of g16_pass_cases with random covariances and dist_cases.base_scan (GICP, VGICP), 1600 of 2000 kept at gate 1.  The restated
unweighted terms are those of symm_cases / color_cases / dist_cases through robust_cases; the end-to-end aligners are those of
robust_cases.e2e_case."""

import numpy as np

import color_cases as cc
import dist_cases as dc
import gicp_cases as gc
import pass_cases as pc
import robust_cases as rc
import symm_cases as sc
import trim_cases as tc
from conftest import load_golden

ALIGNERS = ("symm", "color", "gicp", "vgicp")
# points per lane in flight: the robust kernels', which the adaptive reduce keeps, and the plain kernels'
ROBUST_W = {"symm": 2, "color": 2, "gicp": 3, "vgicp": 2}
PLAIN_W = {"symm": 3, "color": 2, "gicp": 3, "vgicp": 2}
LAMBDA = 0.968


class Side:
    """One aligner over its base scan: the device target, the restated unweighted terms t (m N0, 28) -- zero rows outside the
    gates --, keep (N0,), and how to upload a scan of rows of the base, or other points, with the payload."""

    def __init__(self, name, capi, ctx, tgt, T, md, scan, payload, extra, t, keep, bound, subset):
        self.name, self.capi, self.ctx, self.tgt, self.T, self.md = name, capi, ctx, tgt, T, md
        self.scan, self.payload, self.extra = scan, payload, extra
        self.t, self.keep, self.bound, self.subset = t, keep, bound, subset
        self.m = 2 if name == "color" else 1
        for a in (self.t, self.keep):
            a.setflags(write=False)

    def upload_points(self, pts, payload, flags=None):
        s = self.capi.Scan(self.ctx, np.ascontiguousarray(pts), flags=self.capi.FLAG_KEEP_ORDER if flags is None else flags)
        setter = {"symm": s.set_normals, "color": s.set_intensity, "gicp": s.set_covariances, "vgicp": s.set_covariances}[self.name]
        setter(np.ascontiguousarray(payload))
        return s

    def upload(self, rows, flags=None):
        return self.upload_points(self.scan[rows], self.payload[rows], flags)

    def entry(self, what):
        return getattr(self.capi, f"{self.name}_{what}")

    def plain(self, s, T=None):
        return self.entry("linearize")(self.tgt, s, self.T if T is None else T, self.md, *self.extra)

    def robust(self, s, kind, c, T=None):
        return self.entry("linearize_robust")(self.tgt, s, self.T if T is None else T, self.md, *self.extra, robust=(tc.KIND_ID[kind], c))

    def adaptive(self, s, kind, q, factor=1.0, T=None):
        return self.entry("linearize_adaptive")(self.tgt, s, self.T if T is None else T, self.md, *self.extra,
                                                adaptive=(tc.KIND_ID[kind], q, factor))

    def keys(self, s, T=None):
        """kappa of every scan point in the caller's order, restated from the GPU's own pcr_*_residuals."""
        r = self.entry("residuals")(self.tgt, s, self.T if T is None else T, self.md, *self.extra)
        return tc.key(r.reshape(len(r), self.m))

    def sums_over(self, mult):
        """math.fsum of the unweighted terms of the scan in which base row i appears mult[i] times -> (sums, magnitudes)."""
        mm = np.tile(np.asarray(mult, dtype=np.float64), self.m)
        return gc.fsum_cols(self.t * mm[:, None])[:2]


def _symm_side(capi, ctx, orc, g2):
    T, src, md = g2["T"], g2["source"], float(g2["max_dist"])
    n_p = sc.unit_normals(len(src))
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(md)
    _, t, s, keep = rc.terms_symm(None, 1.0, T, src, orc.transform(T, src), g2["target"][j], n_p, g2["plane_normals"][j], mask)
    tgt = capi.Target.points(ctx, g2["target"])
    tgt.set_normals(g2["plane_normals"])
    P, n = g2["target"][:400].astype(np.float64), g2["plane_normals"][:400].astype(np.float64)
    P[300:] += 0.05 * n[300:]
    return Side("symm", capi, ctx, tgt, T, md, src, n_p, (0.0,), t, keep, sc.sum_bound, (P.astype(np.float32), g2["plane_normals"][:400]))


def _color_side(capi, ctx, orc, g2):
    T, src, md = g2["T"], g2["source"], float(g2["max_dist"])
    I_q = cc.field(g2["target"])
    G = (0.3 * np.random.default_rng(1).normal(size=(5000, 3))).astype(np.float32)
    I_p = np.random.default_rng(0).uniform(0, 1, 2000).astype(np.float32)
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(md)
    _, t, s, keep = rc.terms_color(None, 1.0, T, src, orc.transform(T, src), g2["target"][j], g2["plane_normals"][j], I_q[j], G[j], I_p,
                                   mask, LAMBDA)
    tgt = capi.Target.points(ctx, g2["target"])
    tgt.set_normals(g2["plane_normals"])
    tgt.set_intensity(I_q, G)
    P, n = g2["target"][:400].astype(np.float64), g2["plane_normals"][:400].astype(np.float64)
    P[300:] += 0.05 * n[300:]
    I_s = I_q[:400].copy()
    I_s[300:] += np.float32(0.25)
    return Side("color", capi, ctx, tgt, T, md, src, I_p, (LAMBDA,), t, keep, cc.sum_bound, (P.astype(np.float32), I_s))


def _dist_side(name, capi, ctx, orc, built):
    which = "pt" if name == "gicp" else "vox"
    T, scan, cls = dc.base_scan(which)
    tp = orc.transform(T, scan)
    if name == "gicp":
        t32 = built["pt"]["target32"]
        Cp, Cq = dc.spd_pair(len(scan), len(t32), seed=24)
        tgt = capi.Target.points(ctx, t32)
        tgt.set_covariances(Cq)
        dist, idx = orc.nn_brute(t32, tp)
        mask = dist < np.float32(dc.BASE_GATE)
        q, Cm, res = t32[idx], Cq[idx], "f32"
        centres, n_exact, n_all = t32.astype(np.float64), 300, 400
    else:
        vox = built["vox"]
        Cp, cv = dc.spd_pair(len(scan), 64, seed=25)
        tgt = capi.Target.voxels(ctx, vox["target64"], vox["voxel_size"])
        tgt.set_voxel_covariances(cov=cv.astype(np.float64))
        mean, Cv = tgt.voxel_stats(("mean",))["mean"], tgt.get_voxel_covariances()
        dist, idx = orc.nn_brute_f64(mean, tp)
        mask = dist < dc.BASE_GATE
        q, Cm, res = mean[idx], Cv[idx], "f64"
        centres, n_exact, n_all = mean, 40, 64
    assert np.array_equal(mask, cls == 0)
    _, t, s, keep, eps_min = rc.terms_dist(None, 1.0, T, scan, tp, q, Cp, Cm, mask, res)
    P = centres[:n_all].copy()
    P[n_exact:, 0] += 0.05
    return Side(name, capi, ctx, tgt, T, dc.BASE_GATE, scan, Cp, (), t, keep, lambda n, mag: gc.sum_bound(n, eps_min, mag),
                (P.astype(np.float32), Cp[:n_all]))


def build(capi, ctx, orc, g2):
    built = pc.build_all(load_golden("g16_pass_cases.npz"))
    return {"symm": _symm_side(capi, ctx, orc, g2), "color": _color_side(capi, ctx, orc, g2),
            "gicp": _dist_side("gicp", capi, ctx, orc, built), "vgicp": _dist_side("vgicp", capi, ctx, orc, built)}


def e2e_reg(name, capi, ctx, case, **kw):
    """(aligner with the end-to-end case's target and GIVEN payloads on it, keyword arguments of its calc_H_g_e2 / align)."""
    import point_cloud_registration_amd as pcr
    common = dict(max_dist=rc.E2E_MAX_DIST, tol=rc.E2E_TOL, **kw)
    if name == "symm":
        reg = pcr.SymmetricICP(**common)
        reg.set_target(case["target"], norm=case["n_q"])
        return reg, dict(source_normals=case["n_p"])
    if name == "color":
        reg = pcr.ColoredICP(lambda_geometric=rc.E2E_LAMBDA, **common)
        reg.set_target(case["target"], case["I_q"], norm=case["n_q"], gradient=case["g_q"])
        return reg, dict(source_intensity=case["I_p"])
    if name == "gicp":
        reg = pcr.GICP(**common)
        reg.set_target(case["target"], cov=case["Cq"])
        return reg, dict(source_cov=case["Cp"])
    reg = pcr.VGICP(voxel_size=rc.E2E_VOXEL, **common)
    tgt = capi.Target.voxels_from_stats(ctx, case["means"], case["vnorm"], None, rc.E2E_VOXEL)      # the restated voxels
    tgt.set_voxel_covariances(cov=case["Cv"])
    assert np.array_equal(tgt.voxel_stats(("mean",))["mean"], case["means"]) and np.array_equal(tgt.get_voxel_covariances(), case["Cv"])
    reg._set_target_handle(tgt)
    return reg, dict(source_cov=case["Cp"])
