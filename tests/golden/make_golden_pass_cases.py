#!/usr/bin/env python3
"""Generate tests/golden/g16_pass_cases.npz by RUNNING the reference's four classes on the cases of tests/pass_cases.py.

Run where the reference is at hand only (it is not part of this repository and never travels to the GPU box):

    python tests/golden/make_golden_pass_cases.py

The reference is imported with the pykdtree stand-in of ``make_golden.py`` (scipy.spatial.cKDTree).  Only arrays are stored;
every cloud is regenerated from tests/pass_cases.py and guarded by a crc32.

Contents:
  lat_gates_pt, lat_gates_vox         the 13 gates of pass_cases.gates(1.25) / gates(0.3125)
  lat_T                               (9, 4, 4) the exact poses, in the order of pass_cases.exact_poses
  lat_{case}_{kind}_H / _g / _e2      (9, 13, 6, 6) / (9, 13, 6) / (9, 13): calc_H_g_e2 of the reference at every exact pose and
                                      gate; case in pt (float32 point lattice: icp, plane), pt64 (PlaneICP over the float64 copy,
                                      quirk Q6: plane), heavy (lattice + blobs: icp, plane), vox (voxel lattice: vplane, ndt)
  normals_pt, normals_pt64, normals_heavy, normals_t{norm}
                                      the reference's own k = 15 normal estimate of each point target, as float32 -- estimated
                                      once, then handed to the reference, the oracle and the GPU alike (plane_icp.py:25-27)
  gen_names (as crc32 of the name), gen_T (12, 4, 4), gen_{kind}_H / _g / _e2 (12, ...)
                                      the general-pose cases at max_dist 0.5, voxel size 1.0
  crc32_*                             of every regenerated cloud
Before writing, the oracle must agree with the reference on every stored case: H within 1e-9 (lattices), and rel_H < 1e-5, e2
within 5e-5, Gauss-Newton step within 5e-5 (general poses).  ICP on the lattices is the one place where the stored run cannot
meet 1e-9: icp.py:42-46 sums its moments in float32 (quirk Q5; measured 9.3e-8).  There the 1e-9 bar is taken against the same
class on the float64 copy of the same scan (measured 0), and the stored float32 run is held to pass_cases.F32_SUM_BOUND.
The data-dependent gates of pass_cases.data_gates are NOT stored: a gate placed on an oracle distance is decided by the tree
backend's last ulp."""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                # noqa: E402  (installs the pykdtree stand-in, imports the reference)
import pass_cases as pc                 # noqa: E402
from conftest import rel_H, step_err    # noqa: E402
from oracle import oracle as orc        # noqa: E402

ref = mg.ref
OKIND = {"icp": orc.ICP, "plane": orc.PLANE, "vplane": orc.VPLANE, "ndt": orc.NDT}
WORST = {}
F32_SUM_BOUND = pc.F32_SUM_BOUND           # how far ICP's float32 moment sums may lie from a float64 evaluation


def _note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def ref_normals(target, k=15):
    p = ref.PlaneICP(k=k)
    p.set_target(target)
    return np.ascontiguousarray(np.asarray(p.normal), dtype=np.float32)


def ref_objects(kinds, target, normals, max_dist, voxel_size=1.0):
    objs = {}
    for kind in kinds:
        if kind == "icp":
            o = ref.ICP(max_dist=max_dist); o.set_target(target)
        elif kind == "plane":
            o = ref.PlaneICP(max_dist=max_dist, k=15); o.set_target(target, ref.KDTree(target), normals)
        elif kind == "vplane":
            o = ref.VPlaneICP(voxel_size=voxel_size, max_dist=max_dist); o.set_target(target)
        else:
            o = ref.NDT(voxel_size=voxel_size, max_dist=max_dist); o.set_target(target)
        objs[kind] = o
    return objs


def run_ref(obj, T, scan, max_dist):
    obj.max_dist = max_dist
    with warnings.catch_warnings(), np.errstate(over="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)          # ((float)1e300 overflows to inf in the float32 comparison)
        return mg.triple(obj.calc_H_g_e2(T, scan))


def lattice_case(out, case, kinds, target, normals, probes, d, o_target):
    poses = pc.exact_poses(probes)
    gs = pc.gates(d)
    objs = ref_objects(kinds, target, normals, 1.0)
    for kind in kinds:
        H = np.zeros((len(poses), len(gs), 6, 6)); g = np.zeros((len(poses), len(gs), 6)); e2 = np.zeros((len(poses), len(gs)))
        for pi, (T, scan) in enumerate(poses):
            for gi, md in enumerate(gs):
                H[pi, gi], g[pi, gi], e2[pi, gi] = run_ref(objs[kind], T, scan, md)
                Ho, go, e2o, cnt = orc.calc_H_g_e2(OKIND[kind], o_target, T, scan, md, with_count=True)
                what = (case, kind, pi, md)
                if not H[pi, gi].any():
                    assert cnt == 0 and not Ho.any() and not go.any() and e2o == 0, what
                    continue
                if kind == "icp":
                    # icp.py:42-46 takes its moment sums in the scan's dtype: float32 sums of up to 280 terms (quirk Q5), which
                    # the oracle -- float64 sums -- cannot and must not follow.  The 1e-9 bar is met against the SAME class
                    # given the float64 copy of the same scan (same points, same matches, same gate: only the sums widen); the
                    # stored float32 run is held to the error bound of a pairwise float32 sum of that length.
                    assert cnt == H[pi, gi][0, 0], what
                    H64 = run_ref(objs[kind], T, scan.astype(np.float64), md)[0]
                    assert rel_H(Ho, H64) < 1e-9, (what, rel_H(Ho, H64))
                    assert rel_H(Ho, H[pi, gi]) <= F32_SUM_BOUND, (what, rel_H(Ho, H[pi, gi]))
                    _note("lattice icp rel_H (float64 copy of the scan)", rel_H(Ho, H64))
                else:
                    assert rel_H(Ho, H[pi, gi]) < 1e-9, (what, rel_H(Ho, H[pi, gi]))
                _note(f"lattice {kind} rel_H", rel_H(Ho, H[pi, gi]))
                _note(f"lattice {kind} e2 rel", abs(e2o - e2[pi, gi]) / max(abs(e2[pi, gi]), 1e-300))
        out[f"lat_{case}_{kind}_H"], out[f"lat_{case}_{kind}_g"], out[f"lat_{case}_{kind}_e2"] = H, g, e2
    return poses


def generate():
    out = {}
    lat, heavy, vox = pc.point_lattice(), pc.heavy_lattice(), pc.voxel_lattice()
    out["lat_gates_pt"], out["lat_gates_vox"] = np.array(pc.gates(pc.POINT_D)), np.array(pc.gates(pc.VOXEL_D))
    for name, arr in (("pt_target32", lat["target32"]), ("pt_target64", lat["target64"]), ("pt_probes", lat["probes"]),
                      ("heavy_target32", heavy["target32"]), ("vox_target64", vox["target64"]), ("vox_probes", vox["probes"])):
        out[f"crc32_{name}"] = np.int64(pc.crc(arr))
    # point lattice, float32 and float64 (quirk Q6), and its heavy form
    n_pt = out["normals_pt"] = ref_normals(lat["target32"])
    poses = lattice_case(out, "pt", ("icp", "plane"), lat["target32"], n_pt, lat["probes"], lat["d"],
                         orc.TargetPoints(lat["target32"], normals=n_pt))
    out["lat_T"] = np.array([T for T, _ in poses])
    n_64 = out["normals_pt64"] = ref_normals(lat["target64"])
    lattice_case(out, "pt64", ("plane",), lat["target64"], n_64, lat["probes"], lat["d"],
                 orc.TargetPoints(lat["target64"], normals=n_64, tree_f64=True))
    n_hv = out["normals_heavy"] = ref_normals(heavy["target32"])
    lattice_case(out, "heavy", ("icp", "plane"), heavy["target32"], n_hv, heavy["probes"], heavy["d"],
                 orc.TargetPoints(heavy["target32"], normals=n_hv))
    lattice_case(out, "vox", ("vplane", "ndt"), vox["target64"], None, vox["probes"], vox["d"],
                 orc.TargetVoxels(vox["target64"], vox["voxel_size"]))
    # general poses
    cases = pc.general_cases()
    out["gen_names"] = np.array([pc.crc(name.encode()) for name, _, _, _ in cases], dtype=np.int64)
    out["gen_T"] = np.array([T for _, _, T, _ in cases])
    md, vs = pc.GENERAL_MAX_DIST, pc.GENERAL_VOXEL
    res = {kind: ([], [], []) for kind in pc.KINDS}
    for norm in pc.GENERAL_NORMS:
        target = pc.general_target(norm)
        out[f"crc32_gen_target_t{norm:g}"] = np.int64(pc.crc(target))
        normals = out[f"normals_t{norm:g}"] = ref_normals(target)
        objs = ref_objects(pc.KINDS, target, normals, md, vs)
        o_pts, o_vox = orc.TargetPoints(target, normals=normals), orc.TargetVoxels(target, vs)
        for name, nrm, T, scan in cases:
            if nrm != norm:
                continue
            out[f"crc32_gen_scan_{name}"] = np.int64(pc.crc(scan))
            for kind in pc.KINDS:
                H, g, e2 = run_ref(objs[kind], T, scan, md)
                Ho, go, e2o = orc.calc_H_g_e2(OKIND[kind], o_pts if kind in ("icp", "plane") else o_vox, T, scan, md)
                what = (name, kind, rel_H(Ho, H), abs(e2o - e2) / abs(e2), step_err(Ho, go, H, g))
                assert rel_H(Ho, H) < 1e-5 and abs(e2o - e2) <= 5e-5 * abs(e2) and step_err(Ho, go, H, g) <= 5e-5, what
                _note(f"general {kind} rel_H", what[2]); _note(f"general {kind} e2 rel", what[3]); _note(f"general {kind} step_err", what[4])
                res[kind][0].append(H); res[kind][1].append(g); res[kind][2].append(e2)
    # (cases run grouped by |t|: back into the order of pass_cases.general_cases)
    order = [i for norm in pc.GENERAL_NORMS for i, c in enumerate(cases) if c[1] == norm]
    inv = np.argsort(order)
    for kind in pc.KINDS:
        out[f"gen_{kind}_H"] = np.array(res[kind][0])[inv]
        out[f"gen_{kind}_g"] = np.array(res[kind][1])[inv]
        out[f"gen_{kind}_e2"] = np.array(res[kind][2])[inv]
    return out


def main():
    out = generate()
    for key in sorted(WORST):
        print(f"oracle vs reference, worst {key}: {WORST[key]:.2e}")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g16_pass_cases.npz")      # (another path: the regeneration test)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
