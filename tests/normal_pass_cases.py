"""Cases of the SymmetricICP and ColoredICP passes (csrc/symm.hip, color.hip over csrc/match_pass.h) at the gate boundary and
across the pose space, shared by tests/test_normal_pass_cases.py and tests/test_gpu_symm_color_pass.py.  Plain NumPy plus the
CPU oracle, deterministic, no GPU.  Every cloud, gate and pose is the one of tests/pass_cases.py (g16); the restatement is
symm_cases.terms / kept / dots / reference and color_cases.terms / reference.  What is new here is what rides on the clouds.

a  Exact normal classes on the point lattices.  Probe i carries the WORLD-frame normal KINDS[i % 5], target row j the axis
   eye(3)[j % 3].  At exact pose T = (R, t) the library is handed float32(n_world @ R) = R^T n_world -- R is a signed
   permutation, so the cast is exact and R n_p is n_world again, bit for bit.  c = n_q . R n_p is then one component of a
   KINDS row: every product is with 0 or +-1, every sum has one non-zero term, and c takes exactly the values of C_VALUES
   whatever the contraction or the order of operations.  MIN_COS sits on, one ulp below and one ulp above 0.5 and S; the
   decision |c| >= min_cos is taken ON its boundary, and the sign decision at c == 0 (s = +1, m = 0.5 (n_q + v)) is taken at
   min_cos = 0.  SYMM_COUNTS is written out; ``rule_counts`` derives it from the designed classes alone.
b  A dyadic colour payload on the same lattices: intensities k / 16, given gradients k / 8 that are NOT tangent to the axis
   normals, so a pass that drops the projection m = g - (g . n) n is seen.
c  The twelve general poses of pass_cases.general_cases (a rotation of pi - 1e-4, |t| up to 1e4 m) with random unit normals
   and random given gradients; intensities are color_cases.field of the coordinates relative to the box centre, so they
   do not grow with |t|."""

import numpy as np

import color_cases as cc
import pass_cases as pc
import symm_cases as sc

S = np.float32(0.70710677)
S64 = float(S)
KINDS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0.5, 0.5, S), (-0.5, S, 0.5)], dtype=np.float32)
C_VALUES = (-1.0, -0.5, 0.0, 0.5, S64, 1.0)
MIN_COS = (0.0, float(np.nextafter(0.5, 0.0)), 0.5, float(np.nextafter(0.5, 1.0)), S64, float(np.nextafter(S64, 1.0)), 1.0)
LAMBDAS = (0.0, 0.5, 0.968, 1.0)

# kept pairs per gate of pass_cases.gates(1.25) (rows) and per min_cos of MIN_COS (columns): the same at all nine exact poses
# and for both forms of the lattice.  Column 0 is pass_cases.POINT_COUNTS_F32.
#          min_cos   0   0.5-  0.5  0.5+   S    S+    1
_AT_D = (80, 45, 45, 23, 23, 13, 13)               # the 40 probes ON lattice points and the 40 at d / 2
_ALL = (280, 163, 163, 84, 84, 51, 51)             # ... and the 200 at d
_AT_HALF = (40, 22, 22, 12, 12, 6, 6)              # the 40 ON lattice points alone
SYMM_COUNTS = (
    _AT_D,      # d
    _ALL,       # d + 1 ulp32
    _AT_D,      # d - 1 ulp32
    _AT_D,      # d + 1 ulp64: (float) of it is d
    _AT_D,      # d - 1 ulp64: (float) of it is d
    _AT_HALF,   # d / 2
    _AT_HALF,   # d / 2 + 1 ulp64: (float) of it is d / 2
    _AT_HALF,   # 1e-30
    _AT_HALF,   # 1e-20
    _ALL,       # 1e19
    _ALL,       # 1e20
    _ALL,       # 1e300
    _ALL,       # inf
)
# the gates at which every min_cos of MIN_COS is taken: d, d + 1 ulp32, d / 2, inf
FULL_MIN_COS_GATES = (0, 1, 5, 12)


def _orc():
    from oracle import oracle
    return oracle


# ----------------------------------------------------------------------------- a. exact normal classes
def world_normals(n_probes):
    """KINDS[i % 5] over the probes, float32 (n, 3)."""
    return np.ascontiguousarray(KINDS[np.arange(n_probes) % 5])


def target_normals(n_target):
    """eye(3)[j % 3] over the target rows (blob points of the heavy lattice included), float32 (n, 3)."""
    return np.ascontiguousarray(np.eye(3, dtype=np.float32)[np.arange(n_target) % 3])


def scan_normals(T, n_world):
    """What the library is handed at exact pose T: float32(n_world @ R) = R^T n_world; the cast is exact."""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    n64 = np.asarray(n_world, dtype=np.float32).astype(np.float64) @ R
    n32 = n64.astype(np.float32)
    assert np.array_equal(n32.astype(np.float64), n64)
    return np.ascontiguousarray(n32)


def probe_classes(lat):
    """The designed distance of every probe, in pass_cases order: float64 (n,)."""
    return np.concatenate([np.full(n, d) for d, n in lat["classes"]])


def rule_counts(lat):
    """SYMM_COUNTS from the designed classes alone -- the distance class of probe i, KINDS[i % 5] and the axis of its lattice
    point -- with the reference's float32 comparison of pass_cases.rule_count: no code under test, no search."""
    d = probe_classes(lat)
    i = np.arange(len(d))
    c = KINDS[i % 5, np.asarray(lat["probe_of"]) % 3].astype(np.float64)
    out = []
    with np.errstate(over="ignore"):
        for md in pc.gates(lat["d"]):
            inside = d.astype(np.float32) < np.float32(md)
            out.append(tuple(int(np.sum(inside & (np.abs(c) >= mc))) for mc in MIN_COS))
    return tuple(out)


def colour_payload(n_probes, n_target):
    """(I_q (n_target,), I_p (n_probes,), G (n_target, 3)) float32, all dyadic: I_q = (j % 16) / 16, I_p = (7 i % 16) / 16,
    G = ((j % 5) - 2, (j % 3) - 1, (j % 7) - 3) / 8 -- not tangent to the axis normals."""
    j, i = np.arange(n_target), np.arange(n_probes)
    I_q = ((j % 16) / 16.0).astype(np.float32)
    I_p = (((7 * i) % 16) / 16.0).astype(np.float32)
    G = (np.stack([(j % 5) - 2, (j % 3) - 1, (j % 7) - 3], axis=1) / 8.0).astype(np.float32)
    return I_q, I_p, G


def lattice_case(lat):
    """Everything of a point lattice (pass_cases.point_lattice / heavy_lattice) at the nine exact poses -> dict: target32,
    probes, gates, n_world, n_q, I_q, I_p, G and poses = [(T, scan, n_p, tp, dist, idx, c)] with tp = the probes (the float32
    transform is exact), dist / idx the oracle's brute-force float32 matches, c = symm_cases.dots.  The claims of (a) are
    asserted here: the exact values of c, and SYMM_COUNTS against the rule and against the oracle's mask at every pose."""
    orc = _orc()
    t32, probes = lat["target32"], lat["probes"]
    n_world, n_q = world_normals(len(probes)), target_normals(len(t32))
    I_q, I_p, G = colour_payload(len(probes), len(t32))
    gates = pc.gates(lat["d"])
    assert rule_counts(lat) == SYMM_COUNTS
    assert [row[0] for row in SYMM_COUNTS] == pc.POINT_COUNTS_F32
    poses = []
    for T, scan in pc.exact_poses(probes):
        n_p = scan_normals(T, n_world)
        tp = orc.transform(T, scan)
        dist, idx = orc.nn_brute(t32, tp)
        assert np.array_equal(idx, lat["probe_of"])                       # every probe's nearest neighbour is its lattice point
        assert np.array_equal(sc.rotated(T, n_p), n_world.astype(np.float64))
        c = sc.dots(T, n_p, n_q[idx])
        assert sorted(set(c.tolist())) == sorted(C_VALUES)
        with np.errstate(over="ignore"):
            for gi, md in enumerate(gates):
                mask = dist < np.float32(md)
                for mi, mc in enumerate(MIN_COS):
                    assert int(sc.kept(T, n_p, n_q[idx], mask, mc).sum()) == SYMM_COUNTS[gi][mi], (gi, mi)
        poses.append((T, scan, n_p, tp, dist, idx, c))
    out = {"target32": t32, "probes": probes, "gates": gates, "n_world": n_world, "n_q": n_q, "I_q": I_q, "I_p": I_p, "G": G,
           "poses": poses}
    for a in (n_world, n_q, I_q, I_p, G):
        a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- c. general poses
GENERAL_MIN_COS = (0.0, 0.5)
GENERAL_LAMBDAS = (0.968, 0.5)
GENERAL_K = 10                             # neighbours of the normals and gradients estimated on the device


def general_normals(n_target, n_scan=1500):
    """Random unit normals, symm_cases.unit_normals: (n_q of the target, n_p of a scan)."""
    return sc.unit_normals(n_target, seed=1611), sc.unit_normals(n_scan, seed=1612)


def general_gradients(n_target):
    """Random given gradients 0.3 normal(size = (n, 3)), float32 -- not tangent to any normal."""
    return (0.3 * np.random.default_rng(1613).normal(size=(n_target, 3))).astype(np.float32)


def general_intensities(norm, target, tp):
    """(I_q, I_p): color_cases.field of the coordinates relative to the box centre norm * (0.6, -0.64, 0.48), the scan's at its
    transformed points ``tp`` -- values in [0, 1] whatever |t|."""
    centre = norm * np.array([0.6, -0.64, 0.48])
    return cc.field(np.asarray(target, np.float64) - centre), cc.field(np.asarray(tp, np.float64) - centre)


def away_from_gate(c, mask, min_cos):
    """The condition on the inputs of a general-pose case: no pair inside the distance gate has ||c| - min_cos| < 1e-9."""
    c = np.asarray(c)[np.asarray(mask, dtype=bool)]
    return min_cos == 0.0 or bool(np.min(np.abs(np.abs(c) - min_cos)) >= 1e-9)
