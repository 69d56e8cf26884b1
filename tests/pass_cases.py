"""Inputs shared by tests/test_gpu_pass_cases.py, tests/test_oracle_golden.py and tests/golden/make_golden_pass_cases.py (g16):
one pass (calc_H_g_e2) with scan points ON the gate, gates whose float32 square underflows or overflows, and start poses far
from the identity.  Plain NumPy, deterministic, no GPU and no reference; the builders check their own exactness claims with
the CPU oracle.  The fixture stores the reference's figures only -- every cloud comes from here (crc32-guarded).

Exact lattices: every coordinate is a small dyadic rational, so positions, the float32 transform at the exact poses, squared
distances and their roots are exact in float32 and float64 alike, and the number of points a gate keeps follows from the
reference's comparison alone (``rule_count``), not from any code under test:
  point targets      icp.py:34 / plane_icp.py:41 compare the tree's FLOAT32 distance with max_dist -> with (float)max_dist
  voxel targets      voxelized_plane_icp.py:38 / ndt.py:33 compare a float64 distance with max_dist
  float64 PlaneICP   plane_icp.py:22: the tree over a float64 array returns float64 distances (quirk Q6)
"""

import zlib

import numpy as np

KINDS = ("icp", "plane", "vplane", "ndt")
INF = float("inf")


def _orc():
    from oracle import oracle
    return oracle


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ----------------------------------------------------------------------------- exact lattices
OFFSETS = np.array([(3, 4, 0), (0, 3, 4), (4, 0, 3), (0, 0, 5), (5, 0, 0)], dtype=np.float64)     # every one of length 5
POINT_D, VOXEL_D = 1.25, 0.3125            # OFFSETS * 0.25 and OFFSETS / 16


def point_lattice():
    """8 x 8 x 8 points 4 m apart, each moved by k / 64 (|k| <= 8) per axis so that k-NN normals are not degenerate.
    -> dict: target32, target64 (the float64 array the float32 one was cast from: equal values), probes (280, 3) float32 and
    classes = [(distance, count)]: 40 probes per offset of OFFSETS * 0.25 from distinct lattice points (distance exactly
    1.25), 40 ON lattice points, 40 at (3, 4, 0) * 0.125 (distance 0.625); free = lattice points no probe uses."""
    rng = np.random.default_rng(1601)
    grid = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3) * 4.0
    p64 = grid + rng.integers(-8, 9, grid.shape) / 64.0
    p32 = p64.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p64)
    order = rng.permutation(p64.shape[0])
    off = np.concatenate([np.repeat(OFFSETS * 0.25, 40, axis=0), np.zeros((40, 3)), np.tile(OFFSETS[0] * 0.125, (40, 1))])
    probes64 = p64[order[:280]] + off
    probes = probes64.astype(np.float32)
    assert np.array_equal(probes.astype(np.float64), probes64)
    return {"target32": p32, "target64": p64, "probes": probes, "probe_of": order[:280], "free": order[280:],
            "classes": [(POINT_D, 200), (0.0, 40), (POINT_D / 2, 40)], "d": POINT_D}


def heavy_lattice():
    """The point lattice plus two blobs of 1 500 points (dyadic offsets k / 1024 within 0.39 m) around lattice points that no
    probe uses: hundreds of points in two cells (the heavy-cell form of the index, PCR_HEAVY=1), every probe's nearest
    neighbour unchanged, and few enough points (3 512) for the oracle to search by brute force."""
    lat = point_lattice()
    rng = np.random.default_rng(1602)
    blobs = [lat["target64"][c] + rng.integers(-230, 231, (1500, 3)) / 1024.0 for c in lat["free"][:2]]
    t64 = np.concatenate([lat["target64"]] + blobs)
    t32 = t64.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t64) and t32.shape[0] <= 4096
    orc = _orc()
    d0, i0 = orc.nn_brute(lat["target32"], lat["probes"])
    d1, i1 = orc.nn_brute(t32, lat["probes"])
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    return dict(lat, target32=t32, target64=t64)


def voxel_lattice():
    """4 x 4 x 4 voxels of 1 m, twelve points per voxel placed symmetrically about the centre i + 0.5 (every mean IS its
    centre); 8 probes per offset of OFFSETS / 16 (distance exactly 0.3125), 8 ON centres, 8 at half the first offset."""
    arms = np.array([(0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25), (0.125, 0.125, 0.125), (0.125, -0.125, 0), (0, 0.125, -0.125)])
    centres = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5
    pts = (centres[:, None, :] + np.concatenate([arms, -arms])[None, :, :]).reshape(-1, 3)
    rng = np.random.default_rng(1603)
    pts = pts[rng.permutation(pts.shape[0])]
    vox = _orc().TargetVoxels(pts, 1.0)
    assert vox.mean.shape[0] == 64
    assert np.array_equal(vox.mean[np.lexsort(vox.mean.T[::-1])], centres[np.lexsort(centres.T[::-1])])
    order = rng.permutation(64)
    off = np.concatenate([np.repeat(OFFSETS / 16.0, 8, axis=0), np.zeros((8, 3)), np.tile(OFFSETS[0] / 32.0, (8, 1))])
    probes64 = centres[order[:56]] + off
    probes = probes64.astype(np.float32)
    assert np.array_equal(probes.astype(np.float64), probes64)
    return {"target64": pts, "probes": probes, "classes": [(VOXEL_D, 40), (0.0, 8), (VOXEL_D / 2, 8)], "d": VOXEL_D,
            "voxel_size": 1.0}


def gates(d):
    """The gates of a lattice whose probes lie at distance d: on it, one ulp either side in float32 and in float64, on and just
    above the inner class, gates whose float32 square underflows (1e-30: to zero, 1e-20: to a subnormal) or overflows (1e20;
    1e19 is the last decade that does not), a gate float32 cannot hold, no gate."""
    f32, f64 = np.float32(d), np.float64(d)
    return [float(d),
            float(np.nextafter(f32, np.float32(np.inf))), float(np.nextafter(f32, np.float32(-np.inf))),
            float(np.nextafter(f64, np.inf)), float(np.nextafter(f64, -np.inf)),
            float(d / 2), float(np.nextafter(np.float64(d / 2), np.inf)),
            1e-30, 1e-20, 1e19, 1e20, 1e300, INF]


# The reference's ICP takes its moment sums in the scan's dtype (icp.py:42-46, quirk Q5): float32 products rounded once (1 u),
# summed pairwise over n <= 280 probes (ceil(log2 n) u), two such sums added (1 u); u = 2^-24, relative to sum |terms| <= max |H|.
# That is how far its H may lie from a float64 evaluation of the same matches on the lattices.
F32_SUM_BOUND = (2 + int(np.ceil(np.log2(280)))) * 2.0 ** -24


def rule_count(classes, max_dist, gate_f32):
    """How many probes the reference's ``dist < max_dist`` keeps, from the designed distances: the float32 distance against
    (float)max_dist for a float32 tree, the float64 distance against max_dist otherwise."""
    with np.errstate(over="ignore"):
        if gate_f32:
            return int(sum(n for d, n in classes if np.float32(d) < np.float32(max_dist)))
    return int(sum(n for d, n in classes if d < max_dist))


# expected counts, written out: {d: [count per gate of gates(d)]} for a float32 tree and for a float64 one
#             d   +1ulp32 -1ulp32 +1ulp64 -1ulp64  d/2  d/2+  1e-30 1e-20 1e19 1e20 1e300 inf
POINT_COUNTS_F32 = [80, 280, 80, 80, 80, 40, 40, 40, 40, 280, 280, 280, 280]      # (float) of d +- 1 ulp64 and of d/2+ is d, d/2
POINT_COUNTS_F64 = [80, 280, 80, 280, 80, 40, 80, 40, 40, 280, 280, 280, 280]     # PlaneICP over the float64 lattice (Q6)
VOXEL_COUNTS = [16, 56, 16, 56, 16, 8, 16, 8, 8, 56, 56, 56, 56]


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


EXACT_ROTATIONS = [np.eye(3), np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])]
EXACT_TRANSLATIONS = [(0.0, 0.0, 0.0), (64.0, -32.0, 16.0), (8192.0, -4096.0, 1024.0)]


def make_T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def sensor_frame(T, world):
    """R^T (q - t) in float64, cast to float32: the scan a sensor at pose T sees of the map points ``world``."""
    R, t = T[:3, :3], T[:3, 3]
    return np.ascontiguousarray(((np.asarray(world, np.float64) - t) @ R).astype(np.float32))


def exact_poses(probes):
    """-> [(T, scan)] for the 9 exact poses (rotations by 0 / 90 deg about z / 180 deg about x, translations up to 8192 m): the
    float32 transform of every scan returns the probes bit for bit."""
    orc = _orc()
    out = []
    for R in EXACT_ROTATIONS:
        for t in EXACT_TRANSLATIONS:
            T = make_T(R, t)
            scan = sensor_frame(T, probes)
            assert np.array_equal(orc.transform(T, scan), probes), (R, t)
            out.append((T, scan))
    return out


# ----------------------------------------------------------------------------- general poses
GENERAL_MAX_DIST, GENERAL_VOXEL = 0.5, 1.0
GENERAL_NORMS = (0.0, 50.0, 1.0e4)
_DIRECTION = np.array([0.6, -0.64, 0.48])                  # |.| = 1


def _quat_R(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def general_rotations():
    rng = np.random.default_rng(1604)
    return [np.eye(3), _quat_R(rng.standard_normal(4)), _quat_R(rng.standard_normal(4)), _rot((1.0, 2.0, -2.0), np.pi - 1e-4)]


def general_target(norm):
    """20 000 uniform points in a 6 m box centred at norm * (0.6, -0.64, 0.48), float32 (one target per |t|)."""
    rng = np.random.default_rng(1605)
    return np.ascontiguousarray((rng.uniform(-3.0, 3.0, (20_000, 3)) + norm * _DIRECTION).astype(np.float32))


def general_cases():
    """-> [(name, norm, T, scan)]: 4 rotations x |t| in (0, 50, 1e4); the scan is 1 500 points of a slightly larger box around
    the map (so the gate bites) as a sensor at T sees them -- small coordinates whatever |t| is."""
    out = []
    for ri, R in enumerate(general_rotations()):
        for norm in GENERAL_NORMS:
            rng = np.random.default_rng(1606 + ri)
            T = make_T(R, norm * _DIRECTION)
            world = rng.uniform(-3.3, 3.3, (1500, 3)) + norm * _DIRECTION
            out.append((f"r{ri}_t{norm:g}", norm, T, sensor_frame(T, world)))
    return out


DATA_GATE_CASE = "r1_t50"                     # the general-pose case of the data-dependent gates
DATA_GATE_RANKS = (5, 100, 300, 500, 590)


def data_gates(dist, f32):
    """Gates ON the oracle's own distances (oracle-only material: a reference tree's last ulp may differ): for the distance d_k
    at each rank of DATA_GATE_RANKS among the sorted distances, max_dist = d_k and its successor in the type the gate is taken
    in -> [(max_dist, expected count)] with the count (d < max_dist).sum() on those distances."""
    dt = np.float32 if f32 else np.float64
    d = np.asarray(dist).astype(dt)
    s = np.sort(d)
    out = []
    for k in DATA_GATE_RANKS:
        for md in (s[k], np.nextafter(s[k], dt(np.inf))):
            out.append((float(md), int((d < md).sum())))
    return out


# ----------------------------------------------------------------------------- everything, built once
def build_all(g16=None):
    """Every case of this module; with the g16 fixture given, every cloud is checked against the crc32 stored there."""
    lat, heavy, vox = point_lattice(), heavy_lattice(), voxel_lattice()
    built = {"pt": lat, "heavy": heavy, "vox": vox, "gen": general_cases(),
             "gen_targets": {norm: general_target(norm) for norm in GENERAL_NORMS}}
    if g16 is not None:
        clouds = [("pt_target32", lat["target32"]), ("pt_target64", lat["target64"]), ("pt_probes", lat["probes"]),
                  ("heavy_target32", heavy["target32"]), ("vox_target64", vox["target64"]), ("vox_probes", vox["probes"])]
        clouds += [(f"gen_target_t{norm:g}", t) for norm, t in built["gen_targets"].items()]
        clouds += [(f"gen_scan_{name}", scan) for name, _, _, scan in built["gen"]]
        for name, arr in clouds:
            assert crc(arr) == int(g16[f"crc32_{name}"]), f"{name}: pass_cases.py no longer reproduces the cloud of the g16 fixture"
        assert np.array_equal(g16["lat_gates_pt"], gates(POINT_D)) and np.array_equal(g16["lat_gates_vox"], gates(VOXEL_D))
        assert np.array_equal(g16["gen_T"], np.array([T for _, _, T, _ in built["gen"]]))
    return built
