"""Cases for the point search far from the origin and across long grids, and one function, ``run_all``, that pushes every case
through the library.  tests/test_magnitude_cases.py checks on the CPU that the cases are what they claim;
tests/test_gpu_magnitude.py runs them in its own process with PCR_LIST_SET unset and forced to 0, 1 and 2, and as
``python tests/magnitude_cases.py OUT.npz`` in child processes under PCR_HEAVY=1, PCR_XORDER=0 and PCR_EDGE_SEED=0.

What the cases vary is Geom::slack (index_build.hip: make_geom), 16 * 1.2e-7 * (mag + h): every pruning bound, every list margin
(halo + slack) and the x-order tolerance (2 (xq + slack)) adds or subtracts it.  A regime (m, h) puts a target of 2,500 points in
a grid of 10 x 5 x 4 cells of h at the float32 offset D = (m, -m / 2, m / 64) -- three spacings on three axes -- so that slack / h
runs from 0 to 9.7: below, between and above the three list depths (0.1 / 0.25 / 0.35 cell) and the cell itself.  The long grids
have 2^14 (x) and 2^13 (y, z) cells of 0.3 m along one axis, with the origin at minus half the length, so that at the far end x - ox
is rounded: there sit the slack sites (slack_site), whose match a search without slack loses.  Points and queries within three
float32 steps of cell faces, and tie sites, lie at cell indices from 4,000 on; queries beside the clumps lie outside the grid box.

Every target and query is a float32 value held in float64, so NumPy arithmetic on the cases is exact where it says so.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import list_set_cases as lc                                                     # noqa: E402
from edge_seed_cases import _f32, _fma32, cell_of, outside                      # noqa: E402

N_POINTS = 2500                                        # below 4,096: cell_hint does not force the heavy form
GATE_CELLS = 2.0
RADIUS_CELLS = 0.7
KS = (7, 20)
EXTENT = np.array([8.5, 3.5, 2.5])                     # x cell: the points' box; floor(extent) + 2 = 10 x 5 x 4 cells
DIMS = (10, 5, 4)
WALL_X = 3.25                                          # x cell
GROW = 2.5                                             # x cell: the uniform queries' box is the points' box grown by this
HALOS = lc.HALOS
WARM = lc.WARM
ROTATION = (0.01, -0.02, 0.015)
LOOP_ITERS = 8
# (m, h, slack / h by the library's formula as the issue states it)
REGIMES = ((0.0, 1.0, 0.0), (2.0 ** 15 * 1.1, 1.0, 0.07), (2.0 ** 16 * 1.3, 1.0, 0.16), (2.0 ** 17 * 1.5, 1.0, 0.38),
           (2.0 ** 19 * 1.1, 1.0, 1.1), (2.0 ** 22 * 1.2, 1.0, 9.7), (2.0 ** 15 * 1.1, 0.3, 0.23), (2.0 ** 19 * 1.1, 0.3, 3.7))
LONG_H = 0.3
# cells along the long axis, by axis; 4 x 3 across it: 196,608 cells at most.  y and z have 2^13: the ring search visits the
# (y, z) rows of ring k even where the ring lies outside a grid that is narrow in x, so an unbounded query thousands of cells
# from the nearest point costs O(k^2) there, ~10 s per case at 2^14 cells (docs/EXPERIMENTS.md)
LONG_CELLS = (1 << 14, 1 << 13, 1 << 13)
LONG_ACROSS = (2.5, 1.5)                               # x cell: the extent across the long axis -> 4 and 3 cells
# the grid's origin: across the axis as it comes; ALONG it minus half the length, so that at the far end x - ox lies one binade
# above x and is rounded (ties to even, by up to a whole float32 step of x): the one place where the cell arithmetic of two
# points a few centimetres apart does not round alike (slack_site)
LONG_ACROSS_ORIGIN = (12.3, -4.1)
FACE_FROM = 4000                                       # cell indices of the face sites
N_TIE = 40                                             # tie sites per long grid
N_SLACK = 12                                           # slack sites per long grid
N_BESIDE = 90                                          # queries beside the clumps, outside the grid box across the axis


def snap(a):
    """float32 values, held in float64"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def slack_of(pts, h):
    """Geom::slack restated: 16 * 1.2e-7 * (the largest |coordinate| of the bounding box + h)"""
    p = np.asarray(pts, np.float64)
    return 16.0 * 1.2e-7 * (max(np.abs(p.min(0)).max(), np.abs(p.max(0)).max()) + float(np.float32(h))) + 1e-30


def dims_of(pts, h):
    """make_geom restated: floor(extent / h) + 2 cells per axis, h the float32 cell"""
    p = np.asarray(pts, np.float64)
    return tuple(int(v) for v in np.floor((p.max(0) - p.min(0)) / float(np.float32(h))) + 2)


def offset(m):
    return snap([m, -m / 2.0, m / 64.0])


class Case:
    """name, family, cell, float32 target and queries (held in float64), the frame offset D, the axis the poses shift along"""

    def __init__(self, name, family, h, pts, q, D, axis=0, regime=None):
        self.name, self.family, self.D, self.axis, self.regime = name, family, np.asarray(D, np.float64), axis, regime
        self.h = float(np.float32(h))                  # the grid's cell: cell_hint is a float
        self.pts, self.q = snap(pts), snap(q)
        self.gate = GATE_CELLS * self.h

    def poses(self, frame):
        """the eight shifts of list_set_cases.SHIFTS x h along the case's axis, as pure translations and then composed with the
        rotation; ``map``: the scan is the queries and the rotation turns about D, ``sensor``: the scan is queries - D, the
        rotation turns about the sensor's origin and the translation is D + shift"""
        from point_cloud_registration_amd.math_tools import expSO3
        out = []
        for R in (np.eye(3), np.asarray(expSO3(np.array(ROTATION)), np.float64)):
            for s in lc.SHIFTS:
                shift = np.zeros(3)
                shift[self.axis] = s * self.h
                T = np.eye(4)
                T[:3, :3] = R
                T[:3, 3] = (self.D - R @ self.D if frame == "map" else self.D) + shift
                out.append(T)
        return out

    def loops_in(self, frame):
        """whether the Gauss-Newton loops run in this frame.  In the map frame a step turns the scan about an origin |D| away: from
        3e4 m on the oracle's own loop throws the scan off the target within one to seven steps and ends on a singular system
        (no match left) in fourteen of the sixteen cases.  There the loops run in the sensor frame only, as a caller's would"""
        return frame == "sensor" or float(np.abs(self.D).max()) < 1.0e4

    def scan(self, frame):
        return _f32(self.q) if frame == "map" else (_f32(self.q) - _f32(self.D)).astype(np.float32)


FRAMES = ("map", "sensor")


def _queries(rng, pts, D, h, extent, face_axis_cells):
    """400 target points, 400 with N(0, 0.3 h) jitter, 300 uniform in the box grown by 2.5 h, 100 on cell faces"""
    n = pts.shape[0]
    own = pts[rng.integers(0, n, 400)]
    jit = pts[rng.integers(0, n, 400)] + rng.normal(0.0, 0.3 * h, (400, 3))
    uni = D + rng.uniform(-GROW, extent + GROW, (300, 3)) * h
    face = D + rng.uniform(0.0, extent, (100, 3)) * h
    for k in range(100):                               # one, two or three coordinates of a query exactly on a face
        for a in rng.permutation(3)[: 1 + k % 3]:
            face[k, a] = D[a] + float(rng.integers(0, face_axis_cells[a] + 1)) * float(np.float32(h))
    return own, jit, uni, face


def uniform_wall(m, h, seed):
    rng = np.random.default_rng(seed)
    D = offset(m)
    u = rng.uniform(0.0, 1.0, (N_POINTS, 3)) * EXTENT
    u[1500:, 0] = WALL_X                               # on the wall x is equal: the x order carries no information
    u[0], u[1] = 0.0, EXTENT                           # the corners of the box
    pts = snap(D + u * h)
    pts[1500:, 0] = snap(D[0] + WALL_X * h)
    q = np.concatenate(_queries(rng, pts, D, h, EXTENT, DIMS))
    return pts, snap(q), D


def lattice_step(D, h):
    """per axis: max(h / 4, ulp) as a whole number of float32 steps at the box's magnitude, and the half step where float32 has it"""
    ulp = np.array([float(np.spacing(np.float32(abs(D[a]) + EXTENT[a] * h))) for a in range(3)])
    step = np.maximum(np.round(h / 4.0 / ulp), 1.0) * ulp
    half = np.where(np.round(step / ulp) % 2 == 0, step / 2.0, step)
    return step, half, ulp


def lattice(m, h, seed):
    """points on D + k * step (many twice or more), queries on the half-step lattice: exact ties at every magnitude"""
    rng = np.random.default_rng(seed)
    D = offset(m)
    step, half, _ = lattice_step(D, h)
    kmax = np.floor(EXTENT * h / step).astype(np.int64)
    k = np.stack([rng.integers(0, kmax[a] + 1, N_POINTS) for a in range(3)], 1)
    k[0], k[1] = 0, kmax
    pts = D + k * step
    groups = _queries(rng, pts, D, h, kmax * step / h, DIMS)
    q = np.concatenate([groups[0]] + [D + np.round((g - D) / half) * half for g in groups[1:]])
    return pts, q, D


def first_in_cell(o, h, c):
    """the smallest float32 x whose cell along an axis with origin o is c, by the search's float32 arithmetic"""
    o32, inv = np.float32(o), np.float32(1.0 / h)

    def cell(v):
        return int(np.floor((v - o32) * inv))
    x = np.float32(o + c * h)
    while cell(x) >= c:
        x = np.nextafter(x, np.float32(-np.inf))
    while cell(x) < c:
        x = np.nextafter(x, np.float32(np.inf))
    return x


def tie_site(o, h, c, s):
    """-> (left, right, query) along the long axis, or None.  The query sits s % 4 float32 steps from a face of cell c, one of the
    points is the LAST float32 value of the cell two cells away (ring 2: its distance is one cell plus the query's distance to its
    face plus one step, the tightest a ring-2 point can be against the ring's lower bound), the other mirrors it on the other side
    (ring 1) at exactly the same distance, or one step farther: a bound that rounds up by a step loses the ring-2 point"""
    up, down = np.float32(np.inf), np.float32(-np.inf)
    j = s % 4
    if s % 2 == 0:                                     # the query beside the lower face of its cell
        left = np.nextafter(first_in_cell(o, h, c - 1), down)
        q = first_in_cell(o, h, c)
        for _ in range(j):
            q = np.nextafter(q, up)
        d = q - left
        right = q + d
        ok = right - q == d
    else:                                              # beside the upper face
        right = first_in_cell(o, h, c + 2)
        q = np.nextafter(first_in_cell(o, h, c + 1), down)
        for _ in range(j):
            q = np.nextafter(q, down)
        d = right - q
        left = q - d
        ok = q - left == d
    if not ok:
        return None
    if (s // 4) % 2:                                   # no tie: the ring-1 point one step farther
        if s % 2 == 0:
            right = np.nextafter(right, up)
        else:
            left = np.nextafter(left, down)
    return float(left), float(right), float(q)


def _around(x, n):
    out, lo, hi = [np.float32(x)], np.float32(x), np.float32(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out = [lo] + out + [hi]
    return out


def slack_site(o, h, c, frac=HALOS[0]):
    """-> (query, point, decoy distance) along the long axis, or None.  The certificate of ring 0 (nn_certified: no point off the
    list of the query's cell is closer than fmin + halo - slack) against the rule that builds the list (halo_cells: a point of
    cell c - 1 is on the list of cell c when (c h) - (p - ox) <= halo + slack), both restated in float32 as the library computes
    them.  Sought: a query in cell c and a point of cell c - 1 that is NOT on the list when slack is 0, whose true distance is
    nevertheless below the certificate fx + halo: where fl(q - ox) rounds up and fl(p - ox) rounds down.  A decoy in the query's
    own cell, farther than the point and closer than the certificate, then ends a search without slack in ring 0 with the decoy.
    With the shipped slack (sixteen such steps) the point is on the list."""
    f = np.float32
    o32, h32, inv = f(o), f(h), f(1.0 / h)
    halo = f(frac * float(h32))
    wall = f(c) * h32
    found = None
    for q in _around(o + c * h, 6):
        fx = (q - o32) - wall
        if int(np.floor((q - o32) * inv)) != c or not fx >= 0:
            continue
        lb = fx + halo
        for pt in _around(o + c * h - float(halo), 8):
            if int(np.floor((pt - o32) * inv)) != c - 1 or wall - (pt - o32) <= halo:
                continue                               # (on the list even without slack)
            gain = float(lb) - (float(q) - float(pt))
            if gain > 0 and (found is None or gain > found[0]):
                found = (gain, float(q), float(pt), float(q) - float(pt) + 0.5 * gain)
    return None if found is None else found[1:]


def long_grid(axis, seed):
    """LONG_CELLS[axis] cells of 0.3 m along ``axis``, 4 x 3 across; clumps of points at both ends and in the middle, and face sites: at a
    face of a cell from index 4,000 on, points at three and queries at all seven of the float32 values within three steps of
    the face, all with the same other two coordinates -- distances of a few steps across a face whose side the float32 cell
    arithmetic may get wrong; N_TIE tie sites (tie_site), N_SLACK slack sites (slack_site) and N_BESIDE queries beside the clumps"""
    rng = np.random.default_rng(seed)
    h, cells = float(np.float32(LONG_H)), LONG_CELLS[axis]
    others = [a for a in range(3) if a != axis]
    D = np.zeros(3)
    D[axis], D[others[0]], D[others[1]] = -0.5 * cells * h, LONG_ACROSS_ORIGIN[0], LONG_ACROSS_ORIGIN[1]
    D = snap(D)
    ext = np.zeros(3)
    ext[axis], ext[others[0]], ext[others[1]] = cells - 1.5, LONG_ACROSS[0], LONG_ACROSS[1]
    dims = np.zeros(3, np.int64)
    dims[axis], dims[others[0]], dims[others[1]] = cells, 4, 3
    sites = np.concatenate([rng.integers(FACE_FROM, cells - 2, 50), np.arange(cells // 2 - 3, cells // 2 + 3),
                            np.arange(cells - 8, cells - 2)])
    taken = set(int(c) + k for c in sites for k in range(-5, 6)) | set(range(cells // 2 - 12, cells // 2 + 13))
    ties, c = [], FACE_FROM + 37
    while len(ties) < N_TIE:                           # cells with nothing else within five cells along the axis
        site = None if any(c + k in taken for k in range(-3, 4)) else tie_site(float(D[axis]), h, c, len(ties))
        if site is not None:
            ties.append(site)
        c += 61
    assert c < cells - 20
    slacks, c = [], cells - 30
    while len(slacks) < N_SLACK:                       # from the far end down: where x - ox is rounded
        site = None if any(c + k in taken for k in range(-3, 4)) else slack_site(float(D[axis]), h, c)
        if site is not None:
            slacks.append(site)
            taken |= set(range(c - 4, c + 5))
        c -= 9
        assert c > FACE_FROM, "no slack site: x - ox is not rounded on this grid"
    n_placed = 2 + 3 * len(sites) + 2 * N_TIE + 2 * N_SLACK
    n_clump = (N_POINTS - n_placed) // 3
    pts = [D[None, :], (D + ext * h)[None, :]]
    for at, n in ((0.0, n_clump), (cells / 2 - 4.0, n_clump), (cells - 9.5, N_POINTS - n_placed - 2 * n_clump)):
        u = rng.uniform(0.0, 1.0, (n, 3)) * ext
        u[:, axis] = at + rng.uniform(0.0, 8.0, n)
        pts.append(D + u * h)
    site_q = []
    for c in sites:
        face = np.float32(D[axis] + float(c) * h)
        steps = [face]
        lo = hi = face
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            steps = [lo] + steps + [hi]
        base = D + rng.uniform(0.1, 0.9, 3) * ext * h
        for v in rng.choice(7, 3, replace=False):
            p = base.copy()
            p[axis] = float(steps[v])
            pts.append(p[None, :])
        for v in range(7):
            p = base.copy()
            p[axis] = float(steps[v])
            site_q.append(p)
    for s, (at, point, decoy) in enumerate(slacks):    # the query in the middle of its cell across the axis, the decoy beside it
        base = D.copy()
        base[others[0]], base[others[1]] = D[others[0]] + 1.5 * h, D[others[1]] + 0.5 * h
        beside = base.copy()
        beside[others[0]] += decoy
        for v, b in ((point, base), (at, beside))[:: 1 if s % 2 else -1]:
            p = b.copy()
            p[axis] = v
            pts.append(p[None, :])
        p = base.copy()
        p[axis] = at
        site_q.append(p)
    for s, (left, right, at) in enumerate(ties):       # in both index orders: a tie goes to the smaller index
        base = D + rng.uniform(0.3, 0.7, 3) * ext * h
        base[others[0]] = D[others[0]] + (rng.integers(0, 3) + rng.uniform(0.3, 0.7)) * h      # well inside its cell across the axis
        base[others[1]] = D[others[1]] + (rng.integers(0, 2) + rng.uniform(0.3, 0.7)) * h
        for v in ((left, right), (right, left))[(s // 8) % 2] + (at,):
            p = base.copy()
            p[axis] = v
            (site_q if v == at else pts).append(p if v == at else p[None, :])
    pts = snap(np.concatenate(pts))
    own, jit, uni, face = _queries(rng, pts, D, h, ext, dims - 1)
    # beside the clumps, below the grid box across the axis and within the gate of the points: seeds of queries outside the box
    beside = pts[2 + rng.integers(0, 3 * n_clump, N_BESIDE)].copy()
    for k in range(N_BESIDE):
        a = others[k % 2]
        beside[k, a] = D[a] - rng.uniform(0.05, 1.2) * h
    q = snap(np.concatenate([own, jit, uni, face, beside, np.array(site_q)]))
    return pts, q, D, h


def cases():
    out = []
    for r, (m, h, _) in enumerate(REGIMES):
        out.append(Case(f"uniform_r{r}", "uniform", h, *uniform_wall(m, h, 7100 + r), regime=r))
        out.append(Case(f"lattice_r{r}", "lattice", h, *lattice(m, h, 7200 + r), regime=r))
    for axis in range(3):
        pts, q, D, h = long_grid(axis, 7300 + axis)
        out.append(Case("long_" + "xyz"[axis], "long", h, pts, q, D, axis=axis))
    return out


def d2_rows(pts, q):
    """(M, N) squared distances by the library's float32 formula"""
    pts, q = _f32(pts), _f32(q)
    dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


# ---- the library ----------------------------------------------------------------------------------------------------------
def run_case(capi, ctx, res, case, queries=True):
    name, pts, gate = case.name, _f32(case.pts), case.gate
    tgt = capi.Target.points(ctx, pts, cell_hint=case.h)
    probe = capi.Scan(ctx, pts, flags=capi.FLAG_NO_SCAN_SORT)
    with ctx.pipeline(variant=1, reuse=0):
        for _ in range(WARM):
            capi.linearize(tgt, probe, capi.ICP, np.eye(4), gate)
    pos = probe.matches()                              # cell-sorted position of every point (of its first twin, if it has twins)
    res[name + "/pos"] = pos
    info = tgt.index_info()
    res[name + "/dims"], res[name + "/cell"] = np.array(info["dims"]), np.array(info["cell"])
    res[name + "/sets"] = np.array(info["list_sets"], np.float64)
    res[name + "/form"] = np.array([info["heavy"], info["x_ordered"]], np.int64)
    back = np.full(pts.shape[0], pts.shape[0], np.int64)
    ok = pos >= 0
    np.minimum.at(back, pos[ok], np.nonzero(ok)[0])    # twins share a record's distance: the smaller original index
    q = _f32(case.q)
    if queries:                                        # (no query reads a deeper list set: once per process)
        res[name + "/nn_d"], res[name + "/nn_i"] = tgt.nn_query(q, gate)
        res[name + "/nn_d_inf"], res[name + "/nn_i_inf"] = tgt.nn_query(q)
        for k in KS:
            res[f"{name}/knn{k}_d"], res[f"{name}/knn{k}_i"] = tgt.knn_query(q, k)
        res[name + "/radius"] = tgt.radius_count(q, RADIUS_CELLS * case.h)
    for frame in FRAMES:
        scan, poses = case.scan(frame), case.poses(frame)
        key = f"{name}/{frame}"
        sc = capi.Scan(ctx, scan, flags=capi.FLAG_NO_SCAN_SORT)
        idx, sums = [], []
        with ctx.pipeline(variant=1, reuse=0):
            for P in poses:                            # each after the pose before it: the step picks the set
                sums.append(capi.linearize(tgt, sc, capi.ICP, P, gate).copy())
                mt = sc.matches()
                idx.append(np.where(mt >= 0, back[np.maximum(mt, 0)], -1))
        res[key + "/idx"], res[key + "/sums"] = np.stack(idx), np.stack(sums)
        with ctx.pipeline(variant=0, reuse=0):
            res[key + "/fused"] = np.stack([capi.linearize(tgt, sc, capi.ICP, P, gate).copy() for P in poses])
        with ctx.pipeline(variant=1, reuse=1):
            res[key + "/reuse"] = np.stack([capi.linearize(tgt, sc, capi.ICP, P, gate).copy() for P in poses])
        sorted_sc = capi.Scan(ctx, scan)               # in the device's own order: what a caller's scan is
        with ctx.pipeline(variant=1, reuse=0):         # (_sums_both gates at its own module's distance)
            split = [capi.linearize(tgt, sorted_sc, capi.ICP, P, gate).copy() for P in poses[::5]]
        with ctx.pipeline(variant=0, reuse=0):
            fused = [capi.linearize(tgt, sorted_sc, capi.ICP, P, gate).copy() for P in poses[::5]]
        res[key + "/sorted"] = np.stack([np.stack(split), np.stack(fused)])
        both = capi.FLAG_ICP_RR_QUIRK
        for lname, flag in (("device", capi.FLAG_DEVICE_LOOP), ("host", capi.FLAG_HOST_LOOP)) if case.loops_in(frame) else ():
            with ctx.pipeline(variant=1, reuse=0):     # (any error, a singular system included, ends the run)
                T, it, trace = capi.align(tgt, sorted_sc, capi.ICP, poses[0], LOOP_ITERS, 1e-3, gate, flags=both | flag, want_trace=True)
            res[f"{key}/{lname}"] = np.concatenate([np.asarray(T, np.float64).reshape(-1), [float(it)], trace[:it].reshape(-1)])
        if not case.loops_in(frame):
            sorted_sc.close(); sc.close()
            continue
        batch = capi.ScanBatch(ctx, [scan, scan[:500]])

        Tb, itb, stb = capi.align_batch(tgt, batch, capi.ICP, np.stack([poses[0], poses[1]]), LOOP_ITERS, 1e-3, gate)
        res[key + "/batch"] = np.concatenate([np.asarray(Tb).reshape(-1), np.asarray(itb, np.float64), np.asarray(stb, np.float64)])
        batch.close(); sorted_sc.close(); sc.close()
    probe.close(); tgt.close()


def run_all(capi, ctx, queries=True):
    res = {}
    for case in cases():
        run_case(capi, ctx, res, case, queries)
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from point_cloud_registration_amd import _capi
    np.savez(sys.argv[1], **run_all(_capi, _capi.get_context(0)))
