"""CPU only: the cases of tests/magnitude_cases.py are what they claim -- float32 values, grids of the stated size, slack / h on
the stated side of the three list depths and of the cell, enough matches, matches of queries outside the grid box and exact
ties by brute force alone, and on the long grids points whose float32 cell is not their float64 cell."""
import numpy as np
import pytest

import magnitude_cases as mc

CASES = {c.name: c for c in mc.cases()}


@pytest.fixture(scope="module")
def stats():
    """per case, from one table of float32 squared distances: matched, outside the grid box and matched, matched with a tie"""
    out = {}
    for name, c in CASES.items():
        d2 = mc.d2_rows(c.pts, c.q)
        best = d2.min(1)
        matched = np.sqrt(best) < np.float32(c.gate)
        ties = (d2 == best[:, None]).sum(1) > 1
        out[name] = (matched.mean(), (matched & mc.outside(c.pts.min(0), c.h, mc.dims_of(c.pts, c.h), c.q)).mean(),
                     (matched & ties).mean())
    return out


def test_values_are_float32_and_grids_are_as_stated():
    for c in CASES.values():
        assert c.pts.shape == (mc.N_POINTS, 3) and 1150 <= c.q.shape[0] <= 1800, c.name
        assert np.array_equal(mc.snap(c.pts), c.pts) and np.array_equal(mc.snap(c.q), c.q), c.name
        assert np.array_equal(c.pts.min(0), c.D), c.name                   # the grid's origin is D
        want = mc.DIMS if c.family != "long" else tuple(mc.LONG_CELLS[c.axis] if a == c.axis else (4, 3)[[b for b in range(3) if b != c.axis].index(a)]
                                                      for a in range(3))
        assert mc.dims_of(c.pts, c.h) == want, (c.name, mc.dims_of(c.pts, c.h))
        assert np.prod(want) <= 2.1e5
        for frame in mc.FRAMES:
            assert len(c.poses(frame)) == 16
    assert max(np.prod(mc.dims_of(c.pts, c.h)) for c in CASES.values()) >= 1.9e5 and min(mc.LONG_CELLS) >= 1 << 13


def test_lattice_points_and_queries_sit_on_the_lattice():
    for r, (m, h, _) in enumerate(mc.REGIMES):
        c = CASES[f"lattice_r{r}"]
        step, half, ulp = mc.lattice_step(c.D, h)
        assert (step >= ulp).all() and (step >= h / 4 - ulp / 2).all() and (step <= max(h / 4, ulp.max()) + ulp).all()
        k = (c.pts - c.D) / step
        assert np.array_equal(k, np.round(k)), c.name
        kq = (c.q[400:] - c.D) / half
        assert np.array_equal(kq, np.round(kq)), c.name
        assert np.unique(c.pts, axis=0).shape[0] < mc.N_POINTS                                   # twins
        assert (half < step).any() or m >= 2.0 ** 22                                               # half steps wherever float32 has them


def test_slack_lands_on_the_stated_side_of_every_depth():
    seen = set()
    for r, (m, h, stated) in enumerate(mc.REGIMES):
        for fam in ("uniform", "lattice"):
            c = CASES[f"{fam}_r{r}"]
            ratio = mc.slack_of(c.pts, h) / float(np.float32(h))
            assert abs(ratio - stated) <= 0.06 * stated + 0.005, (c.name, ratio, stated)
            for edge in mc.HALOS + (1.0,):
                assert (ratio < edge) == (stated < edge), (c.name, ratio, edge)
        seen.add(sum(stated > e for e in mc.HALOS + (1.0,)))
    # below the near depth, between near and mid (twice), above the far depth, above the cell; no regime of the issue's
    # list falls between the mid and the far depth (0.25 .. 0.35)
    assert seen == {0, 1, 3, 4}
    for axis in "xyz":
        c = CASES["long_" + axis]
        assert mc.slack_of(c.pts, c.h) / c.h < 0.1


def test_brute_force_finds_matches_outside_matches_and_ties(stats):
    for name, (matched, outside, ties) in stats.items():
        print(f"{name}: matched {matched:.3f}, outside the grid box and matched {outside:.3f}, matched with a tie {ties:.3f}")
    for name, (matched, outside, ties) in stats.items():
        fam = CASES[name].family
        if fam == "uniform":
            assert matched >= 0.70, (name, matched)
        if fam == "lattice":
            assert matched >= 0.40 and ties >= 0.10, (name, matched, ties)
        assert outside >= 0.05, (name, outside)


def test_wall_points_share_one_x():
    for r in range(len(mc.REGIMES)):
        c = CASES[f"uniform_r{r}"]
        assert np.unique(c.pts[1500:, 0]).shape[0] == 1
        assert 3.0 <= (c.pts[1500, 0] - c.D[0]) / c.h <= 3.5


def test_long_grid_has_points_in_another_cell_than_float64_says():
    """the cell by the search's float32 arithmetic, floor((x - ox) * float32(1 / h)), against floor((x - ox) / h) in float64"""
    for axis in range(3):
        c = CASES["long_" + "xyz"[axis]]
        for what, a in (("points", c.pts), ("queries", c.q)):
            x = a[:, axis]
            c32 = mc.cell_of(c.D, c.h, a)[:, axis]
            c64 = np.floor((x - c.D[axis]) / c.h).astype(np.int64)
            differ = c32 != c64
            print(f"long_{'xyz'[axis]}: {differ.sum()} {what} in another cell, at cell indices {sorted(set(c64[differ]))[:6]} ...")
            # (every such point sits at a face site; of the queries, the ones on whole faces of cells lower down differ too)
            assert (differ & (c64 >= mc.FACE_FROM)).sum() >= 3, (c.name, what, differ.sum())
            assert what == "queries" or (c64[differ] >= mc.FACE_FROM).all(), c.name
            near = np.abs(x - np.round((x - c.D[axis]) / c.h) * c.h - c.D[axis]) <= 3.5 * np.spacing(np.float32(np.abs(x)).astype(np.float32))
            assert (near & (c64 >= mc.FACE_FROM)).sum() >= (150 if what == "points" else 400), (c.name, what)


def test_long_grid_tie_sites_have_their_match_two_cells_away():
    """the last N_TIE queries of a long grid: at half of them two points exactly equally far, at three quarters the nearest
    point (the smaller index of a tie) in the ring-2 cell, one cell and a few float32 steps away"""
    for axis in range(3):
        c = CASES["long_" + "xyz"[axis]]
        q = c.q[-mc.N_TIE:]
        d2 = mc.d2_rows(c.pts, q)
        best, arg = d2.min(1), d2.argmin(1)
        ring = np.abs(mc.cell_of(c.D, c.h, c.pts[arg])[:, axis] - mc.cell_of(c.D, c.h, q)[:, axis])
        assert ((d2 == best[:, None]).sum(1) == 2).sum() == mc.N_TIE // 2, c.name
        # (by the float32 cell arithmetic; where x - ox is rounded a mirror point may land a cell off its design)
        assert (ring == 2).sum() >= 5 * mc.N_TIE // 8 and (ring >= 1).sum() >= mc.N_TIE - 4, (c.name, np.bincount(ring))
        # (one cell away by the float32 cell arithmetic, whose faces lie within a few float32 steps of ox + c h)
        assert (np.abs(np.sqrt(best) / c.h - 1.0) < 0.003).all(), c.name
        assert (mc.cell_of(c.D, c.h, q)[:, axis] >= mc.FACE_FROM).all()


def test_long_grid_slack_sites_need_the_slack():
    """the N_SLACK queries before the tie sites, by the library's float32 rules restated: the nearest point lies in the next cell
    and, without slack, is not on the list of the query's cell (halo_cells), although it is closer than the certificate of
    ring 0 (nn_certified); the decoy in the query's own cell lies between the two; with the shipped slack the point is listed"""
    f = np.float32
    for axis in range(3):
        c = CASES["long_" + "xyz"[axis]]
        n0 = c.q.shape[0] - mc.N_TIE - mc.N_SLACK
        q = c.q[n0:n0 + mc.N_SLACK]
        d2 = mc.d2_rows(c.pts, q)
        order = np.argsort(d2, axis=1, kind="stable")
        o32, h32, halo = f(c.D[axis]), f(c.h), f(mc.HALOS[0] * c.h)
        slack = mc.slack_of(c.pts, c.h)
        assert slack > 8 * np.spacing(f(np.abs(c.pts[:, axis]).max()))
        for k in range(mc.N_SLACK):
            near, decoy = c.pts[order[k, 0]], c.pts[order[k, 1]]
            cq, cn, cd = (int(mc.cell_of(c.D, c.h, x[None, :])[0, axis]) for x in (q[k], near, decoy))
            assert cn == cq - 1 and cd == cq and cq >= mc.FACE_FROM, (c.name, k)
            assert (mc.cell_of(c.D, c.h, near[None, :])[0] == mc.cell_of(c.D, c.h, q[k][None, :])[0])[[a for a in range(3) if a != axis]].all()
            wall = f(cq) * h32
            to_face = wall - (f(near[axis]) - o32)                       # halo_cells: dh of the point in its own cell
            fx = (f(q[k, axis]) - o32) - wall                            # nn_cell
            lb = fx + halo                                               # nn_certified at ring 1, slack 0
            assert to_face > halo and float(to_face) <= float(halo) + slack, (c.name, k, to_face)
            assert d2[k, order[k, 0]] < d2[k, order[k, 1]] < lb * lb, (c.name, k)
            assert 0 <= fx <= 0.1 * c.h                                  # the face along the axis is the query's nearest
