"""The float64 query seam on the GPU (csrc/seam64.hip): ``KDTree(float64 data).query(float64 points, k)`` and
``VoxelGrid.kdtree.query`` against the NumPy brute force of tests/seam_f64_cases.py -- indices AND distances bit for bit,
rows in (distance, index) order -- on inputs where rounding the query or the target to float32 changes hundreds of answers
(tests/test_seam_f64_cases.py), and against the reference's own float64 tree (tests/golden/g17_seam_f64.npz)."""
import numpy as np
import pytest

import seam_f64_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from point_cloud_registration_amd import _capi
    assert _capi.device_count() >= 1, "no MI355X visible"
    return _capi


@pytest.fixture(scope="module")
def trees(capi):
    """case -> (target, float64 queries, KDTree over the float64 target): built once, left unchanged."""
    import point_cloud_registration_amd as pcr
    out = {}
    for name, case in (("A", sc.case_a), ("B", sc.case_b)):
        target, q = case()
        tree = pcr.KDTree(target)
        assert tree._target.has_f64
        out[name] = (target, q, tree)
    return out


@pytest.fixture(scope="module")
def brute65():
    """(case, rounded) -> the 65 nearest by brute force, once; the first k columns are the answer for every k <= 65."""
    memo = {}

    def get(name, rounded=False):
        if (name, rounded) not in memo:
            target, q = {"A": sc.case_a, "B": sc.case_b}[name]()
            memo[name, rounded] = sc.brute(target, q.astype(np.float32) if rounded else q, 65)
        return memo[name, rounded]
    return get


@pytest.fixture(scope="module")
def grid(capi):
    import point_cloud_registration_amd as pcr
    g = pcr.VoxelGrid(1.0)
    g.set_points(sc.case_c_cloud())
    assert g.mean.dtype == np.float64 and g.mean.shape == (1493, 3)
    return g


@pytest.mark.parametrize("name", ["A", "B"])
def test_float64_queries_nearest(trees, brute65, name):
    """1. k = 1 with float64 queries, unbounded and bounded.  (Fails without the float64 query path: the queries are
    rounded to float32 and 400 of A's, 397 of B's neighbours move.)"""
    target, q, tree = trees[name]
    d2, io = (x[:, 0] for x in brute65(name))
    do = np.sqrt(d2)
    d, i = tree.query(q)
    assert d.dtype == np.float64 and d.shape == (len(q),)
    print(f"case {name}: {int((np.asarray(i) != io).sum())} of {len(q)} indices differ from the brute force")
    assert np.array_equal(i, io)
    assert np.array_equal(d, do)
    r = float(np.median(do))
    db, ib = tree.query(q, distance_upper_bound=r)
    inside = do < r
    assert 0 < inside.sum() < len(q)
    assert np.array_equal(ib, np.where(inside, io, -1))
    assert db.dtype == np.float64 and np.array_equal(db, np.where(inside, do, np.inf))


@pytest.mark.parametrize("rounded", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name,k", [("B", 2), ("B", 4), ("B", 17), ("B", 64), ("A", 5)])
def test_float64_tree_knn(trees, brute65, name, k, rounded):
    """2. k > 1 on a float64 tree ranks the float64 coordinates, for float64 queries and for their float32 roundings (as
    a float32 array).  (Fails without the float64 k-NN: the float32 copy of B holds 1256 of its 2000 pairs as one point.)"""
    target, q, tree = trees[name]
    d2, io = (x[:, :k] for x in brute65(name, rounded))
    d, i = tree.query(q.astype(np.float32) if rounded else q, k)
    assert d.dtype == np.float64 and d.shape == i.shape == (len(q), k)
    print(f"case {name}, k = {k}: {int(np.any(np.asarray(i) != io, axis=1).sum())} of {len(q)} rows differ from the brute force")
    assert np.array_equal(i, io)
    assert np.array_equal(d, np.sqrt(d2))


def test_knn_beyond_the_size_of_the_target(capi):
    """3. k = 64 on 40 points: columns 40..63 are inf / n; k outside [1, 64] is refused and the target still answers."""
    import point_cloud_registration_amd as pcr
    target, q = sc.case_b()
    target, q = np.ascontiguousarray(target[:40]), q[:20]
    tree = pcr.KDTree(target)
    assert tree._target.has_f64
    d2, io = sc.brute(target, q, 64)
    d, i = tree.query(q, 64)
    assert np.array_equal(i, io) and np.array_equal(d, np.sqrt(d2))
    assert np.all(np.isinf(d[:, 40:])) and np.all(i[:, 40:] == 40) and np.all(np.isfinite(d[:, :40]))
    for k in (0, 65):
        with pytest.raises(ValueError):
            tree.query(q, k)
    d, i = tree.query(q, 2)
    assert np.array_equal(i, io[:, :2]) and np.array_equal(d, np.sqrt(d2[:, :2]))


def test_voxel_grid_float64_queries(grid):
    """4. The centroid tree with float64 queries, k = 1, 3 and 20, and VoxelGrid.query on the same points."""
    q = sc.case_c_queries(grid.mean)
    d2, io = sc.brute(grid.mean, q, 20)
    d, i = grid.kdtree.query(q)
    assert d.dtype == np.float64 and np.array_equal(i, io[:, 0]) and np.array_equal(d, np.sqrt(d2[:, 0]))
    for k in (3, 20):
        dk, ik = grid.kdtree.query(q, k)
        assert dk.dtype == np.float64 and dk.shape == (len(q), k)
        assert np.array_equal(ik, io[:, :k]) and np.array_equal(dk, np.sqrt(d2[:, :k])), k
    out = grid.query(q, ["mean"])
    assert np.array_equal(out["dist"], d) and np.array_equal(out["mean"], grid.mean[io[:, 0]])


def test_float32_doors_are_unchanged(capi, trees, g9):
    """5. float32 queries with k = 1 on the float64 tree: the fixture's float64-tree neighbours, as before; a float32 tree
    answers k = 5 in float32, exactly as Target.knn_query."""
    import point_cloud_registration_amd as pcr
    target, q, tree = trees["A"]
    assert g9["source_tie"].dtype == np.float32
    d, i = tree.query(g9["source_tie"])
    assert d.dtype == np.float64 and np.array_equal(i, g9["nn_idx_f64_tree"])
    assert np.allclose(d, g9["nn_dist_f64_tree"], rtol=1e-12)
    t32, q32 = target.astype(np.float32), q.astype(np.float32)
    tree32 = pcr.KDTree(t32)
    assert not getattr(tree32._target, "has_f64", False)
    d5, i5 = tree32.query(q32, k=5)
    dt, it = tree32._target.knn_query(q32, 5)
    assert d5.dtype == np.float32 and dt.dtype == np.float32
    assert np.array_equal(d5, dt) and np.array_equal(i5, it)
    # the float64 entry points refuse a float32-only point target, and an empty query array is a no-op on the others
    dist, idx = np.empty(len(q)), np.empty(len(q), np.int64)
    assert capi.lib().pcr_nn_query_dd(tree32._target.handle, q, len(q), np.inf, dist, idx) == capi.PCR_ERR_INVALID
    assert capi.lib().pcr_knn_query_f64(tree32._target.handle, q, len(q), 1, dist, idx) == capi.PCR_ERR_INVALID
    assert capi.lib().pcr_nn_query_dd(tree._target.handle, q[:0].copy(), 0, np.inf, dist[:0].copy(), idx[:0].copy()) == capi.PCR_OK
    assert capi.lib().pcr_knn_query_f64(tree._target.handle, q[:0].copy(), 0, 3, dist[:0].copy(), idx[:0].copy()) == capi.PCR_OK


def test_queries_the_float32_index_cannot_place(trees, grid):
    """6. Queries 1e12 m out along an axis (float32 cannot hold them, and a search that counts rings from the query's own
    cell would never arrive) and one exactly on a target point: the clamped float64 ring search answers, k = 1 and k = 4,
    on the point tree and on the centroid tree.  At 1e12 m the squared distances are ~1e24 with steps of 1.3e8, so whole
    groups of points tie exactly and the index decides, as in the brute force."""
    target, _, tree = trees["B"]
    for pts, tr in ((target, tree), (grid.mean, grid.kdtree)):
        c = pts.mean(axis=0)
        q = np.array([[1e12, c[1], c[2]], [-1e12, c[1], c[2]], [c[0], 1e12, c[2]], [c[0], -1e12, c[2]], [c[0], c[1], -1e12],
                      pts[123]])
        d2, io = sc.brute(pts, q, 4)
        d, i = tr.query(q)
        assert np.array_equal(i, io[:, 0]) and np.array_equal(d, np.sqrt(d2[:, 0]))
        assert d[5] == 0.0 and i[5] == 123
        d4, i4 = tr.query(q, 4)
        assert np.array_equal(i4, io) and np.array_equal(d4, np.sqrt(d2))


def test_reference_parity(trees):
    """7. What the reference's KDTree over the float64 target returns for float64 queries, k = 1 and k = 5."""
    g17 = load_golden("g17_seam_f64.npz")
    target, q, tree = trees["A"]
    assert np.array_equal(g17["query"], q[g17["rows"]]) and len(g17["rows"]) >= 900
    d, i = tree.query(g17["query"])
    assert np.array_equal(i, g17["k1_idx"]) and np.allclose(d, g17["k1_dist"], rtol=1e-12, atol=0.0)
    d5, i5 = tree.query(g17["query"], k=5)
    assert np.array_equal(i5, g17["k5_idx"]) and np.allclose(d5, g17["k5_dist"], rtol=1e-12, atol=0.0)
