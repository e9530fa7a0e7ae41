"""The voxel map's restatement (tests/cpp/vmap_oracle.cpp) against hand-worked values of the contract, docs/VOXEL_MAP.md
section 1: cells at the boundaries, floor on negatives, the two rounding rules of the centroid, what is dropped, the
order-independence, the box and min_count.  Each rule has a mutation of the restatement (truncation for floor, '<' for
'<=' at the box, arrival order for key order) and a test named here that catches it.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import vmap_cases as K
import vmap_oracle as V
from slam_amd import api


def fresh(points=None, leaf=K.LEAF, mutation=V.MUT_NONE):
    m = V.OracleMap(leaf, mutation)
    dropped = m.integrate(points) if points is not None else 0
    return m, dropped


# ------------------------------------------------------------------ cells
def boundary_cells(mutation=V.MUT_NONE):
    pts, _ = K.boundary_points()
    m, dropped = fresh(pts, mutation=mutation)
    assert dropped == 0
    xyz4, count, key, sums = m.extract()
    return list(V.cells_of(key)[0]), list(count), xyz4


def test_boundaries_at_a_dyadic_leaf():
    ix, count, xyz4 = boundary_cells()
    # -0.25 alone in cell -1; -0.0, 0.0 and 0.25 - ulp in cell 0; 0.25 alone in cell 1
    assert ix == [-1, 0, 1] and count == [1, 3, 1]
    assert xyz4[0, 0] == K.F(-0.25) and xyz4[2, 0] == K.F(0.25)
    # cell 0: fixed-point values 0, 0 and rint((0.25 - 2^-26) 2^20) = 262144 (2^18 - 1/64 rounds to 2^18)
    assert xyz4[1, 0] == K.F((262144.0 / 3.0) * K.U)


def negative_cells(mutation=V.MUT_NONE):
    pts, _ = K.negative_points()
    m, _ = fresh(pts, mutation=mutation)
    return sorted(zip(*[list(c) for c in V.cells_of(m.extract()[2])]))


def test_floor_not_truncation_on_negatives():
    want = K.negative_points()[1]
    assert negative_cells() == sorted((c, c, c) for c in want)


def test_mutation_truncation_is_caught():
    """The restatement with trunc() for floor() fails the two tests above's expectations."""
    want = K.negative_points()[1]
    assert negative_cells(V.MUT_TRUNCATE) != sorted((c, c, c) for c in want)
    ix, count, _ = boundary_cells(V.MUT_TRUNCATE)
    assert (ix, count) == ([-1, 0, 1], [1, 3, 1])    # the boundary points alone do not tell them apart: -0.25 / 0.25 is -1 either way
    assert negative_cells(V.MUT_TRUNCATE) == [(-1, -1, -1), (0, 0, 0), (1, 1, 1)]


def test_centroid_rounding_rules():
    pts, want_sums, want_c = K.rounding_points()
    m, dropped = fresh(pts)
    xyz4, count, key, sums = m.extract()
    assert dropped == 0 and len(key) == 1 and count[0] == 3 and key[0] == V.key_of(0, 0, 0)
    assert tuple(int(s) for s in sums[0]) == want_sums
    assert tuple(xyz4[0, :3]) == want_c and xyz4[0, 3] == 0
    # half-up or truncating fixed point would have given S = 6 or 3 on x
    assert sums[0, 0] not in (3, 6)


def test_dropped_points_are_counted():
    pts, want_dropped = K.dropped_points()
    m, dropped = fresh(pts)
    assert dropped == want_dropped and m.n_points == len(pts) - want_dropped == 2 and m.n_voxels == 2
    ix = V.cells_of(m.extract()[2])[0]
    assert list(ix) == [0, (1 << 20) - 1]
    for row in pts[1:8]:
        assert fresh(row[None])[1] == 1          # each of them on its own


def test_key_layout():
    m, _ = fresh(np.array([[0.3, -0.3, 0.6]], K.F))      # cells 1, -2, 2
    assert m.extract()[2][0] == V.key_of(1, -2, 2) == ((2 + (1 << 20)) << 42) | (((1 << 20) - 2) << 21) | ((1 << 20) + 1)


# ------------------------------------------------------------------ order
def integrate_all(order, reverse_points=False, mutation=V.MUT_NONE, leaf=K.LEAF):
    m = V.OracleMap(leaf, mutation)
    for i in order:
        pts, (R, t) = K.FOUR_CLOUDS[i]
        m.integrate(pts[::-1] if reverse_points else pts, R, t)
    return m


def test_any_order_of_points_and_clouds_gives_the_same_bits():
    base = integrate_all(K.ORDERS[0]).extract()
    assert len(base[2]) > 500 and base[1].max() > 3
    for order in K.ORDERS[1:]:
        assert K.same_map(integrate_all(order).extract(), base)
    assert K.same_map(integrate_all(K.ORDERS[0], reverse_points=True).extract(), base)
    rng = np.random.default_rng(5)
    m = V.OracleMap(K.LEAF)
    for i in (1, 3, 0, 2):
        pts, (R, t) = K.FOUR_CLOUDS[i]
        m.integrate(pts[rng.permutation(len(pts))], R, t)
    assert K.same_map(m.extract(), base)


def test_extraction_is_in_key_order():
    key = integrate_all(K.ORDERS[2]).extract()[2]
    assert np.all(key[1:] > key[:-1])


def test_mutation_arrival_order_is_caught():
    base = integrate_all(K.ORDERS[0]).extract()
    mut = integrate_all(K.ORDERS[0], mutation=V.MUT_ARRIVAL_ORDER).extract()
    assert not np.all(mut[2][1:] > mut[2][:-1])
    assert not K.same_map(mut, integrate_all(K.ORDERS[1], mutation=V.MUT_ARRIVAL_ORDER).extract())
    assert sorted(mut[2]) == list(base[2])


def test_transform_arithmetic():
    """q = (float)(((r0 x + r1 y) + r2 z) + t) in double, term by term: numpy's elementwise arithmetic contracts nothing."""
    pts, (R, t) = K.FOUR_CLOUDS[1]
    p = pts.astype(np.float64)
    q = np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], axis=1).astype(K.F)
    a, b = V.OracleMap(K.LEAF), V.OracleMap(K.LEAF)
    a.integrate(pts, R, t)
    b.integrate(q)
    assert K.same_map(a.extract(), b.extract())


# ------------------------------------------------------------------ the box and min_count
def box_case(mutation=V.MUT_NONE):
    """Voxels whose centroids are exact floats: one point each at the centre of cells (i, j, 0), i, j = 0 .. 3."""
    c = (np.arange(4) + 0.5) * K.LEAF
    pts = np.array([(x, y, 0.1) for y in c for x in c], K.F)
    m, _ = fresh(pts, mutation=mutation)
    lo, hi = (K.F(c[1]), K.F(c[0])), (K.F(c[2]), K.F(c[2]))   # both ends of both axes lie on centroids
    return m, lo, hi


def test_box_keeps_both_ends():
    m, lo, hi = box_case()
    xyz4, count, key, _ = m.extract(lo, hi)
    ix, iy, _ = V.cells_of(key)
    assert sorted(zip(ix, iy)) == sorted((i, j) for i in (1, 2) for j in (0, 1, 2))
    assert len(m.extract()[2]) == 16


def test_mutation_open_box_is_caught():
    m, lo, hi = box_case(V.MUT_OPEN_BOX)
    ix, iy, _ = V.cells_of(m.extract(lo, hi)[2])
    assert len(ix) == 0 or sorted(zip(ix, iy)) != sorted((i, j) for i in (1, 2) for j in (0, 1, 2))


def test_min_count():
    m = integrate_all(K.ORDERS[0])
    allv = m.extract()
    for mc in (0, 1, 2, 5):
        got = m.extract(min_count=mc)
        keep = allv[1] >= mc
        assert keep.sum() > 0 and K.same_map(got, tuple(a[keep] for a in allv))
    assert (allv[1] >= 2).sum() < len(allv[1])


def test_one_full_voxel_and_clear():
    pts = K.one_voxel(2000)
    m, _ = fresh(pts)
    xyz4, count, key, sums = m.extract()
    assert list(count) == [2000] and key[0] == V.key_of(2, 2, 2)
    fx = np.rint(pts.astype(np.float64) * 2.0 ** 20).astype(np.int64)
    assert np.array_equal(sums[0], fx.sum(axis=0))
    assert np.array_equal(xyz4[0, :3], ((fx.sum(axis=0).astype(np.float64) / 2000.0) * K.U).astype(K.F))
    m.clear()
    assert m.n_voxels == 0 and m.n_points == 0 and len(m.extract()[2]) == 0


# ------------------------------------------------------------------ the binding's struct
def test_params_struct_mirrors_the_header():
    size, off_leaf, off_cap = V.params_layout()
    assert C.sizeof(api.VmapParams) == size
    assert api.VmapParams.leaf.offset == off_leaf and api.VmapParams.initial_capacity.offset == off_cap


# ------------------------------------------------------------------ the builder loop on the restatement
# Recorded on the CPU when the test was written (leaf 0.30, gate 2.0, at most 100 iterations; clouds k = 0 .. 5 of
# make_cloud3d(k, n_loop=50, rings=16, n_az=512), 8 192 points each; oracle_lib.voxel_downsample as the store's filter):
#   step  map points  scan points  iterations  state      fitness  error vs truth (3-D m, yaw)  smallest stop margin
#   1     3 666       3 608        5           TRANSFORM  0.0498   2.59 mm, 0.040 mrad          0.776
#   2     5 235       3 641        5           TRANSFORM  0.0440   4.00 mm, 0.112 mrad          0.975
#   3     6 370       3 672        5           TRANSFORM  0.0420   3.67 mm, 0.097 mrad          0.965
#   4     7 362       3 680        5           TRANSFORM  0.0388   2.90 mm, 0.110 mrad          0.963
#   5     8 238       3 730        5           TRANSFORM  0.0391   3.70 mm, 0.071 mrad          0.946
# The map ends at 9 049 voxels, the fullest holding 57 points.  Cloud k = 25 from the last pose: 22 iterations, TRANSFORM,
# fitness 0.2191 over 3 726 pairs (accepted at MAX_SCORE 1.0).  A cloud shifted by 1 km: NO_CORRESPONDENCES, no pairs.
RECORDED_ERR = [(2.59e-3, 0.040e-3), (4.00e-3, 0.112e-3), (3.67e-3, 0.097e-3), (2.90e-3, 0.110e-3), (3.70e-3, 0.071e-3)]


def build_six():
    """the six clouds through the restated builder: (builder, clouds, per-step rows)"""
    clouds = V.builder_clouds()
    b = V.OracleBuilder()
    rows = []
    for k, (c, pose) in enumerate(clouds):
        ok, r = b.add_cloud(c)
        if k == 0:
            assert ok and r is None
            continue
        err = V.pose_error(r["transform"], V.truth_in_first_frame(clouds[0][1], pose))
        rows.append((ok, b.last_sizes, r, err))
        print("step %d: map %d scan %d iterations %d state %d fitness %.4f error %.2f mm %.3f mrad margin %.3g" %
              (k, b.last_sizes[0], b.last_sizes[1], r["iterations"], r["state"], r["fitness"], err[0] * 1e3, err[1] * 1e3, r["margin"]))
    count = b.vmap.extract()[1]
    print("map: %d voxels, the fullest holds %d points" % (len(count), count.max()))
    return b, clouds, rows


@pytest.fixture(scope="module")
def built():
    """build_six() once for the tests that only read it"""
    return build_six()


def test_builder_accepts_the_five_clouds(built):
    b, clouds, rows = built
    assert len(rows) == 5 and all(ok for ok, _, _, _ in rows)
    for (ok, sizes, r, err), rec in zip(rows, RECORDED_ERR):
        assert r["state"] == api.KF_TRANSFORM and r["converged"] and r["fitness_pairs"] > 0
        # twice the recorded value: the bound guards the inputs (a changed scene or filter), not the device
        assert err[0] <= 2 * rec[0] and err[1] <= 2 * rec[1], (err, rec)
    # the sequence runs both target paths of kf_gicp_kernel: the map passes the 6 144-point LDS staging boundary
    assert rows[1][1][0] <= 6144 < rows[2][1][0]
    assert b.vmap.n_points == 6 * 8192


def test_builder_rejects_a_bad_cloud_and_goes_on():
    from slam_amd import synth
    b, clouds, rows = build_six()              # a builder of its own: it changes MAX_SCORE and the map
    bad = synth.make_cloud3d(25, n_loop=50, rings=16, n_az=512)[0]
    ok, r = b.register(bad)
    worst_good = max(row[2]["fitness"] for row in rows)
    print("cloud 25 from the last pose: accepted %d at MAX_SCORE 1.0, %d iterations, fitness %.4f; largest accepted fitness %.4f" %
          (ok, r["iterations"], r["fitness"], worst_good))
    assert r["fitness"] > 2 * worst_good       # the two populations are apart: their geometric mean separates them
    b.MAX_SCORE = float(np.sqrt(r["fitness"] * worst_good))
    before, pose = b.vmap.extract(), b.trans_full.copy()
    ok, r = b.add_cloud(bad)
    assert not ok and r["fitness"] > b.MAX_SCORE and r["fitness_pairs"] > 0
    assert K.same_map(b.vmap.extract(), before) and np.array_equal(b.trans_full, pose)
    # a cloud a kilometre away: no pairs
    ok, r = b.add_cloud(clouds[3][0] + np.float32([1000, 0, 0]))
    assert not ok and r["fitness_pairs"] == 0 and r["state"] == api.KF_NO_CORRESPONDENCES
    assert K.same_map(b.vmap.extract(), before) and np.array_equal(b.trans_full, pose)
    # a good cloud after them is accepted, at the tightened score
    c6, p6 = synth.make_cloud3d(6, n_loop=50, rings=16, n_az=512)
    ok, r = b.add_cloud(c6)
    err = V.pose_error(r["transform"], V.truth_in_first_frame(clouds[0][1], p6))
    print("cloud 6 after the rejections: fitness %.4f, error %.2f mm %.3f mrad" % (r["fitness"], err[0] * 1e3, err[1] * 1e3))
    assert ok and r["fitness"] <= b.MAX_SCORE and err[0] <= 2 * max(e[0] for e in RECORDED_ERR)
    assert b.vmap.n_points == 7 * 8192 and not np.array_equal(b.trans_full, pose)
