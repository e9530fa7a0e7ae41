"""The exhaustive lattice pose search without a device (docs/VOXEL_MAP.md section 13): the restatement
tests/vmap_search_cases.py on a hand-worked case, around zero, on ties, on the suppression box; its mutations, each caught by a
named test; the scene of section 9.5 / 11.4, where the restatement alone must find the truth's neighbourhood and the restated
relocalize the truth; and the library's entry points as far as they go without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import map_localizer_cases as ML
import vmap_oracle as V
import vmap_search_cases as SC
from slam_amd import api, build
from test_cabi_cpu import header_functions

SYMBOLS = ("slam_vmap_default_search_params", "slam_vmap_search_dev", "slam_vmap_search", "slam_vmap_search_keyframe")


def scores(hits):
    return [(h["score"], h["k"], h["dx"], h["dy"], h["dz"]) for h in hits]


# ------------------------------------------------------------------ the cell rule in numpy is the oracle map's
def test_the_numpy_cells_are_the_oracle_maps_cells():
    cloud = V.builder_clouds([0])[0][0][:2000]
    p = SC.params(yaw0=0.3, n_yaw=7, cx=-3.25, cy=1.75, cz=0.4)
    for leaf in (0.30, 1.0):
        for k in (0, 3):
            M = SC.rotation(p, k).astype(np.float64)
            om = V.OracleMap(leaf)
            assert om.integrate(cloud, M[:3, :3], M[:3, 3]) == 0
            _, count, key, _ = om.extract()
            cells, has = SC.moved_cells(cloud, SC.rotation(p, k), leaf)
            assert has.all()
            u, n = np.unique(np.array([V.key_of(*c) for c in cells.tolist()], np.uint64), return_counts=True)
            assert np.array_equal(u, key) and np.array_equal(n, count) and (cells.min() < 0 < cells.max())


# ------------------------------------------------------------------ the hand-worked case
def test_hand_worked_case():
    """Leaf 1, centre 0, n_yaw 4, window 1/1/0.  The points' cells are A = (0 0), (1 0), (0 2) (z = 0 throughout), the voxels
    V = (0 0), (1 0), (0 2), (-1 -1).  A quarter turn takes the centre of cell (x y) to that of (-y - 1, x), so under k = 1, 2, 3
    the cells are (-1 0) (-1 1) (-3 0); (-1 -1) (-2 -1) (-1 -3); (0 -1) (0 -2) (2 -1).  The score of (k, dx, dy) is the number of
    cells c with c + (dx dy) in V; rows are dy = -1, 0, 1 and columns dx = -1, 0, 1:
      k = 0   1 0 0 / 1 3 1 / 0 0 0      (0 0): all three; (-1 -1): (0 0) -> (-1 -1); (-1 0): (1 0) -> (0 0); (1 0): (0 0) -> (1 0)
      k = 1   0 1 1 / 0 0 1 / 0 0 1      (0 -1): (-1 0) -> (-1 -1); (1 -1): (-1 1) -> (0 0); (1 0): (-1 0) -> (0 0); (1 1): (-1 1) -> (0 2)
      k = 2   0 0 0 / 0 1 1 / 0 0 1      (0 0): (-1 -1); (1 0): (-2 -1) -> (-1 -1); (1 1): (-1 -1) -> (0 0)
      k = 3   0 0 0 / 1 0 0 / 2 1 1      (-1 0): (0 -1) -> (-1 -1); (-1 1): (0 -2) -> (-1 -1) and (2 -1) -> (1 0); (0 1): (0 -1) -> (0 0);
                                         (1 1): (0 -1) -> (1 0)"""
    qual = SC.qualifying(SC.map_of(SC.HAND_VOXELS), False, 1)
    assert qual == SC.HAND_VOXELS
    hits, vol, nwc = SC.search(SC.HAND_POINTS, qual, 1.0, SC.HAND_PARAMS)
    assert vol[:, 0].tolist() == [[[1, 0, 0], [1, 3, 1], [0, 0, 0]], [[0, 1, 1], [0, 0, 1], [0, 0, 1]],
                                  [[0, 0, 0], [0, 1, 1], [0, 0, 1]], [[0, 0, 0], [1, 0, 0], [2, 1, 1]]]
    assert nwc.tolist() == [3, 3, 3, 3]
    # nms 0 / 0 suppresses the hit alone: the 3, the 2, then the ones in flat order
    assert scores(hits) == [(3, 0, 0, 0, 0), (2, 3, -1, 1, 0), (1, 0, -1, -1, 0), (1, 0, -1, 0, 0), (1, 0, 1, 0, 0), (1, 1, 0, -1, 0),
                            (1, 1, 1, -1, 0), (1, 1, 1, 0, 0)]
    # a hit's init: planar of the float yaw, the offset times the leaf added to the centre in double
    h = hits[1]
    yaw = np.float32(2.0 * math.pi * 3 / 4)
    c, s = np.float32(math.cos(float(yaw))), np.float32(math.sin(float(yaw)))
    assert h["init"].tobytes() == np.array([[c, -s, 0, -1], [s, c, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32).tobytes()
    assert SC.same_hits(SC.search(SC.HAND_POINTS, qual, 1.0, SC.HAND_PARAMS, dense=True)[0], hits)


AROUND_ZERO = np.array([(x, 0.25, 0.25) for x in (-1.5, -0.5, 0.5, 1.5)], np.float32)            # cells -2 .. 1


def around_zero_search(mutation=SC.MUT_NONE):
    """cells -2 .. 1 at leaf 1 against the voxels two cells to the left: the only full score is at dx = -2"""
    p = SC.params(n_yaw=1, wx=3, wy=0, wz=0, top_m=1)
    return SC.search(AROUND_ZERO, {(x, 0, 0) for x in (-4, -3, -2, -1)}, 1.0, p, mutation)


def test_cells_around_zero_floor_with_negative_offsets():
    cells, has = SC.moved_cells(AROUND_ZERO, SC.rotation(SC.params(n_yaw=1), 0), 1.0)
    assert has.all() and cells[:, 0].tolist() == [-2, -1, 0, 1]
    hits, vol, _ = around_zero_search()
    assert vol[0, 0, 0].tolist() == [3, 4, 3, 2, 1, 0, 0] and scores(hits) == [(4, 0, -2, 0, 0)]


def four_fold_search(mutation=SC.MUT_NONE, **kw):
    """the points are the voxels' centres and the set maps onto itself under a quarter turn: every rotation scores all of them"""
    cells = SC.four_fold()
    p = SC.params(n_yaw=4, wx=1, wy=1, wz=0, **kw)
    return SC.search(SC.cell_centres(cells), cells, 1.0, p, mutation), len(cells)


def test_four_fold_tie_goes_to_the_lowest_flat_index():
    (hits, vol, _), n = four_fold_search(top_m=4, nms_yaw=0, nms_cells=0)
    assert n == 12 and vol[:, 0, 1, 1].tolist() == [12] * 4 and int(vol.max()) == 12
    assert scores(hits) == [(12, k, 0, 0, 0) for k in range(4)]


def wrap_search(mutation=SC.MUT_NONE):
    """n_yaw 8: the four quarter turns k = 0, 2, 4, 6 score alike.  k = 0 is taken first and with nms_yaw 2 suppresses k = 6, 7, 0, 1
    and 2, whatever they hold; k = 4 follows and suppresses the rest.  The box around dx = dy = 0 is clipped at the window's
    edge (half-width 1, nms_cells 2)."""
    cells = SC.four_fold()
    p = SC.params(n_yaw=8, wx=1, wy=1, wz=0, top_m=8, nms_yaw=2, nms_cells=2)
    return SC.search(SC.cell_centres(cells), cells, 1.0, p, mutation)


def test_suppression_wraps_in_yaw_and_is_clipped_at_the_edge():
    hits, vol, _ = wrap_search()
    assert int(vol[7].max()) > 0 and int(vol[6].max()) == 12                  # k = 6 and 7 are not empty: k = 0 suppresses them
    assert scores(hits) == [(12, k, 0, 0, 0) for k in (0, 4)]


def test_score_zero_is_never_a_hit():
    qual = {(40, 40, 0)}                                                      # out of every pose's reach
    hits, vol, _ = SC.search(SC.HAND_POINTS, qual, 1.0, SC.HAND_PARAMS)
    assert not vol.any() and hits == []
    hits, vol, _ = SC.search(SC.HAND_POINTS, SC.HAND_VOXELS, 1.0, SC.params(n_yaw=4, wx=1, wy=1, wz=0, top_m=64, nms_yaw=0, nms_cells=0))
    assert len(hits) == int((vol > 0).sum()) == 15 and all(h["score"] > 0 for h in hits)
    assert SC.search(SC.HAND_POINTS, SC.HAND_VOXELS, 1.0, dict(SC.HAND_PARAMS, top_m=0))[0] == []


def no_cell_search(mutation=SC.MUT_NONE):
    return SC.search(SC.NO_CELL, {(0, 0, 0)}, 1.0, SC.params(n_yaw=1, wx=0, wy=0, wz=0, top_m=1), mutation)


def test_points_without_a_cell_count_nowhere():
    hits, vol, nwc = no_cell_search()
    assert vol.tolist() == [[[[1]]]] and nwc.tolist() == [1] and hits[0]["n_with_cell"] == 1
    # 2^22 is out and the float below it is in; at a leaf of 2 a cell of 2^20 is out
    edge = np.array([(np.nextafter(np.float32(4194304.0), np.float32(0)), 0, 0), (4194304.0, 0, 0)], np.float32)
    assert SC.moved_cells(edge, np.eye(4, dtype=np.float32), 4.0)[1].tolist() == [True, False]
    assert SC.moved_cells(edge[:1], np.eye(4, dtype=np.float32), 2.0)[1].tolist() == [False]


def test_a_cell_beyond_the_limit_holds_no_voxel():
    """|c + d| >= 2^20 holds none, even were the set to name it"""
    far = float(np.float32((1 << 20) - 0.5))
    pts = np.array([(far, 0.5, 0.5)], np.float32)
    qual = {((1 << 20) - 1, 0, 0), (1 << 20, 0, 0)}
    _, vol, _ = SC.search(pts, qual, 1.0, SC.params(n_yaw=1, wx=1, wy=0, wz=0))
    assert vol[0, 0, 0].tolist() == [0, 1, 0]


def test_dense_and_set_lookups_give_the_same_integers():
    rng = np.random.default_rng(5)
    pts = (rng.random((200, 3)) * [12, 12, 3] - [6, 6, 1]).astype(np.float32)
    pts[::17, 0] = np.nan
    qual = set(map(tuple, rng.integers(-7, 7, (300, 3)).tolist()))
    p = SC.params(n_yaw=5, yaw0=0.2, cx=0.5, cy=-0.25, cz=0.1, wx=3, wy=2, wz=1)
    a, b = SC.search(pts, qual, 1.0, p), SC.search(pts, qual, 1.0, p, dense=True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and SC.same_hits(a[0], b[0]) and len(a[0]) == 4


def test_refusals_of_the_restatement():
    assert not SC.refused(SC.params()) and not SC.refused(SC.params(n_yaw=1 << 26, wx=0, wy=0))
    for bad in (dict(n_yaw=0), dict(wx=-1), dict(wy=-1), dict(wz=-1), dict(top_m=-1), dict(n_yaw=(1 << 26) + 1, wx=0, wy=0),
                dict(n_yaw=64, wx=512, wy=512, wz=0), dict(nms_yaw=-1), dict(nms_cells=-1), dict(top_m=4097)):
        assert SC.refused(SC.params(**bad)), bad
    assert SC.refused(SC.params(), n=-1)


# ------------------------------------------------------------------ mutations of the restatement
def test_mutation_truncation_is_caught():
    """test_cells_around_zero_floor_with_negative_offsets' expectation: truncation puts -0.5 and 0.5 into one cell"""
    hits, vol, _ = around_zero_search(SC.MUT_TRUNCATE)
    assert vol[0, 0, 0].tolist() != [3, 4, 3, 2, 1, 0, 0] and scores(hits) != [(4, 0, -2, 0, 0)]


def test_mutation_subtracted_offset_is_caught():
    """test_cells_around_zero_floor_with_negative_offsets' expectation: the full score moves to dx = +2"""
    hits, _, _ = around_zero_search(SC.MUT_SUBTRACT)
    assert scores(hits) == [(4, 0, 2, 0, 0)]


def test_mutation_tie_to_the_highest_index_is_caught():
    """test_four_fold_tie_goes_to_the_lowest_flat_index's expectation"""
    (hits, _, _), _ = four_fold_search(SC.MUT_TIE_HIGH, top_m=4, nms_yaw=0, nms_cells=0)
    assert scores(hits) == [(12, k, 0, 0, 0) for k in (3, 2, 1, 0)]


def test_mutation_suppression_not_cyclic_is_caught():
    """test_suppression_wraps_in_yaw_and_is_clipped_at_the_edge's expectation: k = 7 comes back as a hit"""
    hits, _, _ = wrap_search(SC.MUT_NO_WRAP)
    assert [h["k"] for h in hits] == [0, 4, 7]


def test_mutation_points_without_a_cell_counted_is_caught():
    """test_points_without_a_cell_count_nowhere's expectation: the four land in the cell the rule leaves them, 0 on the bad axis"""
    _, vol, _ = no_cell_search(SC.MUT_COUNT_NO_CELL)
    assert vol.tolist() == [[[[5]]]]


# ------------------------------------------------------------------ the scene of sections 9.5 and 11.4
@pytest.fixture(scope="module")
def world():
    parts, cloud, truth = ML.scene()
    ora = ML.OracleLocalizer(parts, 2)                                        # leaves 1 and 2
    ora.set_scan(cloud)
    return dict(cloud=cloud, truth=truth, ora=ora)


@pytest.mark.parametrize("level", (0, 1))
def test_scene_hit_0_lies_in_the_truths_neighbourhood(world, level):
    """The condition on the inputs: with plane voxels, 64 yaws over the full circle and a window over the whole map -- no prior --
    the restatement's best pose lies within one leaf and one yaw step of the truth.  It does: 0.380 m and 0.0393 rad at leaf 1
    (2 884 of 3 730 points), 1.198 m and 0.0393 rad at leaf 2 (3 340)."""
    m, truth = world["ora"].levels[level], world["truth"]
    cx, cy, w = SC.map_window(m, m.leaf)
    hits, vol, nwc = SC.search(world["ora"].src.xyz, SC.qualifying(m, True), m.leaf, SC.params(cx=cx, cy=cy, wx=w, wy=w), dense=True)
    d, a = SC.hit_offset(hits[0], truth)
    print("leaf %g: window %d cells around (%g, %g), %d poses; hit 0 scores %d of %d, %.3f m %.4f rad from the truth; then %s"
          % (m.leaf, w, cx, cy, vol.size, hits[0]["score"], hits[0]["n_with_cell"], d, a, [h["score"] for h in hits[1:]]))
    assert nwc.tolist() == [len(world["ora"].src.xyz)] * 64
    assert d <= m.leaf and a <= 2 * math.pi / 64
    assert hits[0]["score"] > hits[1]["score"]


def test_scene_restated_relocalize_finds_the_truth_from_no_prior(world):
    ora, truth = world["ora"], world["truth"]
    cx, cy, w = SC.map_window(ora.levels[1], 2.0)
    out = SC.relocalize(ora, world["cloud"], cx, cy, 0.0, 2.0 * w, api.MapLocalizer.MAX_SCORE)
    assert out["found"] and len(out["hits"]) == 4
    e = V.pose_error(out["transform"], truth)
    print("relocalize: hit %d wins, %.3f mm %.4f mrad from the truth" % (out["index"], e[0] * 1e3, e[1] * 1e3))
    assert e[0] * 1e3 <= 2 * ML.RECORDED_MM and e[1] * 1e3 <= 2 * ML.RECORDED_MRAD
    assert all(r is not None for r in out["last"][1])                         # the descent began at level 1 with every hit
    assert (api.MapLocalizer.SEARCH_LEVEL, api.MapLocalizer.SEARCH_YAWS, api.MapLocalizer.SEARCH_STARTS) == (1, 64, 4)


# ------------------------------------------------------------------ the library, as far as it goes without a device
@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def test_the_symbols_are_declared_exported_and_bound(L):
    for s in SYMBOLS:
        assert s in header_functions() and s in api.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes is not None
    assert (len(L.slam_vmap_search_dev.argtypes), len(L.slam_vmap_search.argtypes), len(L.slam_vmap_search_keyframe.argtypes)) == (9, 8, 8)
    assert callable(api.VoxelMap.search) and callable(api.MapLocalizer.search) and callable(api.MapLocalizer.relocalize)
    p = api.vmap_default_search_params()
    assert {f: getattr(p, f) for f, _ in p._fields_} == SC.DEFAULTS and not SC.refused(SC.DEFAULTS)


def calls(L, m, p, n=0, pts=None, stride=3, top=True):
    """the three forms with one set of arguments: their return codes"""
    hits, got = (api.VmapSearchHit * 4096)(), C.c_int(-1)
    store = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    tail = (C.byref(p), hits if top else None, C.byref(got), None)
    return (L.slam_vmap_search_dev(m, pts, n, stride, *tail, None), L.slam_vmap_search(m, pts, n, stride, *tail),
            L.slam_vmap_search_keyframe(m, store, 0, *tail, None))


def test_every_refusal_needs_no_device(L):
    word = np.zeros(64, np.uint64)
    m = word.ctypes.data_as(C.c_void_p)
    pts = np.zeros((4, 3), np.float32).ctypes.data_as(C.c_void_p)
    ok = api.vmap_default_search_params()
    assert calls(L, None, ok) == (api.E_INVALID,) * 3 and b"map is NULL" in L.slam_last_error()
    assert calls(L, m, ok, n=-1, pts=pts)[:2] == (api.E_INVALID,) * 2
    assert calls(L, m, ok, n=4, pts=None)[:2] == (api.E_INVALID,) * 2 and calls(L, m, ok, n=4, pts=pts, stride=2)[:2] == (api.E_INVALID,) * 2
    for bad in (dict(n_yaw=0), dict(wx=-1), dict(wy=-1), dict(wz=-1), dict(top_m=-1), dict(top_m=4097), dict(nms_yaw=-1), dict(nms_cells=-1),
                dict(n_yaw=(1 << 26) + 1, wx=0, wy=0), dict(n_yaw=64, wx=512, wy=512), dict(n_yaw=1, wx=1 << 30, wy=1 << 30, wz=1 << 30)):
        assert SC.refused(SC.params(**bad))
        assert calls(L, m, api.vmap_default_search_params(**bad)) == (api.E_INVALID,) * 3, bad
        assert b"slam_vmap_search" in L.slam_last_error()
    assert calls(L, m, ok, top=False) == (api.E_INVALID,) * 3                 # top_m 4 and nowhere to put the hits
    got = C.c_int()
    assert L.slam_vmap_search_keyframe(m, None, 0, C.byref(ok), None, C.byref(got), None, None) == api.E_INVALID
    assert L.slam_vmap_search_dev(m, None, 0, 3, C.byref(ok), None, None, None, None) == api.E_INVALID


@pytest.mark.skipif(api.device_count() != 0, reason="a GPU is present")
def test_well_formed_arguments_answer_no_device(L):
    m = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    pts = np.zeros((4, 3), np.float32).ctypes.data_as(C.c_void_p)
    assert calls(L, m, api.vmap_default_search_params(), n=4, pts=pts) == (api.E_NO_DEVICE,) * 3
    assert calls(L, m, api.vmap_default_search_params(n_yaw=1 << 26, wx=0, wy=0, top_m=0), top=False) == (api.E_NO_DEVICE,) * 3
