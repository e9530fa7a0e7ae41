"""The carve restatement (tests/cpp/vmap_carve_oracle.cpp) against hand-worked values of the contract, docs/VOXEL_MAP.md
section 8: which cells a ray visits (directions, ties, floor at the origin, margin, tail, the length limit), the closed form
against the iteration, scans as units, the order-independence, the carved extraction, the structs, the entry points without
a device, and the mover scene.  Each rule has a mutation of the restatement and a test named here that catches it.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import vmap_carve_cases as K
import vmap_carve_oracle as VC
import vmap_oracle as V
from slam_amd import api


def carve_ray(o, q, p, mutation=VC.MUT_NONE):
    """one ray through a map that holds every cell around it: (the cells charged a miss, the voxel map, the counters)"""
    m = VC.CarveOracleMap(K.LEAF, mutation)
    m.integrate(K.box_points(o, q))
    r = m.carve(np.asarray(q, K.F)[None], origin=o, p=p)
    return K.crossed_cells(m), m, r


# ------------------------------------------------------------------ the hand-worked rays
@pytest.mark.parametrize("name", sorted(K.RAYS))
def test_hand_worked_ray(name):
    o, q, p, want = K.RAYS[name]
    got, m, r = carve_ray(o, q, p)
    seen, miss, key = m.read_carve()
    assert r["n_rays"] == 1 and r["n_dropped"] == 0 and r["n_seen"] == 1 and seen.sum() == 1
    if want is None:
        assert (r["n_skipped"], r["n_steps"], r["n_missed"]) == (1, 0, 0) and len(got) == 0
        return
    assert np.array_equal(got, K.sorted_rows(want)), (name, got)
    assert (r["n_skipped"], r["n_steps"], r["n_missed"]) == (0, len(want), len(want)) and miss.max(initial=0) <= 1
    # the walk itself, in order
    c0, c1 = np.floor(o.astype(np.float64) / K.LEAF), np.floor(q.astype(np.float64) / K.LEAF)
    assert np.array_equal(VC.ray_cells(c0, c1, p), want)


def test_the_end_cell_is_never_visited():
    """with no margin and no tail every step but the last is visited: n cells, the end cell not among them"""
    p = VC.params(end_margin=0, tail_num=0)
    cells = VC.ray_cells((0, 0, 0), (5, -3, 2), p)
    assert len(cells) == 5 and not any(np.array_equal(c, (5, -3, 2)) for c in cells) and np.array_equal(cells[0], (0, 0, 0))


def test_closed_form_equals_the_iteration_on_random_rays():
    rng = np.random.default_rng(11)
    for j in range(1500):
        c0 = rng.integers(-50, 50, 3)
        c1 = c0 + rng.integers(-70, 71, 3) * rng.integers(0, 2, 3)       # zero extents and ties among them
        p = VC.params(end_margin=int(rng.integers(0, 3)), tail_num=int(rng.integers(0, 3)), tail_den=int(rng.integers(1, 9)), max_ray_cells=64)
        a, b = VC.ray_cells(c0, c1, p), VC.closed_form_cells(c0, c1, p)
        assert (a is None) == (b is None)
        assert a is None or np.array_equal(a, b), (c0, c1)
    # long rays: the products pass 2^31
    for c1 in ((1 << 20) - 1, 40000, -70001), (-(1 << 20) + 1, (1 << 20) - 1, 3):
        p = VC.params(max_ray_cells=1 << 22)
        assert np.array_equal(VC.ray_cells((1 - (1 << 20), 5, 0), c1, p), VC.closed_form_cells((1 - (1 << 20), 5, 0), c1, p))


# ------------------------------------------------------------------ the mutations
def test_mutation_end_cell_is_caught():
    o, q, p, want = K.RAYS["axis_plus_x"]
    assert len(carve_ray(o, q, p, VC.MUT_END_CELL)[0]) == len(want) + 1
    cells = VC.ray_cells((0, 0, 0), (5, -3, 2), VC.params(end_margin=0, tail_num=0), VC.MUT_END_CELL)
    assert len(cells) == 6 and np.array_equal(cells[-1], (5, -3, 2))      # test_the_end_cell_is_never_visited fails


def test_mutation_ge_for_gt_is_caught():
    o, q, p, want = K.RAYS["tie_xy"]
    got = carve_ray(o, q, p, VC.MUT_GE)[0]
    assert not np.array_equal(got, K.sorted_rows(want))
    assert np.array_equal(VC.ray_cells((0, 0, 0), (4, 4, 2), p, VC.MUT_GE), [(0, 0, 0), (1, 1, 1), (2, 2, 1)])   # z moves a step early


def test_mutation_truncation_is_caught():
    o, q, p, want = K.RAYS["through_zero"]
    got = carve_ray(o, q, p, VC.MUT_TRUNCATE)[0]
    assert np.array_equal(got, [(0, 0, 0), (1, 1, 1)]) and not np.array_equal(got, K.sorted_rows(want))


# ------------------------------------------------------------------ scans as units
O = K.centre((0, 0, 0))
A = K.centre((4, 0, 0))            # ends in cell (4, 0, 0)
B = K.centre((10, 0, 0))           # n 10, T 2: visits cells 0 .. 7, cell (4, 0, 0) among them
KEY4, KEY2 = V.key_of(4, 0, 0), V.key_of(2, 0, 0)


def line_map(mutation=VC.MUT_NONE):
    m = VC.CarveOracleMap(K.LEAF, mutation)
    m.integrate(K.box_points(O, B))
    return m


def at(m, key):
    seen, miss, keys = m.read_carve()
    i = int(np.searchsorted(keys, np.uint64(key)))
    assert keys[i] == key
    return int(seen[i]), int(miss[i])


def planes(m):
    seen, miss, key = m.read_carve()
    return seen.copy(), miss.copy(), key.copy()


def test_within_a_cloud_a_hit_overrides_every_miss():
    for cloud in (np.stack([A, B]), np.stack([B, A])):
        m = line_map()
        r = m.carve(cloud, origin=O)
        assert at(m, KEY4) == (1, 0)
        assert at(m, KEY2) == (0, 1)            # crossed by both rays of the cloud: one scan, one miss
        assert (r["n_seen"], r["n_missed"], r["n_steps"]) == (2, 7, 3 + 8)


def test_mutation_no_hit_protection_is_caught():
    m = line_map(VC.MUT_NO_PROTECTION)
    m.carve(np.stack([A, B]), origin=O)
    assert at(m, KEY4) == (1, 1)


def test_mutation_per_ray_units_is_caught():
    m = line_map(VC.MUT_PER_RAY)
    m.carve(np.stack([A, B, B, A]), origin=O)
    assert at(m, KEY2) == (0, 4) and at(m, KEY4)[0] == 2
    m = line_map()
    m.carve(np.stack([A, B, B, A]), origin=O)
    assert at(m, KEY2) == (0, 1) and at(m, KEY4) == (1, 0)


def test_two_clouds_in_both_orders_and_the_same_cloud_twice():
    a, b = line_map(), line_map()
    a.carve(A[None], origin=O), a.carve(B[None], origin=O)
    b.carve(B[None], origin=O), b.carve(A[None], origin=O)
    assert at(a, KEY4) == at(b, KEY4) == (1, 1)
    assert all(np.array_equal(x, y) for x, y in zip(planes(a), planes(b)))
    once = planes(a)
    a.carve(A[None], origin=O), a.carve(B[None], origin=O)
    twice = planes(a)
    assert np.array_equal(twice[0], 2 * once[0]) and np.array_equal(twice[1], 2 * once[1]) and at(a, KEY4) == (2, 2)


def test_carve_claims_nothing_and_later_voxels_are_not_charged():
    m = VC.CarveOracleMap(K.LEAF)
    m.integrate(K.centre((2, 0, 0))[None])
    before = m.extract()
    r = m.carve(np.stack([A, B]), origin=O)
    assert m.n_voxels == 1 and (r["n_seen"], r["n_missed"], r["n_steps"]) == (0, 1, 11)
    assert K_same(m.extract(), before)
    m.integrate(K.centre((3, 0, 0))[None])
    assert at(m, V.key_of(3, 0, 0)) == (0, 0) and at(m, KEY2) == (0, 1)


def K_same(a, b):
    import vmap_cases
    return vmap_cases.same_map(a, b)


def test_dropped_points_and_an_origin_without_a_cell():
    import vmap_cases
    pts, want_dropped = vmap_cases.dropped_points()
    m = line_map()
    r = m.carve(pts, origin=O, max_ray_cells=1 << 22)
    assert r["n_dropped"] == want_dropped and r["n_rays"] == len(pts) - want_dropped
    for bad in ((np.nan, 0, 0), (0, 2.0 ** 22, 0), (0, 0, -(2.0 ** 20) * K.LEAF)):
        before = planes(m)
        with pytest.raises(ValueError):
            m.carve(A[None], origin=bad)
        assert all(np.array_equal(x, y) for x, y in zip(planes(m), before))
    # the origin moves as a point does
    R, t = vmap_cases.transform(1)
    o = np.array([0.3, -0.2, 0.1])
    a, b = VC.CarveOracleMap(K.LEAF), VC.CarveOracleMap(K.LEAF)
    cloud = vmap_cases.cloud(300, 5, spread=3.0)
    for mm in (a, b):
        mm.integrate(cloud, R, t)
        mm.integrate(K.box_points((-3, -3, -1), (3, 3, 1)))           # a block of voxels around the moved origin to cross
    p = cloud.astype(np.float64)
    moved = np.stack([((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k] for k in range(3)], axis=1).astype(K.F)
    om = np.array([((R[k, 0] * o[0] + R[k, 1] * o[1]) + R[k, 2] * o[2]) + t[k] for k in range(3)]).astype(K.F)
    ra, rb = a.carve(cloud, R, t, origin=o), b.carve(moved, origin=om)
    assert ra == rb and ra["n_missed"] > 0 and all(np.array_equal(x, y) for x, y in zip(planes(a), planes(b)))


# ------------------------------------------------------------------ the carved extraction
def test_carved_extraction():
    m = line_map()
    KEY6 = V.key_of(6, 0, 0)                                        # crossed by B alone
    m.carve(A[None], origin=O), m.carve(B[None], origin=O)          # (4, 0, 0): seen 1, miss 1; (6, 0, 0): seen 0, miss 1
    keys = lambda mm: set(m.extract(max_miss=mm)[2].tolist())
    assert at(m, KEY4) == (1, 1) and at(m, KEY6) == (0, 1) and at(m, KEY2) == (0, 2)
    assert KEY4 in keys((1, 1)) and KEY4 not in keys((1, 2))        # equality at the ratio is kept
    assert KEY6 in keys((1, 1)) and KEY6 not in keys((1, 2))        # seen = 0 counts as 1
    assert KEY2 not in keys((1, 1)) and KEY2 in keys((2, 1))
    m.carve(B[None], origin=O)                                      # (6, 0, 0): seen 0, miss 2; (4, 0, 0): seen 1, miss 2
    assert KEY6 not in keys((1, 1)) and KEY6 in keys((2, 1)) and KEY4 not in keys((1, 1)) and KEY4 in keys((2, 1))
    assert len(keys((0, 1))) == int((m.read_carve()[1] == 0).sum()) > 0
    # the uncarved extraction ignores the planes
    assert len(m.extract()[2]) == m.n_voxels
    # min_count and the box together with the ratio, against numpy on the accumulators
    m.integrate(K.centre((2, 0, 0))[None]), m.integrate(K.centre((9, 1, 0))[None])
    xyz4, count, key, sums = m.extract()
    seen, miss, _ = m.read_carve()
    lo, hi = (K.F(0.3), K.F(-1.0)), (K.F(2.4), K.F(0.2))
    for mc, mm in ((0, (1, 1)), (2, (2, 1)), (2, (1, 1)), (1, (1, 3))):
        keep = (count >= mc) & (miss.astype(np.uint64) * np.uint64(mm[1]) <= np.maximum(seen, 1).astype(np.uint64) * np.uint64(mm[0]))
        keep &= (xyz4[:, 0] >= lo[0]) & (xyz4[:, 0] <= hi[0]) & (xyz4[:, 1] >= lo[1]) & (xyz4[:, 1] <= hi[1])
        got = m.extract(lo, hi, mc, mm)
        assert K_same(got, tuple(a[keep] for a in (xyz4, count, key, sums)))
    assert len(m.extract(lo, hi, 2, (3, 1))[2]) == 1                # (2, 0, 0) alone: two points, miss 3, inside the box


# ------------------------------------------------------------------ the binding
def test_structs_mirror_the_header():
    lp, lr = VC.layout()
    for S, L in ((api.VmapCarveParams, lp), (api.VmapCarveResult, lr), (VC.CarveParams, lp), (VC.CarveResult, lr)):
        assert C.sizeof(S) == L[0]
        assert [getattr(S, f).offset for f, _ in S._fields_] == L[1:]
    assert [f for f, _ in api.VmapCarveResult._fields_] == list(VC.COUNTERS)
    d = api.vmap_default_carve_params()
    assert (d.end_margin, d.tail_num, d.tail_den, d.max_ray_cells) == (1, 1, 8, 512)
    o = VC.params()
    assert (o.end_margin, o.tail_num, o.tail_den, o.max_ray_cells) == (1, 1, 8, 512)


def new_entry_points(h, pts, bad=None):
    """the return code of each new entry point on handle h with well-formed arguments (`bad`: one broken argument)"""
    L = api.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n, res = C.c_int(-5), api.VmapCarveResult()
    cp = api.vmap_default_carve_params(**(bad or {}))
    out = np.zeros(64, np.uint64)
    return dict(
        carve=L.slam_vmap_carve(h, p(pts), len(pts), 3, None, None, None, C.byref(cp), C.byref(res)),
        carve_dev=L.slam_vmap_carve_dev(h, p(pts), len(pts), 3, None, None, None, C.byref(cp), C.byref(res), None),
        extract_carved_dev=L.slam_vmap_extract_carved_dev(h, None, None, 0, 1, 1, p(out), None, None, 4, C.byref(n), None),
        read_carved=L.slam_vmap_read_carved(h, None, None, 0, 1, 1, p(out), None, None, 4, C.byref(n)),
        read_carve=L.slam_vmap_read_carve(h, p(out), p(out), p(out), 4, C.byref(n)))


def test_entry_points_without_a_device_and_argument_errors():
    """Well-formed arguments: SLAM_E_NO_DEVICE on a machine without a device (no handle can exist there); with a device a NULL
    map is SLAM_E_INVALID.  Broken arguments are SLAM_E_INVALID on both, before the device is asked for."""
    L = api.lib()
    pts = np.zeros((4, 3), np.float32)
    want = api.E_NO_DEVICE if api.device_count() == 0 else api.E_INVALID
    assert new_entry_points(None, pts) == dict.fromkeys(("carve", "carve_dev", "extract_carved_dev", "read_carved", "read_carve"), want)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n, R = C.c_int(-5), np.eye(3).reshape(9)
    for bad in (dict(tail_den=0), dict(tail_den=-1), dict(end_margin=-1), dict(tail_num=-1), dict(max_ray_cells=0)):
        rc = new_entry_points(None, pts, bad)
        assert rc["carve"] == rc["carve_dev"] == api.E_INVALID, bad
    assert L.slam_vmap_carve(None, p(pts), 4, 2, None, None, None, None, None) == api.E_INVALID                  # stride < 3
    assert b"slam_vmap_carve" in L.slam_last_error()
    assert L.slam_vmap_carve_dev(None, p(pts), 4, 3, p(R), None, None, None, None, None) == api.E_INVALID        # R without t
    assert L.slam_vmap_carve_dev(None, p(pts), -1, 3, None, None, None, None, None, None) == api.E_INVALID
    assert L.slam_vmap_read_carved(None, None, None, 0, 1, 0, None, None, None, 0, C.byref(n)) == api.E_INVALID  # den <= 0
    assert L.slam_vmap_extract_carved_dev(None, None, None, 0, 1, -2, None, None, None, 0, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_extract_carved_dev(None, None, None, 0, -1, 1, None, None, None, 0, C.byref(n), None) == api.E_INVALID
    assert L.slam_vmap_read_carve(None, None, None, None, -1, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_carve(None, None, None, None, 0, None) == api.E_INVALID
    assert n.value == -5


# ------------------------------------------------------------------ the mover scene
# Recorded on the CPU when the test was written (leaf 0.30, the defaults: end_margin 1, tail 1 / 8, max_ray_cells 512; eight
# scans of 16 rings x 512 of tests/vmap_carve_cases.py's mover scene at the truth transforms, integrate scan k then carve
# scan k; removal rule miss > seen, i.e. the carved extraction at 1 / 1):
#   10 460 voxels, 184 of them ghosts; static voxels removed 2 of 10 276 (0.019 %); ghost voxels removed 144 of 184 (78.3 %)
RECORDED_STATIC_REMOVED, RECORDED_GHOST_SHARE = 2, 0.783
STATIC_BOUND = max(10, 3 * RECORDED_STATIC_REMOVED)         # voxels
GHOST_BOUND = RECORDED_GHOST_SHARE - 0.10                   # share: ten points below the recorded one


def carve_scene(mutation=VC.MUT_NONE, **kw):
    scene = K.mover_scene()
    m = VC.CarveOracleMap(0.30, mutation)
    for c, pose, T in scene:
        m.integrate(c, T[:3, :3], T[:3, 3])
        m.carve(c, T[:3, :3], T[:3, 3], **kw)
    return m, scene


def removal(m, scene):
    """(voxels, ghosts, static voxels removed, ghost voxels removed) at the default ratio"""
    allv, kept = m.extract(), m.extract(max_miss=(1, 1))
    ghost = K.ghost_mask(allv[0], scene[0][1])
    removed = ~np.isin(allv[2], kept[2])
    return len(ghost), int(ghost.sum()), int((removed & ~ghost).sum()), int((removed & ghost).sum())


def test_scene_static_voxels_stay_and_ghosts_go():
    m, scene = carve_scene()
    n, ghosts, static_removed, ghosts_removed = removal(m, scene)
    print("mover scene: %d voxels, %d ghosts; static removed %d (%.3f %%), ghosts removed %d (%.1f %%)" %
          (n, ghosts, static_removed, 100.0 * static_removed / (n - ghosts), ghosts_removed, 100.0 * ghosts_removed / ghosts))
    assert ghosts > 100
    # these bounds guard the inputs (a changed scene), not the device
    assert static_removed <= STATIC_BOUND
    assert ghosts_removed / ghosts >= GHOST_BOUND


def test_scene_without_the_tail_eats_the_ground():
    """why the tail is proportional: with end_margin 1 alone the rays that end on the ground charge the ground's own voxel
    layer on their way in, and static voxels go by the hundred"""
    m, scene = carve_scene(tail_num=0)
    n, ghosts, static_removed, ghosts_removed = removal(m, scene)
    print("mover scene without the tail: static removed %d of %d, ghosts removed %d of %d" % (static_removed, n - ghosts, ghosts_removed, ghosts))
    assert static_removed > 10 * STATIC_BOUND


def test_builder_with_carve_on_the_scene():
    scene = K.mover_scene()
    b, plain = VC.OracleCarveBuilder(carve=True), VC.OracleCarveBuilder(carve=False)
    assert plain.max_miss() is None
    for k, (c, pose, T) in enumerate(scene):
        ok, r = b.add_cloud(c)
        ok2, _ = plain.add_cloud(c)
        assert ok and ok2, k
        if k:
            err = V.pose_error(r["transform"], T)
            print("step %d: iterations %d state %d fitness %.4f error %.2f mm %.3f mrad; carve %s" %
                  (k, r["iterations"], r["state"], r["fitness"], err[0] * 1e3, err[1] * 1e3, b.last_carve))
    carved, whole = b.map(), plain.map()
    g_carved = int(K.ghost_mask(carved, scene[0][1]).sum())
    g_whole = int(K.ghost_mask(whole, scene[0][1]).sum())
    print("builder on the mover scene: %d voxels, %d ghosts uncarved; %d voxels, %d ghosts carved" % (len(whole), g_whole, len(carved), g_carved))
    assert g_whole > 100 and g_carved <= g_whole - GHOST_BOUND * g_whole
