"""slam_vmap_search* on the device against tests/vmap_search_cases.py (docs/VOXEL_MAP.md section 13): the volume, the hits and
n_with_cell bit for bit over the sizes, windows and rotation counts at which the kernels take another path; the maps and sources
at the edges; the three forms; what a search leaves alone; and MapLocalizer.search / relocalize on the scene of section 11.4."""
import signal

import numpy as np
import pytest

import map_localizer_cases as ML
import vmap_gicp_oracle as VG
import vmap_oracle as V
import vmap_search_cases as SC
from slam_amd import api
from test_gpu_vmap_gicp import device_filter

pytestmark = pytest.mark.gpu
TEST_SECONDS = 120
POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_map_localizer.py
SIZES = (0, 1, 63, 64, 65, 257)
WINDOWS = ((0, 0, 0), (1, 1, 0), (3, 2, 1))
YAWS = (1, 4, 64)
LEAF = 0.5


@pytest.fixture(autouse=True)
def time_limit():
    """Every test here ends after TEST_SECONDS, and the session with it: nothing more is started on the GPU."""
    def expired(signum, frame):
        pytest.exit("GPU test exceeded %d s" % TEST_SECONDS, returncode=3)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def cloud(n, seed, half=(8.0, 8.0, 1.5)):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 3)) * 2 - 1) * np.array(half)).astype(np.float32)


def check(dm, qual, leaf, xyz, p, form="host", dense=True, **how):
    """one device call against the restatement: the volume, the hits and n_with_cell, bit for bit"""
    want_hits, want_vol, _ = SC.search(xyz, qual, leaf, p, dense=dense)
    cp = SC.ctypes_params(p)
    if form == "host":
        hits, vol = dm.search(xyz, params=cp, volume=True)
    elif form == "dev":
        a = np.ascontiguousarray(xyz, np.float32)
        d = api.DeviceArray.from_host(a) if len(a) else None
        hits, vol = dm.search(d_xyz=d.ptr if d else 0, n=len(a), stride=a.shape[1] if a.ndim > 1 else 3, params=cp, volume=True, **how)
    assert vol.dtype == np.int32 and vol.shape == want_vol.shape and np.array_equal(vol, want_vol), (p, len(xyz))
    assert SC.same_hits(hits, want_hits), (p, len(xyz), hits, want_hits)
    return hits, vol


@pytest.fixture(scope="module")
def base():
    """a count map at leaf 0.5 around zero (3 000 points, about 2 000 voxels), its restatement, and the source cloud the sizes are
    cut from: the same box, so that scores are not zero"""
    pts = cloud(3000, 1)
    dm, om = api.VoxelMap(leaf=LEAF), V.OracleMap(LEAF)
    assert dm.integrate(pts) == om.integrate(pts) == 0
    qual = {c: SC.qualifying(om, False, c) for c in (1, 2)}
    assert len(qual[1]) > 1500 and 100 < len(qual[2]) < len(qual[1])
    yield dict(dm=dm, om=om, qual=qual, src=cloud(257, 2))
    dm.close()


@pytest.mark.parametrize("n_yaw", YAWS)
@pytest.mark.parametrize("window", WINDOWS)
def test_sizes_windows_and_rotation_counts(base, window, n_yaw):
    p = SC.params(n_yaw=n_yaw, yaw0=0.1, cx=0.3, cy=-0.2, cz=0.1, wx=window[0], wy=window[1], wz=window[2], planes_only=0, min_count=1)
    for n in SIZES:
        hits, vol = check(base["dm"], base["qual"][1], LEAF, base["src"][:n], p)
        assert (len(hits) > 0) == (n > 0)                                     # a guard of the inputs: the sources score


@pytest.mark.parametrize("wx", (31, 32))
def test_a_row_one_lane_short_of_a_wavefront_and_one_past_it(base, wx):
    """63 and 65 poses a row; wy = 9 makes 19 rows: five tiles of four, the last one partly idle"""
    p = SC.params(n_yaw=4, wx=wx, wy=9, wz=0, planes_only=0, min_count=2, top_m=6)
    hits, vol = check(base["dm"], base["qual"][2], LEAF, base["src"], p)
    assert vol.shape == (4, 1, 19, 2 * wx + 1) and len(hits) == 6
    check(base["dm"], base["qual"][2], LEAF, base["src"][:65], SC.params(n_yaw=1, wx=wx, wy=0, wz=2, planes_only=0, min_count=2))


def test_more_points_than_one_stage_of_lds(base):
    """8 192 bit indices are staged at a time: 8 193 points take a second pass of one"""
    src = cloud(8193, 3)
    hits, vol = check(base["dm"], base["qual"][1], LEAF, src, SC.params(n_yaw=2, wx=2, wy=2, wz=0, planes_only=0, min_count=1))
    assert int(vol.max()) > 1000


def test_cells_straddle_zero_and_points_without_a_cell(base):
    src = np.concatenate([base["src"][:100], SC.NO_CELL, np.array([(3e6, 3e6, 0), (-np.inf, 0, 0)], np.float32)])
    p = SC.params(n_yaw=4, wx=2, wy=2, wz=1, planes_only=0, min_count=1)
    cells, has = SC.moved_cells(src, SC.rotation(p, 1), LEAF)
    assert cells[has].min() < 0 < cells[has].max() and int(has.sum()) == 101
    hits, _ = check(base["dm"], base["qual"][1], LEAF, src, p, dense=False)
    assert [h["n_with_cell"] for h in hits] == [101] * len(hits) and len(hits) > 0
    # nothing but points without a cell: a zero volume, no hits
    hits, vol = check(base["dm"], base["qual"][1], LEAF, SC.NO_CELL[1:], p)
    assert hits == [] and not vol.any()


def test_a_map_of_no_voxels_and_top_m(base):
    empty = api.VoxelMap(leaf=LEAF)
    hits, vol = check(empty, set(), LEAF, base["src"], SC.params(n_yaw=4, wx=1, wy=1, planes_only=0))
    assert hits == [] and not vol.any()
    empty.close()
    dm = api.VoxelMap(leaf=1.0)
    dm.integrate(SC.cell_centres(SC.HAND_VOXELS))
    for top_m, n in ((0, 0), (1, 1), (8, 8), (64, 15)):                       # 15 poses of the hand-worked case score at all
        hits, _ = check(dm, SC.HAND_VOXELS, 1.0, SC.HAND_POINTS, dict(SC.HAND_PARAMS, top_m=top_m, planes_only=0, min_count=1), dense=False)
        assert len(hits) == n
    dm.close()


def test_ties_and_the_suppression_that_wraps(base):
    cells = SC.four_fold()
    dm = api.VoxelMap(leaf=1.0)
    dm.integrate(SC.cell_centres(cells))
    src = SC.cell_centres(cells)
    hits, _ = check(dm, cells, 1.0, src, SC.params(n_yaw=4, wx=1, wy=1, wz=0, top_m=4, nms_yaw=0, nms_cells=0, planes_only=0, min_count=1), dense=False)
    assert [(h["score"], h["k"]) for h in hits] == [(12, k) for k in range(4)]
    hits, _ = check(dm, cells, 1.0, src, SC.params(n_yaw=8, wx=1, wy=1, wz=0, top_m=8, nms_yaw=2, nms_cells=2, planes_only=0, min_count=1), dense=False)
    assert [(h["score"], h["k"]) for h in hits] == [(12, 0), (12, 4)]
    dm.close()


def test_a_table_grown_through_rehashes(base):
    pts = cloud(3000, 1)
    dm = api.VoxelMap(leaf=LEAF, initial_capacity=64)
    for part in np.array_split(pts, 5):
        dm.integrate(part)
    assert dm.info()["capacity"] >= 4096 > 64
    check(dm, base["qual"][1], LEAF, base["src"], SC.params(n_yaw=4, wx=3, wy=2, wz=1, planes_only=0, min_count=1))
    check(dm, base["qual"][2], LEAF, base["src"], SC.params(n_yaw=4, wx=3, wy=2, wz=1, planes_only=0, min_count=2))
    dm.close()


@pytest.fixture(scope="module")
def planes():
    """a 1 m map with distributions of the scene's first cloud, carved by the second; the source is part of the first"""
    (c0, _), (c1, _) = V.builder_clouds([0, 1])
    yield dict(c0=c0, c1=c1, src=np.ascontiguousarray(c0[::16]))


def test_planes_only_with_stale_distributions_and_the_carved_rule(planes):
    p = SC.params(n_yaw=8, wx=3, wy=3, wz=0)
    dm, om = api.VoxelMap(leaf=1.0), VG.OracleDistMap(1.0)
    dm.enable_distributions()
    assert dm.integrate(planes["c0"]) == om.integrate(planes["c0"]) == 0
    qual = SC.qualifying(om, True)                                            # the distributions were never computed on the device: stale
    assert 50 < len(qual) < om.n_voxels
    hits, _ = check(dm, qual, 1.0, planes["src"], p)
    assert hits[0]["k"] == 0 and (hits[0]["dx"], hits[0]["dy"]) == (0, 0)
    dm.integrate(planes["c1"])                                                # stale again
    om.integrate(planes["c1"])
    check(dm, SC.qualifying(om, True), 1.0, planes["src"], p)
    dm.close()
    # the carved rule as part of the plane rule
    dm, om = api.VoxelMap(leaf=1.0), VG.OracleDistMap(1.0, max_miss_num=1, max_miss_den=2)
    dm.enable_distributions(max_miss_num=1, max_miss_den=2)
    dm.integrate(planes["c0"])
    om.integrate(planes["c0"])
    before = SC.qualifying(om, True)
    for _ in range(3):
        dm.carve(planes["c1"], origin=(0.0, 0.0, 2.0))
    om.set_carve(*dm.read_carve())
    qual = SC.qualifying(om, True)
    assert len(qual) < len(before)                                            # a guard of the inputs: the rule removed plane voxels
    check(dm, qual, 1.0, planes["src"], p)
    dm.close()


def test_planes_only_is_refused_without_distributions_and_counts_are_not(base):
    with pytest.raises(api.SlamError) as e:
        base["dm"].search(base["src"], planes_only=1)
    assert e.value.code == api.E_INVALID
    store = api.KeyframeStore(leaf_size=0.30, gate=2.0)
    for kid in (-1, 0, 5):
        with pytest.raises(api.SlamError) as e:
            base["dm"].search(store=store, kid=kid, planes_only=0)
        assert e.value.code == api.E_INVALID
    kid = store.add_keyframe(base["src"])
    store.remove_keyframe(kid)
    with pytest.raises(api.SlamError) as e:
        base["dm"].search(store=store, kid=kid, planes_only=0)                # a dead keyframe
    assert e.value.code == api.E_INVALID
    store.close()


def test_the_three_forms_a_stream_and_what_a_search_leaves_alone(planes):
    dm = api.VoxelMap(leaf=1.0)
    dm.enable_distributions()
    dm.integrate(planes["c0"])
    dm.compute_distributions()
    sums, moments = dm.read_sums(), dm.read_moments()
    store = api.KeyframeStore(leaf_size=0.30, gate=2.0)
    kid = store.add_keyframe(planes["c1"])
    src = store.read_keyframe(kid)                                            # [n, 4]: the filtered cloud as the store holds it
    n = len(src)
    assert n > 1000
    p = api.vmap_default_search_params(n_yaw=16, wx=5, wy=5, wz=1, cx=0.5, cy=0.25)
    d = api.DeviceArray.from_host(np.ascontiguousarray(src, np.float32))
    st = api.Stream()
    forms = [dm.search(d_xyz=d.ptr, n=n, stride=4, params=p, volume=True),
             dm.search(d_xyz=d.ptr, n=n, stride=4, params=p, volume=True, stream=st),
             dm.search(src, params=p, volume=True),
             dm.search(np.ascontiguousarray(src[:, :3]), params=p, volume=True),
             dm.search(store=store, kid=kid, params=p, volume=True),
             dm.search(store=store, kid=kid, params=p, volume=True, stream=st)]
    assert len(forms[0][0]) == 4 and forms[0][0][0]["n_with_cell"] == n
    for hits, vol in forms[1:]:
        assert SC.same_hits(hits, forms[0][0]) and np.array_equal(vol, forms[0][1])
    assert dm.search(store=store, kid=kid, params=p)[1] is None               # the volume stays on the device unless asked for
    for a, b in zip(sums + moments, dm.read_sums() + dm.read_moments()):
        assert VG.same_bits(a, b)
    store.close()
    dm.close()


def test_a_brick_too_large_is_refused_and_the_handle_stays_usable(base):
    """two points 4 km apart in x and y at leaf 0.05: 80 000 x 80 000 cells are more than 2^31 bits"""
    dm = api.VoxelMap(leaf=0.05)
    dm.integrate(base["src"])
    far = np.array([(-2000, -2000, 0), (2000, 2000, 0)], np.float32)
    before = dm.read_sums()
    with pytest.raises(api.SlamError) as e:
        dm.search(far, n_yaw=1, wx=1, wy=1, planes_only=0)
    assert e.value.code == api.E_NOMEM
    for a, b in zip(before, dm.read_sums()):
        assert VG.same_bits(a, b)
    om = V.OracleMap(0.05)
    om.integrate(base["src"])
    check(dm, SC.qualifying(om, False, 1), 0.05, base["src"], SC.params(n_yaw=2, wx=2, wy=2, planes_only=0, min_count=1))
    dm.close()


def test_create_search_destroy_cycles_keep_device_memory_flat(base):
    """As tests/test_gpu_vmap_coarsen.py sizes and checks it: 40 cycles may cost at most what one cycle's handle holds alive."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    pts = cloud(3000, 1)

    def cycle(alive=None):
        m = api.VoxelMap(leaf=LEAF, initial_capacity=1 << 20)
        m.integrate(pts)
        hits, _ = m.search(base["src"], n_yaw=16, wx=8, wy=8, planes_only=0, min_count=1)
        if alive is not None:
            alive.append(free_bytes(rt))
        m.close()
        return [(h["score"], h["k"], h["dx"], h["dy"]) for h in hits]

    first = cycle()
    assert len(first) == 4
    for _ in range(2):
        cycle()
    free_after_warmup = free_bytes(rt)
    alive = []
    assert cycle(alive) == first
    size = free_after_warmup - alive[0]
    for _ in range(40):
        assert cycle() == first
    free_after = free_bytes(rt)
    print("vmap search lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (size, free_after_warmup - free_after))
    assert size > 0 and free_after >= free_after_warmup - size


# ------------------------------------------------------------------ MapLocalizer.search and relocalize on the scene
@pytest.fixture(scope="module")
def world():
    parts, scan, truth = ML.scene()
    fine = api.VoxelMap(leaf=ML.LEAF)
    fine.enable_distributions()
    for c, T in parts:
        assert fine.integrate(c, T[:3, :3], T[:3, 3]) == 0
    loc = api.MapLocalizer(levels=2)
    loc.set_map(fine)
    ora = ML.OracleLocalizer(parts, 2, filter=device_filter(ML.STORE_LEAF, 2.0))
    cx, cy, w = SC.map_window(ora.levels[1], 2.0)
    out = loc.relocalize(scan, cx, cy, 0.0, 2.0 * w)
    yield dict(scan=scan, truth=truth, fine=fine, loc=loc, ora=ora, window=(cx, cy, w), out=out)
    loc.close()
    fine.close()


@pytest.mark.parametrize("level", (0, 1))
def test_map_localizer_search_on_the_scene(world, level):
    """no prior: 64 yaws and a window over the whole map; the hits are the restatement's, hit 0 in the truth's neighbourhood"""
    ora, loc = world["ora"], world["loc"]
    m = ora.levels[level]
    cx, cy, w = SC.map_window(m, m.leaf)
    p = SC.params(cx=cx, cy=cy, wx=w, wy=w)
    hits = loc.search(world["scan"], params=SC.ctypes_params(p), level=level)
    assert ora.set_scan(world["scan"]) == hits[0]["n_with_cell"]
    want = SC.search(ora.src.xyz, SC.qualifying(m, True), m.leaf, p, dense=True)[0]
    assert SC.same_hits(hits, want)
    d, a = SC.hit_offset(hits[0], world["truth"])
    print("leaf %g: hit 0 scores %d of %d, %.3f m %.4f rad from the truth" % (m.leaf, hits[0]["score"], hits[0]["n_with_cell"], d, a))
    assert d <= m.leaf and a <= 2 * np.pi / 64


def test_relocalize_finds_the_truth_from_no_prior(world):
    """By section 11.4's rule: the hits are the restatement's bits; per (start, level) the restatement registers from the device's
    own f32 init; the winner is the restatement's and lies within twice the recorded distance of the truth."""
    out, ora, (cx, cy, w) = world["out"], world["ora"], world["window"]
    assert out["found"] and len(out["hits"]) == 4 and out["n_source"] == ora.set_scan(world["scan"])
    own = SC.relocalize(ora, world["scan"], cx, cy, 0.0, 2.0 * w, api.MapLocalizer.MAX_SCORE)
    assert SC.same_hits(out["hits"], own["hits"])
    inits = [[None] * 4 for _ in range(2)]
    for i, h in enumerate(out["hits"]):
        init = h["init"]
        for k in (1, 0):
            if out["last"][k][i] is None:
                break
            inits[k][i] = init
            init = out["last"][k][i]["transform"]
    want = SC.relocalize(ora, world["scan"], cx, cy, 0.0, 2.0 * w, api.MapLocalizer.MAX_SCORE, hits=out["hits"], inits=inits)
    for k in (1, 0):
        for i in range(4):
            r, ro = out["last"][k][i], want["last"][k][i]
            assert (r is None) == (ro is None), (k, i)
            if r is None:
                continue
            dp, da = V.pose_error(r["transform64"], ro["transform64"])
            assert dp <= POS_TOL and da <= ANG_TOL and (r["state"] in ML.OUT) == (ro["state"] in ML.OUT), (k, i)
    assert out["index"] == ML.pick(out["last"][0], out["n_source"], api.MapLocalizer.MAX_SCORE)
    e = V.pose_error(out["transform"], world["truth"])
    print("relocalize: hit %d wins (restatement %d), %.3f mm %.4f mrad from the truth" % (out["index"], own["index"], e[0] * 1e3, e[1] * 1e3))
    assert e[0] * 1e3 <= 2 * ML.RECORDED_MM and e[1] * 1e3 <= 2 * ML.RECORDED_MRAD


def test_relocalize_twice_gives_the_same_bits_and_localize_is_the_call_it_was(world):
    from test_gpu_map_localizer import answer_bits
    loc, (cx, cy, w) = world["loc"], world["window"]

    def all_bits(o):
        return answer_bits({k: v for k, v in o.items() if k != "hits"}), [(h["score"], h["k"], h["dx"], h["dy"], h["dz"], h["init"].tobytes()) for h in o["hits"]]
    assert all_bits(loc.relocalize(world["scan"], cx, cy, 0.0, 2.0 * w)) == all_bits(world["out"])
    starts = [h["init"] for h in world["out"]["hits"]]
    assert answer_bits(loc.localize(world["scan"], starts)) == answer_bits(loc.localize(world["scan"], starts, from_level=1))   # two levels: the default
    for kid in range(len(loc.store)):
        with pytest.raises(api.SlamError):
            loc.store.info(kid)                                               # no keyframe stays
    # a window that sees nothing: not found
    none = loc.relocalize(world["scan"], 5000.0, 5000.0, 0.0, 4.0)
    assert not none["found"] and none["hits"] == [] and none["index"] == -1
