"""slam_vmap_coarsen on the device (slam_amd/csrc/voxmap.hip, docs/VOXEL_MAP.md section 11) against the Python restatement
tests/vmap_coarsen_cases.py and against device maps integrated directly at the coarser leaf.  Every comparison is bit for bit,
through read_sums / read_moments / read_carve / read_distributions."""
import signal

import numpy as np
import pytest

import vmap_coarsen_cases as CC
import vmap_oracle as V
from slam_amd import api

pytestmark = pytest.mark.gpu
TEST_SECONDS = 300
GICP = dict(gate=4.0, max_iterations=100, transformation_epsilon=1e-6)


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


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def new_map(leaf, moments=True, **kw):
    m = api.VoxelMap(leaf=leaf, **kw)
    if moments:
        m.enable_distributions()
    return m


def built(leaf, clouds, moments=True, carve=False, **kw):
    m = new_map(leaf, moments, **kw)
    for c in clouds:
        pts, (R, t) = c if isinstance(c, tuple) else (c, (None, None))
        assert m.integrate(pts, R, t) == 0
        if carve:
            m.carve(pts, R, t)
    return m


def records_of(m):
    """the map's records through the key-ordered readers, under CoarseMap.records()'s names"""
    sums, count, key = m.read_sums()
    seen, miss, key2 = m.read_carve()
    out = dict(key=key, count=count, sums=sums, seen=seen, miss=miss)
    assert bits(key) == bits(key2)
    if m.layout()["distributions"]:
        out["E"], out["M"], key3 = m.read_moments()
        assert bits(key) == bits(key3)
    return out


def everything(m):
    """every reader of a map as bytes: what two equal maps must agree on"""
    out = {f: bits(a) for f, a in records_of(m).items()}
    out["read"] = [bits(a) for a in m.read()]
    i, lay = m.info(), m.layout()
    out["info"] = (i["n_voxels"], i["n_points"], lay["leaf"], lay["carved"], lay["distributions"])
    if lay["distributions"]:
        d = m.read_distributions()
        out["dist"] = {f: bits(d[f]) for f in d}
    return out


def check(m, ref):
    """the device map against the restatement: every record plane and the counters"""
    got, want = records_of(m), ref.records()
    for f in got:
        assert got[f].dtype == want[f].dtype and bits(got[f]) == bits(want[f]), f
    i = m.info()
    assert (i["n_voxels"], i["n_points"]) == (ref.n_voxels, ref.n_points)


# ------------------------------------------------------------------ sizes, shifts, an empty and a filled destination
@pytest.mark.parametrize("n", CC.SIZES)
@pytest.mark.parametrize("start", ("empty", "filled"))
@pytest.mark.parametrize("moments", (False, True))
def test_source_sizes(n, start, moments):
    src = built(0.25, [CC.chain(n)] if n else [], moments)
    assert src.info()["n_voxels"] == n
    dst, ref = new_map(0.5, moments), CC.CoarseMap(0.5, moments)
    if start == "filled":
        first = built(0.25, [CC.FOUR_CLOUDS[0]], moments)
        dst.coarsen(first)
        ref.coarsen(0.25, records_of(first))
        first.close()
    before = everything(src)
    dst.coarsen(src)
    ref.coarsen(0.25, records_of(src))
    check(dst, ref)
    assert everything(src) == before                                          # the source is unchanged
    if start == "empty":
        direct = built(0.5, [CC.chain(n)] if n else [], moments)
        assert everything(dst) == everything(direct)
        assert n // 2 <= dst.info()["n_voxels"] <= n // 2 + 1                   # the chain fills its parents two by two
        direct.close()
    src.close()
    dst.close()


@pytest.mark.parametrize("j", (1, 2, 3))
@pytest.mark.parametrize("moments", (False, True))
def test_shifts_against_maps_integrated_directly(j, moments):
    clouds = list(CC.FOUR_CLOUDS) + [CC.around_zero(0.25), CC.parent_corner(0.25)]
    coarse = 0.25 * 2 ** j
    src, dst, direct = built(0.25, clouds, moments), new_map(coarse, moments), built(coarse, clouds, moments)
    dst.coarsen(src)
    assert everything(dst) == everything(direct)
    ref = CC.CoarseMap(coarse, moments)
    ref.coarsen(0.25, records_of(src))
    check(dst, ref)
    parents = {CC.cells_of(k)[0] for k in dst.read_sums()[2]}
    assert -1 in parents and 0 in parents                                     # the cells on both sides of zero
    # shifting by j equals shifting by 1 j times
    level = src
    steps = []
    for s in range(1, j + 1):
        nxt = new_map(0.25 * 2 ** s, moments)
        nxt.coarsen(level)
        steps.append(nxt)
        level = nxt
    assert everything(level) == everything(direct)
    for m in [src, dst, direct] + steps:
        m.close()


def test_hand_worked_parent_with_eight_children():
    pts, cells, parent, E, M = CC.eight_children(1.0)
    src, dst = built(1.0, [pts]), new_map(2.0)
    dst.coarsen(src)
    r = records_of(dst)
    assert [int(k) for k in r["key"]] == [parent] and list(r["count"]) == [8]
    assert r["E"].tolist() == [E] and r["M"].tolist() == [M]
    direct = built(2.0, [pts])
    assert everything(dst) == everything(direct)
    for m in (src, dst, direct):
        m.close()


def test_leaf_0375_and_leaf_030():
    src, dst, direct = built(0.375, CC.FOUR_CLOUDS), new_map(1.5), built(1.5, CC.FOUR_CLOUDS)
    dst.coarsen(src)
    assert everything(dst) == everything(direct)
    fine, coarse = CC.PLAIN_ONLY
    psrc, pdst, pdirect = built(fine, CC.FOUR_CLOUDS, False), new_map(coarse, False), built(coarse, CC.FOUR_CLOUDS, False)
    pdst.coarsen(psrc)
    assert everything(pdst) == everything(pdirect)
    for m in (src, dst, direct, psrc, pdst, pdirect):
        m.close()


# ------------------------------------------------------------------ growth, partitions, a stream
@pytest.mark.parametrize("moments", (False, True))
def test_a_destination_of_64_slots_grows_through_rehashes(moments):
    dst, ref = new_map(0.5, moments, initial_capacity=64), CC.CoarseMap(0.5, moments)
    caps = [dst.info()["capacity"]]
    for k in range(4):
        pts, (R, t) = CC.FOUR_CLOUDS[k]
        for o in range(0, len(pts), 150):
            src = built(0.25, [(pts[o:o + 150], (R, t))], moments)
            dst.coarsen(src)
            ref.coarsen(0.25, records_of(src))
            src.close()
            caps.append(dst.info()["capacity"])
        check(dst, ref)
    assert caps[0] == 64 and len(set(caps)) >= 4, caps                          # at least three rehashes
    direct = built(0.5, CC.FOUR_CLOUDS, moments)
    assert everything(dst) == everything(direct)
    dst.close()
    direct.close()


@pytest.mark.parametrize("order", CC.ORDERS)
def test_fine_maps_of_a_partition_into_one_coarse_map(order):
    direct = built(1.0, CC.FOUR_CLOUDS)
    dst = new_map(1.0)
    halves = [built(0.25, [CC.FOUR_CLOUDS[k] for k in order[:2]]), built(0.25, [CC.FOUR_CLOUDS[k] for k in order[2:]])]
    for h in halves:
        dst.coarsen(h)
    assert everything(dst) == everything(direct)
    for m in halves + [dst, direct]:
        m.close()


def test_on_a_stream():
    st = api.Stream()
    src, dst, direct = built(0.25, CC.FOUR_CLOUDS), new_map(1.0), built(1.0, CC.FOUR_CLOUDS)
    dst.coarsen(src, stream=st)
    dst.compute_distributions(stream=st)
    st.synchronize()
    assert everything(dst) == everything(direct)
    for m in (src, dst, direct):
        m.close()


# ------------------------------------------------------------------ carve planes are not derived
def test_a_carved_source_and_a_carved_destination():
    src = built(0.25, CC.FOUR_CLOUDS[:2], carve=True)
    assert src.layout()["carved"] and int(src.read_carve()[0].sum()) > 0
    dst = new_map(0.5)
    dst.coarsen(src)
    assert not dst.layout()["carved"] and not dst.read_carve()[0].any()       # nothing is derived from the source's planes
    direct = built(0.5, CC.FOUR_CLOUDS[:2])
    assert everything(dst) == everything(direct)
    # a carved destination: its planes are what they were, the new voxels' are zero
    cdst = built(0.5, CC.FOUR_CLOUDS[2:3], carve=True)
    seen0, miss0, key0 = cdst.read_carve()
    assert int(seen0.sum()) > 0
    cdst.coarsen(src)
    seen1, miss1, key1 = cdst.read_carve()
    old = np.isin(key1, key0)
    assert bits(key1[old]) == bits(key0) and bits(seen1[old]) == bits(seen0) and bits(miss1[old]) == bits(miss0)
    assert len(key1) > len(key0) and not seen1[~old].any() and not miss1[~old].any()
    both = built(0.5, CC.FOUR_CLOUDS[:3])
    for f in ("key", "count", "sums", "E", "M"):
        assert bits(records_of(cdst)[f]) == bits(records_of(both)[f]), f
    for m in (src, dst, direct, cdst, both):
        m.close()


# ------------------------------------------------------------------ refusals
def test_refusals():
    fine, plain = built(0.25, [CC.parent_corner()]), built(0.25, [CC.parent_corner()], False)
    cases = [(new_map(0.25), fine), (new_map(0.125), fine), (new_map(0.75), fine), (new_map(128.0, False), plain),
             (new_map(float(np.nextafter(0.5, 1.0))), fine), (new_map(0.5, False), fine), (new_map(0.5), plain), (fine, fine)]
    p07 = built(0.7, [CC.parent_corner()])
    cases.append((new_map(1.4), p07))                                         # moments at a leaf that is no multiple of 2^-16 m
    for dst, src in cases:
        before = everything(dst)
        with pytest.raises(api.SlamError) as e:
            dst.coarsen(src)
        assert e.value.code == api.E_INVALID and "slam_vmap_coarsen" in str(e.value)
        assert everything(dst) == before
    ok = new_map(64.0, False)                                                 # shift 8 is the last legal one
    ok.coarsen(plain)
    assert ok.info()["n_voxels"] == 1 and ok.info()["n_points"] == 2
    q07, q14 = built(0.7, [CC.parent_corner()], False), new_map(1.4, False)   # plain, 0.7 is legal
    q14.coarsen(q07)
    assert q14.info()["n_points"] == 2
    for m in {id(x): x for pair in cases for x in pair}.values():
        m.close()
    for m in (ok, q07, q14):
        m.close()


# ------------------------------------------------------------------ onward: a registration against a coarsened map
def test_registration_against_a_coarsened_map_returns_the_same_struct():
    clouds = V.builder_clouds(range(2))
    fine, direct, coarse = built(0.5, [clouds[0][0]]), built(2.0, [clouds[0][0]]), new_map(2.0)
    coarse.coarsen(fine)
    store = api.KeyframeStore(leaf_size=0.30, gate=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
    store.set_gicp_params(max_iterations=100, transformation_epsilon=1e-6)
    kid = store.add_keyframe(clouds[1][0])
    a = direct.register_gicp(store, kid, np.eye(4, dtype=np.float32), **GICP)
    b = coarse.register_gicp(store, kid, np.eye(4, dtype=np.float32), **GICP)
    assert a["iterations"] > 0 and a["pairs"] >= 3                             # a guard of the inputs: the registration ran
    assert {f: bits(v) if isinstance(v, np.ndarray) else v for f, v in a.items()} == {f: bits(v) if isinstance(v, np.ndarray) else v for f, v in b.items()}
    for m in (fine, direct, coarse):
        m.close()
    store.close()


# ------------------------------------------------------------------ handle lifetime
def test_create_coarsen_destroy_cycles_keep_device_memory_flat():
    """As tests/test_gpu_vmap_gicp.py sizes and checks it: a destination of 2^20 slots, so that a cycle's handle moves free
    device memory in pieces it can be read in; 40 cycles may cost at most what one cycle's handle holds while alive."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    src = built(0.25, CC.FOUR_CLOUDS)

    def cycle(alive=None):
        m = api.VoxelMap(leaf=1.0, initial_capacity=1 << 20)
        m.enable_distributions()
        m.coarsen(src)
        if alive is not None:
            alive.append(free_bytes(rt))
        got = (m.info()["n_voxels"], m.info()["n_points"])
        m.close()
        return got

    first = cycle()
    assert first[1] == sum(len(c[0]) for c in CC.FOUR_CLOUDS)
    for _ in range(2):
        cycle()
    free_after_warmup = free_bytes(rt)
    alive = []
    assert cycle(alive) == first
    size = free_after_warmup - alive[0]
    for _ in range(40):
        assert cycle() == first
    free_after = free_bytes(rt)
    print("vmap coarsen lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (size, free_after_warmup - free_after))
    assert size > 0 and free_after >= free_after_warmup - size
    src.close()
