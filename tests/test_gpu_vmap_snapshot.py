"""Save, load and merge of the voxel map on the device (slam_vmap_absorb[_dev], slam_vmap_merge, slam_vmap_save,
slam_vmap_load; docs/VOXEL_MAP.md section 10) against the Python restatement tests/vmap_snapshot_cases.py.  Every comparison is
bit for bit, through the key-ordered readers: absorb at the sizes around a wavefront and a workgroup, repeats, rejected records,
growth; the round trip through a file; merges of maps built from disjoint clouds against one map built from all; going on
after a load; handle lifetime."""
import signal

import numpy as np
import pytest

import vmap_cases as K
import vmap_oracle as V
import vmap_snapshot_cases as S
from slam_amd import api

pytestmark = pytest.mark.gpu
TEST_SECONDS = 300
PLANES = {"plain": (False, False), "carved": (True, False), "moments": (False, True), "both": (True, True)}
GICP = dict(gate=2.0, max_iterations=100, transformation_epsilon=1e-6)


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


def new_map(moments, leaf=K.LEAF, **kw):
    m = api.VoxelMap(leaf=leaf, **kw)
    if moments:
        m.enable_distributions()
    return m


def random_records(n, seed, carve, moments, span=6):
    """n records over (2 span)^3 cells: keys repeat within a call and across calls when span is small"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-span, span, (n, 3))
    key = np.array([S.key_of(*row) for row in c], np.uint64).reshape(n)
    r = dict(key=key, count=rng.integers(1, 60, n).astype(np.uint32), sums=rng.integers(-2 ** 41, 2 ** 41, (n, 3)))
    if carve:
        r.update(seen=rng.integers(0, 5, n).astype(np.uint32), miss=rng.integers(0, 5, n).astype(np.uint32))
    if moments:
        r.update(E3=rng.integers(-2 ** 36, 2 ** 36, (n, 3)), M6=rng.integers(-2 ** 56, 2 ** 56, (n, 6)))
    return r


def records_of(m):
    """the map's records through the key-ordered readers, under RefMap.records()'s names"""
    sums, count, key = m.read_sums()
    seen, miss, key2 = m.read_carve()
    out = dict(key=key, count=count, sums=sums, seen=seen, miss=miss)
    assert bits(key) == bits(key2)
    if m.layout()["distributions"]:
        out["E"], out["M"], key3 = m.read_moments()
        assert bits(key) == bits(key3)
    return out


def check(m, ref):
    """the device map against the restatement: every record plane, the counters and the carve state"""
    got, want = records_of(m), ref.records()
    for f in got:
        assert got[f].dtype == want[f].dtype and bits(got[f]) == bits(want[f]), f
    i, lay = m.info(), m.layout()
    assert (i["n_voxels"], i["n_points"]) == (ref.n_voxels, ref.n_points)
    assert (lay["carved"], lay["distributions"]) == (ref.carved, ref.moments)


def everything(m):
    """every reader of a map as bytes: what two equal maps must agree on"""
    out = {f: bits(a) for f, a in records_of(m).items()}
    out["read"] = [bits(a) for a in m.read()]
    i, lay = m.info(), m.layout()
    out["info"] = (i["n_voxels"], i["n_points"], lay["leaf"], lay["carved"], lay["distributions"])
    if lay["distributions"]:
        d = m.read_distributions()
        out["dist"] = {f: bits(d[f]) for f in d}
        out["dist_params"] = [getattr(lay["dist_params"], f) for f, _ in api.VmapDistParams._fields_]
    return out


def python_bytes(m):
    """the file the Python writer makes of the readers' output"""
    lay = m.layout()
    dist = {f: getattr(lay["dist_params"], f) for f, _ in api.VmapDistParams._fields_} if lay["distributions"] else None
    return S.write_file(lay["leaf"], records_of(m), n_points=m.info()["n_points"], carved=lay["carved"], dist=dist)


def built(which, carve, moments, leaf=K.LEAF, **kw):
    """a device map of FOUR_CLOUDS[which], each integrated (and carved) with its transform"""
    m = new_map(moments, leaf, **kw)
    for k in which:
        c, (R, t) = K.FOUR_CLOUDS[k]
        assert m.integrate(c, R, t) == 0
        if carve:
            m.carve(c, R, t)
    return m


# ------------------------------------------------------------------ absorb against the restatement
@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("start", ("empty", "filled"))
@pytest.mark.parametrize("planes", ("plain", "both"))
def test_absorb_sizes(n, start, planes):
    carve, moments = PLANES[planes]
    m, ref = new_map(moments), S.RefMap(moments)
    if start == "filled":
        r0 = random_records(100, 5, carve, moments)
        assert m.absorb(**r0) == ref.absorb(**r0) == 0
    r = random_records(n, 100 + n, carve, moments)
    assert m.absorb(**r) == ref.absorb(**r) == 0
    check(m, ref)
    if n > 64:
        assert len(set(r["key"].tolist())) < n       # keys repeat inside the call
    m.close()


def test_one_key_300_times_in_one_call():
    k = S.key_of(-7, 3, 1)
    n = 300
    r = dict(key=[k] * n, count=np.arange(1, n + 1), sums=np.arange(3 * n).reshape(n, 3) - 400, seen=[1] * n, miss=[2] * n,
             E3=np.arange(3 * n).reshape(n, 3) * -3, M6=np.arange(6 * n).reshape(n, 6) * 2 ** 40)
    m, ref = new_map(True), S.RefMap(True)
    assert m.absorb(**r) == ref.absorb(**r) == 0
    check(m, ref)
    assert m.info()["n_voxels"] == 1 and m.info()["n_points"] == n * (n + 1) // 2 and int(m.read_carve()[1][0]) == 2 * n
    m.close()


def test_invalid_records_among_valid_ones():
    r = random_records(257, 9, True, False, span=40)
    key, count = r["key"].copy(), r["count"].copy()
    good = int(key[0])
    key[3] = S.ALL_ONES
    key[64] = good | 1 << 63
    key[65] = good | S.FIELD                      # x field 2^21 - 1
    key[130] = good | S.FIELD << 21
    key[200] = good | S.FIELD << 42
    count[255] = 0
    count[256] = 0
    r.update(key=key, count=count)
    m, ref = new_map(False), S.RefMap(False)
    rejected = m.absorb(**r)
    assert rejected == ref.absorb(**r) == 7
    check(m, ref)
    keep = np.ones(257, bool)
    keep[[3, 64, 65, 130, 200, 255, 256]] = False
    i = m.info()
    assert i["n_points"] == int(count[keep].sum()) and i["n_voxels"] == len(set(key[keep].tolist()))
    m.close()


@pytest.mark.parametrize("planes", ("plain", "both"))
def test_growth_through_rehashes(planes):
    carve, moments = PLANES[planes]
    m, ref = new_map(moments, initial_capacity=64), S.RefMap(moments)
    caps = [m.info()["capacity"]]
    for j in range(6):
        r = random_records(100, 300 + j, carve, moments, span=8)
        assert m.absorb(**r) == ref.absorb(**r) == 0
        caps.append(m.info()["capacity"])
        check(m, ref)
    assert caps[0] == 64 and len(set(caps)) >= 4, caps          # at least three rehashes
    m.close()


@pytest.mark.parametrize("planes", ("plain", "both"))
def test_device_form_on_a_stream_equals_the_host_form(planes):
    carve, moments = PLANES[planes]
    r = random_records(257, 21, carve, moments)
    host, dev, ref = new_map(moments), new_map(moments), S.RefMap(moments)
    assert host.absorb(**r) == ref.absorb(**r) == 0
    st = api.Stream()
    d = {f: api.DeviceArray.from_host(np.ascontiguousarray(a)) for f, a in r.items()}
    api.synchronize()
    assert dev.absorb_dev(d["key"], d["count"], d["sums"], 257, d.get("seen"), d.get("miss"), d.get("E3"), d.get("M6"), stream=st) == 0
    check(host, ref)
    check(dev, ref)
    assert dev.absorb_dev(None, None, None, 0) == 0 and host.absorb([], [], []) == 0          # n = 0 touches nothing
    check(dev, ref)
    host.close()
    dev.close()


def test_refusals():
    r = random_records(10, 1, False, True)
    plain, dist = new_map(False), new_map(True)
    with pytest.raises(api.SlamError) as e:
        plain.absorb(**r)                                               # moments into a map without
    assert e.value.code == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        dist.absorb(r["key"], r["count"], r["sums"])                    # none into a map with
    assert e.value.code == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        plain.absorb(r["key"], r["count"], r["sums"], seen=r["count"])  # half a pair
    assert e.value.code == api.E_INVALID
    assert plain.info()["n_voxels"] == dist.info()["n_voxels"] == 0 and not plain.layout()["carved"]
    other = new_map(False, leaf=float(np.nextafter(K.LEAF, 1.0)))
    for dst, src in ((plain, plain), (plain, other), (plain, dist), (dist, plain)):
        with pytest.raises(api.SlamError) as e:
            dst.merge(src)
        assert e.value.code == api.E_INVALID
    for m in (plain, dist, other):
        m.close()


# ------------------------------------------------------------------ the round trip through a file
@pytest.mark.parametrize("planes", list(PLANES))
def test_save_load_round_trip(planes, tmp_path):
    carve, moments = PLANES[planes]
    m = built(range(4), carve, moments)
    want = everything(m)
    assert want["info"][0] > 500 and want["info"][3] == carve
    p = str(tmp_path / "m.vmap")
    m.save(p)
    saved = open(p, "rb").read()
    assert saved == python_bytes(m)                           # the library's writer against the Python writer
    f = S.read_file(saved)
    assert (f["n"], f["n_points"], f["flags"]) == (want["info"][0], want["info"][1], (1 if carve else 0) | (2 if moments else 0))
    loaded = api.VoxelMap.load(p)
    assert everything(loaded) == want
    assert loaded.info()["capacity"] == max(64, 1 << (2 * f["n"] - 1).bit_length())         # room at half load: the absorb did not grow
    p2 = str(tmp_path / "again.vmap")
    loaded.save(p2)
    assert open(p2, "rb").read() == saved
    # a file the Python writer made loads to the same map
    p3 = str(tmp_path / "python.vmap")
    open(p3, "wb").write(python_bytes(m))
    from_python = api.VoxelMap.load(p3)
    assert everything(from_python) == want
    # the bytes depend on the contents, not on how the map was built: another order, a small first table
    other = built((2, 0, 3, 1), carve, moments, initial_capacity=64)
    if not carve:                                             # a carve depends on what the map held when it ran
        other.save(p2)
        assert open(p2, "rb").read() == saved
    for x in (m, loaded, from_python, other):
        x.close()


def test_empty_maps_round_trip(tmp_path):
    for planes, (carve, moments) in PLANES.items():
        m = new_map(moments)
        if carve:
            m.carve(np.zeros((1, 3), np.float32) + 5)
        p = str(tmp_path / (planes + ".vmap"))
        m.save(p)
        b = open(p, "rb").read()
        assert len(b) == 96 and b == python_bytes(m)
        loaded = api.VoxelMap.load(p)
        assert everything(loaded) == everything(m)
        for x in (m, loaded):
            x.close()
    with pytest.raises(api.SlamError) as e:
        api.VoxelMap.load(str(tmp_path / "absent.vmap"))
    assert e.value.code == api.E_IO
    open(str(tmp_path / "bad.vmap"), "wb").write(b[:-1])
    with pytest.raises(api.SlamError) as e:
        api.VoxelMap.load(str(tmp_path / "bad.vmap"))
    assert e.value.code == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        new_map(False).save(str(tmp_path / "no_such_dir" / "m.vmap"))
    assert e.value.code == api.E_IO


# ------------------------------------------------------------------ merge
@pytest.mark.parametrize("planes", ("plain", "moments"))
def test_merge_of_disjoint_clouds_equals_one_map_of_all(planes, tmp_path):
    carve, moments = PLANES[planes]
    A, B, C = built((0, 1), carve, moments), built((2, 3), carve, moments), built(range(4), carve, moments)
    A2, B2 = built((0, 1), carve, moments, initial_capacity=64), built((2, 3), carve, moments)
    b_before, a2_before = everything(B), everything(A2)
    assert A.merge(B) == 0 and B2.merge(A2) == 0
    want = everything(C)
    assert everything(A) == want and everything(B2) == want
    assert everything(B) == b_before and everything(A2) == a2_before          # the source is unchanged
    files = []
    for name, m in (("a", A), ("b", B2), ("c", C)):
        m.save(str(tmp_path / name))
        files.append(open(str(tmp_path / name), "rb").read())
    assert files[0] == files[1] == files[2]
    # into an empty map: the source
    E = new_map(moments)
    assert E.merge(C) == 0 and everything(E) == want
    E2 = new_map(moments)
    assert E.merge(E2) == 0 and everything(E) == want and E2.info()["n_voxels"] == 0        # an empty source adds nothing
    for m in (A, B, C, A2, B2, E, E2):
        m.close()


@pytest.mark.parametrize("moments", (False, True))
def test_merge_adds_the_carve_planes(moments):
    A, B = built((0, 1), True, moments), built((2, 3), True, moments)
    ra, rb = records_of(A), records_of(B)
    ref = S.RefMap(moments)
    for r in (ra, rb):
        ref.absorb(r["key"], r["count"], r["sums"], r["seen"], r["miss"], r.get("E"), r.get("M"))
    assert int(ra["miss"].sum()) + int(rb["miss"].sum()) > 0 and int(ra["seen"].sum()) > 0 and int(rb["seen"].sum()) > 0
    assert A.merge(B) == 0
    check(A, ref)
    # a destination never carved gains the planes; a source never carved adds nothing to a carved destination's
    D = built((0, 1), False, moments)
    assert not D.layout()["carved"]
    assert D.merge(B) == 0 and D.layout()["carved"]
    ref2 = S.RefMap(moments)
    rd = ra          # read before A's merge: D holds the same clouds, never carved, so its seen and miss are not offered
    ref2.absorb(rd["key"], rd["count"], rd["sums"], None, None, rd.get("E"), rd.get("M"))
    ref2.absorb(rb["key"], rb["count"], rb["sums"], rb["seen"], rb["miss"], rb.get("E"), rb.get("M"))
    check(D, ref2)
    P = built((2, 3), False, moments)
    before = records_of(A)
    assert A.merge(P) == 0
    after = records_of(A)
    assert bits(after["seen"]) == bits(before["seen"]) and bits(after["miss"]) == bits(before["miss"])
    assert A.info()["n_points"] == sum(len(K.FOUR_CLOUDS[k][0]) for k in (0, 1, 2, 3, 2, 3))
    for m in (A, B, D, P):
        m.close()


# ------------------------------------------------------------------ onward from a loaded map
@pytest.mark.parametrize("planes", ("plain", "both"))
def test_a_loaded_map_goes_on_as_the_original_would(planes, tmp_path):
    carve, moments = PLANES[planes]
    three, four = built((0, 1, 2), carve, moments), built(range(4), carve, moments)
    p = str(tmp_path / "three.vmap")
    three.save(p)
    loaded = api.VoxelMap.load(p)
    c, (R, t) = K.FOUR_CLOUDS[3]
    assert loaded.integrate(c, R, t) == 0
    if carve:
        loaded.carve(c, R, t)
    assert everything(loaded) == everything(four)
    for m in (three, four, loaded):
        m.close()


def test_registration_against_a_loaded_map_returns_the_same_struct(tmp_path):
    clouds = V.builder_clouds(range(2))
    dm = new_map(True, leaf=1.0)
    dm.integrate(clouds[0][0])
    p = str(tmp_path / "dist.vmap")
    dm.save(p)
    loaded = api.VoxelMap.load(p)
    store = api.KeyframeStore(leaf_size=0.30, gate=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
    store.set_gicp_params(max_iterations=100, transformation_epsilon=1e-6)
    kid = store.add_keyframe(clouds[1][0])
    a = dm.register_gicp(store, kid, np.eye(4, dtype=np.float32), **GICP)
    b = loaded.register_gicp(store, kid, np.eye(4, dtype=np.float32), **GICP)
    assert a["converged"] and a["pairs"] > 1000
    assert {f: bits(v) if isinstance(v, np.ndarray) else v for f, v in a.items()} == {f: bits(v) if isinstance(v, np.ndarray) else v for f, v in b.items()}
    for m in (dm, loaded):
        m.close()
    store.close()


# ------------------------------------------------------------------ handle lifetime
def test_load_and_absorb_cycles_keep_device_memory_flat(tmp_path):
    """As tests/test_gpu_vmap_gicp.py sizes and checks it: tables of 2^20 slots, so that a cycle's handle moves free device
    memory in pieces it can be read in; 40 cycles may cost at most what one cycle's handle holds while alive."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    n = 1 << 19
    i = np.arange(n, dtype=np.int64)
    key = ((i % 1000 + 1) | ((i // 1000 + 1) << 21) | (np.int64(7) << 42)).astype(np.uint64)
    assert np.all(key[1:] > key[:-1])
    rec = dict(key=key, count=np.ones(n, np.uint32), sums=np.zeros((n, 3), np.int64))
    p = str(tmp_path / "big.vmap")
    open(p, "wb").write(S.write_file(0.3, rec))
    small = random_records(257, 4, True, False)

    def load_cycle(alive=None):
        m = api.VoxelMap.load(p)
        if alive is not None:
            alive.append(free_bytes(rt))
        got = (m.info()["n_voxels"], m.info()["capacity"])
        m.close()
        return got

    def absorb_cycle(alive=None):
        m = api.VoxelMap(leaf=0.3, initial_capacity=1 << 20)
        m.absorb(**small)
        if alive is not None:
            alive.append(free_bytes(rt))
        got = (m.info()["n_voxels"], m.layout()["carved"])
        m.close()
        return got

    for name, cycle, first in (("load", load_cycle, (n, 1 << 20)), ("absorb", absorb_cycle, (len(set(small["key"].tolist())), True))):
        for _ in range(3):
            assert cycle() == first
        free_after_warmup = free_bytes(rt)
        alive = []
        assert cycle(alive) == first
        size = free_after_warmup - alive[0]
        for _ in range(40):
            assert cycle() == first
        free_after = free_bytes(rt)
        print("vmap %s lifetime: S = %d bytes, drift over 40 cycles %d bytes" % (name, size, free_after_warmup - free_after))
        assert size > 0 and free_after >= free_after_warmup - size
