"""slam_kf_sc_* (slam_amd/csrc/kf_sc.hip) against its scalar restatement (tests/cpp/sc_oracle.cpp), bit for bit: the
descriptor on the filtered cloud as the store holds it, the search on every pair; then the convention of the shift and of
the rotation that seeds a registration, and place recognition on the synthetic loop.  docs/SCAN_CONTEXT.md."""
import ctypes as C
import signal

import numpy as np
import pytest

import sc_cases as K
import sc_oracle as SO
from slam_amd import api

pytestmark = pytest.mark.gpu
TEST_SECONDS = 120
NONE = (-1, 0, 0, 0, 0)


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


def make_store(p, clouds=(), leaf=K.LEAF):
    store = api.KeyframeStore(leaf_size=leaf)
    store.set_sc_params(**p.dict())
    for c in clouds:
        store.add_keyframe(c)
    return store


def restated(store, p, tabs, kid):
    return SO.descriptor(store.read_keyframe(kid)[:, :3], p, tabs)


def check_pairs(store, p, tabs, removed=()):
    """every live keyframe against every id, in one call; -> the call's result"""
    live = [k for k in range(len(store)) if k not in removed]
    got = store.sc_match(live)
    desc = {k: restated(store, p, tabs, k) for k in live}
    for row, q in zip(got, live):
        for k in range(len(store)):
            want = NONE if (k == q or k in removed) else SO.match(desc[q], desc[k])
            assert tuple(int(v) for v in row[k]) == want, (q, k)
    return got


def refused(fn, *args, **kw):
    with pytest.raises(api.SlamError) as e:
        fn(*args, **kw)
    return e.value.code == api.E_INVALID


@pytest.mark.parametrize("name", sorted(K.PARAM_SETS))
def test_tables_are_libm_within_one_ulp(name):
    p = K.PARAM_SETS[name]
    got, want = make_store(p).sc_tables(), SO.tables(p)
    for g, w in zip(got, want):
        assert np.abs(g.view(np.int64) - w.view(np.int64)).max() <= 1
    assert np.array_equal(got[0], want[0])               # the ring edges are plain arithmetic


@pytest.mark.parametrize("name", sorted(K.PARAM_SETS))
def test_descriptor_equals_restatement(name):
    p = K.PARAM_SETS[name]
    store = make_store(p)
    tabs = store.sc_tables()
    clouds = K.descriptor_clouds(p, tabs)
    for _, c in clouds[:-1]:
        store.add_keyframe(c)
    store.sc_compute()                                   # the batch: one launch for all of them
    last = store.add_keyframe(clouds[-1][1])
    store.sc_compute(last)                               # ... and one keyframe by its id
    store.sc_compute()                                   # nothing left to do
    for k, (cname, cloud) in enumerate(clouds):
        got = store.sc_read(k)
        assert got.shape == (p.n_rings, p.n_sectors) and got.dtype == np.uint8
        assert np.array_equal(got, restated(store, p, tabs, k)), cname
    # the edges reach the kernel: the filter hands single points of short coordinates on as they were
    f = store.read_keyframe(0)[:, :3].astype(np.float64)
    assert np.isin(tabs[0], f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]).all()
    per = p.n_sectors // 4
    if per % 2 == 0:
        k = per // 2
        assert ((f[:, 1] * tabs[1][k] == f[:, 0] * tabs[2][k]) & (f[:, 0] > 0) & (f[:, 1] > 0)).any()
    if p.n_sectors >= 16:                                # the height points have a cell each: both ends of the clamp are there
        assert store.sc_read(0).max() == 255 and store.sc_read(0)[store.sc_read(0) > 0].min() == 1
    # the search on what the edge clouds gave, these parameters' word and thread layout included
    check_pairs(store, p, tabs)


@pytest.mark.parametrize("sname", ["one", "two", "seventy", "identical", "tie", "empty", "rolled"])
def test_search_equals_restatement(sname):
    p = K.PARAM_SETS["twenty_by_64"]
    store = make_store(p, K.match_sets(p)[sname])
    got = check_pairs(store, p, store.sc_tables())
    if sname == "identical":
        assert tuple(got[0][1]) [:2] == (0, 0) and got[0][1]["n_both"] == got[0][1]["n_query"] > 0
    if sname == "tie":
        assert int(got[0][1]["shift"]) == 3 and tuple(got[0][1])[2:] == (1, 2, 1)
    if sname == "empty":
        assert not store.sc_read(0).any() and int(got[0][1]["distance"]) == int(store.sc_read(1).astype(np.int64).sum())
        assert int(got[0][1]["shift"]) == 0


@pytest.mark.parametrize("name", ["most", "one_ring_four_sectors", "sixty"])
def test_search_on_other_layouts(name):
    p = K.PARAM_SETS[name]
    sets = K.match_sets(p)
    store = make_store(p, sets["rolled"] + sets["tie"] + sets["empty"] + sets["two"])
    check_pairs(store, p, store.sc_tables())


def test_removed_and_replaced_keyframes():
    p = K.PARAM_SETS["twenty_by_64"]
    clouds = K.match_sets(p)["seventy"][:5]
    store = make_store(p, clouds)
    tabs = store.sc_tables()
    before = check_pairs(store, p, tabs)
    store.remove_keyframe(1)
    after = check_pairs(store, p, tabs, removed=(1,))
    live = [0, 2, 3, 4]
    for i, q in enumerate(live):
        assert tuple(after[i][1]) == NONE
        for k in live:
            assert after[i][k] == before[q][k]          # nothing changes for the keyframes that stay
    assert refused(store.sc_read, 1) and refused(store.sc_compute, 1) and refused(store.sc_match, [1])
    old = store.sc_read(2)
    store.replace_keyframe(2, K.random_cloud(999, 350, p))
    assert refused(store.sc_read, 2)                     # the descriptor went with the cloud
    check_pairs(store, p, tabs, removed=(1,))            # ... and is computed again on demand
    assert not np.array_equal(store.sc_read(2), old) and np.array_equal(store.sc_read(2), restated(store, p, tabs, 2))


def test_a_pair_does_not_depend_on_the_batch_and_calls_repeat():
    p = K.PARAM_SETS["twenty_by_64"]
    clouds = K.match_sets(p)["seventy"][:12]
    store = make_store(p, clouds)
    everything = store.sc_match(range(12))
    assert np.array_equal(everything, store.sc_match(range(12)))
    some = store.sc_match([5, 3, 5, 11])
    for row, q in zip(some, [5, 3, 5, 11]):
        assert np.array_equal(row, everything[q])
    two = make_store(p, [clouds[7], clouds[2]])
    assert two.sc_match([0])[0][1] == everything[7][2] and two.sc_match([1])[0][0] == everything[2][7]


def test_refusals_leave_everything_as_it_was():
    p = K.PARAM_SETS["twenty_by_64"]
    store = make_store(p, K.match_sets(p)["two"])
    tabs = store.sc_tables()
    for bad in (dict(n_rings=0), dict(n_rings=33), dict(n_sectors=0), dict(n_sectors=62), dict(n_sectors=132), dict(max_range=0.0),
                dict(max_range=float("nan")), dict(z_step=0.0), dict(z_step=-1.0), dict(z_min=float("inf"))):
        assert refused(store.set_sc_params, **dict(p.dict(), **bad)), bad
    assert all(np.array_equal(a, b) for a, b in zip(tabs, store.sc_tables()))
    L = api.lib()
    desc = np.full(p.n_rings * p.n_sectors, 7, np.uint8)
    r, s = C.c_int(-5), C.c_int(-6)
    assert L.slam_kf_sc_read(store.h, 0, desc.ctypes.data_as(C.c_void_p), desc.size, C.byref(r), C.byref(s)) == api.E_INVALID   # none yet
    assert (r.value, s.value) == (-5, -6) and (desc == 7).all()
    out = np.full((2, len(store)), -9, api.SC_MATCH_DTYPE)
    for queries in ([0, 2], [-1, 0], [0, 7]):
        q = np.array(queries, np.int32)
        assert L.slam_kf_sc_match(store.h, q.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.POINTER(api.KfScMatch)), None) == api.E_INVALID
    assert all((out[f] == -9).all() for f in out.dtype.names)
    assert refused(store.sc_compute, 2) and refused(store.sc_compute, -2)
    store.set_sc_params(**dict(p.dict(), n_rings=7))     # no descriptor yet: free to change
    store.set_sc_params(**p.dict())
    store.sc_compute(0)
    assert refused(store.set_sc_params, **dict(p.dict(), z_min=-0.25))          # fixed from the first descriptor on
    store.set_sc_params(**p.dict())                      # the same values are no change
    assert L.slam_kf_sc_read(store.h, 0, desc.ctypes.data_as(C.c_void_p), desc.size - 1, C.byref(r), C.byref(s)) == api.E_INVALID
    assert (desc == 7).all()
    assert np.array_equal(store.sc_read(0), restated(store, p, tabs, 0))


# ---------------------------------------------------------------- the conventions
def rz(yaw):
    m = np.eye(4)
    m[0, 0] = m[1, 1] = np.cos(yaw)
    m[0, 1], m[1, 0] = -np.sin(yaw), np.sin(yaw)
    return m


def yaw_of(T):
    return float(np.arctan2(T[1, 0], T[0, 0]))


@pytest.fixture(scope="module")
def place():
    return K.place_clouds()


def test_shift_and_seed_rotation_have_the_documented_sign(place):
    """Keyframe 1 is keyframe 0's cloud turned about z by +5 sectors.  The candidate rolled by +shift lies on the query, so
    query 1 finds candidate 0 at shift 5 (and 0 finds 1 at -5); the registration of source 1 onto target 0 starts from
    Rz(-shift 2 pi / n_sectors), which here is the true transform.  Bounds: the seed is the truth up to the two clouds'
    different voxel centroids, so ICP must stay within a fifth of the 0.5 m leaf and 0.02 rad (0.1 m at 5 m, where the
    cloud is densest); seeded with the opposite sign it starts 56 degrees off, beyond what the 0.75 m gate can bring
    back, and must end more than 0.2 rad from the truth."""
    p = SO.Params(max_range=K.PLACE_MAX_RANGE)
    step = 2.0 * np.pi / p.n_sectors
    base = place[0][0]
    store = make_store(p, [base, K.rotate_z(base, 5 * step)], leaf=0.5)
    m = store.sc_match([0, 1])
    assert int(m[1][0]["shift"]) == 5 and int(m[0][1]["shift"]) == p.n_sectors - 5
    cands = store.loop_candidates(1, k=3, min_gap=0)
    assert [c[:3] for c in cands] == [(0, int(m[1][0]["distance"]), 5)] and abs(cands[0][3] + 5 * step) < 1e-12
    truth = rz(-5 * step)
    good, bad = store.register_edges([(0, 1, rz(cands[0][3])), (0, 1, rz(-cands[0][3]))])
    Tg, Tb = np.array(good["transform"]).reshape(4, 4), np.array(bad["transform"]).reshape(4, 4)
    err_g = (abs(yaw_of(Tg) - yaw_of(truth)), float(np.linalg.norm(Tg[:3, 3])))
    err_b = abs(yaw_of(Tb) - yaw_of(truth))
    print("sign test: documented seed ends %.5f rad, %.4f m from the truth; the opposite seed %.4f rad" % (err_g + (err_b,)))
    assert err_g[0] <= 0.02 and err_g[1] <= 0.1
    assert err_b > 0.2


def test_place_recognition_on_the_loop(place):
    """All 24 queries: the best keyframe among 0 .. 23 is one of the two true neighbours and its shift is within one sector
    of (phi + th_kf - th_q) / (2 pi / n_sectors).  No allowance."""
    kf, kf_pose, qs, q_pose, phis = place
    p = SO.Params(max_range=K.PLACE_MAX_RANGE)
    store = make_store(p, kf + qs, leaf=0.5)
    m = store.sc_match(range(24, 48))
    res = [K.place_check(m[j], j, kf_pose, q_pose, phis[j], p.n_sectors) for j in range(24)]
    print("place recognition: %d / 24 neighbours, %d / 24 shifts, nearest wrong / best >= %.3f"
          % (sum(r[0] for r in res), sum(bool(r[1]) for r in res), min(r[2] for r in res)))
    assert all(r[0] for r in res) and all(r[1] for r in res)
    tabs = store.sc_tables()
    for k in (0, 23, 24, 47):                            # ... on descriptors that are the restatement's
        assert np.array_equal(store.sc_read(k), restated(store, p, tabs, k))
