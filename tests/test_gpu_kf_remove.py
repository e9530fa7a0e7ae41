"""slam_kf_remove_keyframe and slam_kf_replace_keyframe_dev (slam_amd/csrc/kf_store.hip): the store gives a keyframe's
memory back, refuses the id from then on, and a replaced keyframe is, bit for bit, the keyframe a fresh store would hold;
nothing changes for the keyframes that stay."""
import signal

import numpy as np
import pytest

import kf_edge_oracle as KE
from slam_amd import api, synth
from test_gpu_kf_gicp import same_edge, same_result

pytestmark = pytest.mark.gpu
TEST_SECONDS = 300
KS = (0, 1, 2, 3)


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


@pytest.fixture(scope="module")
def clouds():
    """four small scans of the loop (16 rings x 512 azimuths) and their poses"""
    return [synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512) for k in KS]


def init(clouds, frm, to):
    return KE.relative_init(clouds[frm][1], clouds[to][1])


def requests(store, edges):
    """both solvers on the same edges: (ICP results, GICP results)"""
    return store.register_edges(edges), store.register_gicp(edges)


def same_all(a, b):
    return all(same_edge(x, y) for x, y in zip(a[0], b[0])) and all(same_result(x, y) for x, y in zip(a[1], b[1]))


def refused(fn, *args):
    with pytest.raises(api.SlamError) as e:
        fn(*args)
    return e.value.code == api.E_INVALID


def test_add_remove_cycles_keep_device_memory_flat(clouds):
    """Free device memory moves in pieces far larger than one small keyframe (one keyframe alone read as 0 bytes on the
    MI355X), and the runtime may keep freed pieces for the next allocation.  So the instrument is calibrated first: H is
    what 200 keyframes cost while all of them are held, which must be at least half of 200 times what the store says one
    holds.  After their removal free memory is the baseline; holding and removing 200 again, and then 200 add -> remove
    cycles with covariances computed in each, may each leave at most H / 4 less than that: a keyframe leaked per removal costs
    about H, in every fourth H / 4; a covariance block (212 bytes per point, four times the keyframe's own) leaked per cycle 4 H."""
    from test_gpu_lifetime import free_bytes, hip_runtime
    rt = hip_runtime()
    store = api.KeyframeStore()
    keep = store.add_keyframe(clouds[0][0])
    first = store.read_keyframe(keep).copy()
    d = api.DeviceArray.from_host(clouds[1][0])
    n = len(clouds[1][0])
    for _ in range(3):                                   # warm-up: the store's staging buffers reach their size
        store.remove_keyframe(store.add_keyframe_dev(d, n))

    def hold_and_remove():
        before = free_bytes(rt)
        held = [store.add_keyframe_dev(d, n) for _ in range(200)]
        cost, one = before - free_bytes(rt), store.info(held[0])["device_bytes"]
        for kid in held:
            store.remove_keyframe(kid)
        return cost, one

    H, S = hold_and_remove()                             # S: the cloud and its lattice, by the store's own count
    baseline = free_bytes(rt)
    hold_and_remove()
    after_second = baseline - free_bytes(rt)
    for _ in range(200):
        kid = store.add_keyframe_dev(d, n)
        store.compute_covariances(kid)                   # every cycle: 200 leaked covariance blocks (0.8 MB each) are 4 H
        store.remove_keyframe(kid)
    drift = baseline - free_bytes(rt)
    print("kf remove: one keyframe holds %d bytes, 200 held cost %d; below the baseline after holding and removing 200 again %d, "
          "after 200 add -> remove cycles %d bytes" % (S, H, after_second, drift))
    assert S > 0 and H >= 100 * S                        # the instrument sees 200 keyframes
    assert after_second < H / 4 and drift < H / 4
    assert len(store) == 1 + 3 + 400 + 200 and kid == len(store) - 1     # ids are never issued twice
    assert np.array_equal(store.read_keyframe(keep), first)
    store.close()


def test_a_removed_id_is_refused_everywhere(clouds):
    store = api.KeyframeStore()
    ids = [store.add_keyframe(c) for c, _ in clouds[:3]]
    store.compute_covariances(ids[1])
    store.remove_keyframe(ids[1])
    assert len(store) == 3
    q = clouds[1][0][:10]
    T = init(clouds, 0, 1)
    for fn, args in ((store.info, (1,)), (store.read_keyframe, (1,)), (store.nearest, (1, q)), (store.compute_covariances, (1,)),
                     (store.covariances, (1,)), (store.neighbours, (1,)), (store.remove_keyframe, (1,)),
                     (store.replace_keyframe, (1, clouds[3][0])), (store.register_edges, ([(0, 1, T)],)),
                     (store.register_edges, ([(1, 0, T)],)), (store.register_gicp, ([(0, 1, T)],)), (store.register_gicp, ([(1, 2, T)],)),
                     (store.register_gicp, ([(0, 2, T), (2, 1, T)],)), (store.remove_keyframe, (7,)), (store.remove_keyframe, (-1,))):
        assert refused(fn, *args), (fn.__name__, args[0])
    assert api.lib().slam_kf_remove_keyframe(None, 0) == api.E_INVALID
    assert api.lib().slam_kf_replace_keyframe_dev(None, 0, None, 0, 3, None) == api.E_INVALID
    # the parameters the keyframes fixed stay fixed, even with every keyframe gone
    store.remove_keyframe(0)
    store.remove_keyframe(2)
    assert refused(lambda: store.set_params(leaf_size=0.25))
    assert refused(lambda: store.set_gicp_params(k_correspondences=10))
    # and the store goes on: the next id is new
    assert store.add_keyframe(clouds[3][0]) == 3 and store.info(3)["n_points"] > 0
    store.close()


def test_replace_gives_the_bits_of_a_fresh_store(clouds):
    a = api.KeyframeStore()
    a.add_keyframe(clouds[0][0])
    a.add_keyframe(clouds[1][0])
    a.register_gicp([(0, 1, init(clouds, 0, 1))])          # keyframe 0 holds covariances that the replacement must drop
    before = a.info(0)
    a.replace_keyframe(0, clouds[2][0])
    assert len(a) == 2 and a.info(0) != before
    b = api.KeyframeStore()
    b.add_keyframe(clouds[2][0])
    b.add_keyframe(clouds[1][0])
    assert a.info(0) == b.info(0) and np.array_equal(a.read_keyframe(0).view(np.uint32), b.read_keyframe(0).view(np.uint32))
    edges = [(0, 1, init(clouds, 2, 1)), (1, 0, init(clouds, 1, 2))]
    ra, rb = requests(a, edges), requests(b, edges)
    assert same_all(ra, rb)
    assert all(r["pairs"] > 0 and r["fitness_pairs"] > 0 for r in ra[1])     # no empty comparison
    assert np.array_equal(a.covariances(0).view(np.uint64), b.covariances(0).view(np.uint64))
    # the device form with a stride, onto the source side
    pts = np.zeros((len(clouds[3][0]), 4), np.float32)
    pts[:, :3] = clouds[3][0]
    a.replace_keyframe_dev(1, api.DeviceArray.from_host(pts), len(pts), 4)
    b2 = api.KeyframeStore()
    b2.add_keyframe(clouds[2][0])
    b2.add_keyframe(clouds[3][0])
    edges = [(0, 1, init(clouds, 2, 3))]
    assert same_all(requests(a, edges), requests(b2, edges))
    for s in (a, b, b2):
        s.close()


def test_a_failed_replace_keeps_the_old_keyframe(clouds):
    store = api.KeyframeStore()
    store.add_keyframe(clouds[0][0])
    store.add_keyframe(clouds[1][0])
    edges = [(0, 1, init(clouds, 0, 1))]
    before, cloud = requests(store, edges), store.read_keyframe(0).copy()
    nothing = np.full((50, 3), np.nan, np.float32)      # no finite point: slam_kf_add_keyframe_dev refuses it
    assert refused(store.replace_keyframe, 0, nothing)
    assert refused(store.replace_keyframe, 0, np.zeros((0, 3), np.float32))
    assert len(store) == 2 and np.array_equal(store.read_keyframe(0).view(np.uint32), cloud.view(np.uint32))
    assert same_all(requests(store, edges), before)
    store.close()


def test_the_other_keyframes_answer_the_same_after_a_removal(clouds):
    store = api.KeyframeStore()
    for c, _ in clouds:
        store.add_keyframe(c)
    edges = [(0, 1, init(clouds, 0, 1)), (3, 0, init(clouds, 3, 0)), (1, 3, init(clouds, 1, 3))]
    before = requests(store, edges)
    nn = store.nearest(3, clouds[0][0][:200])
    store.remove_keyframe(2)
    assert same_all(requests(store, edges), before)
    after = store.nearest(3, clouds[0][0][:200])
    assert np.array_equal(nn[0], after[0]) and np.array_equal(nn[1].view(np.uint32), after[1].view(np.uint32))
    assert [store.info(k)["n_points"] > 0 for k in (0, 1, 3)] == [True] * 3
    store.close()
