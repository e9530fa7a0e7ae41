"""The pending store and the closure kernel of slam_mls_* (slam_amd/csrc/mls.hip) at their edges, device against the
scalar restatement bit for bit: the store growing with carried points in it (grow_store), with calls in flight, the
host's bound of the carried count above the device's count (pad_keys_kernel, an empty cloud, a clear between adds in
flight), closure rounds wider than the workgroup and chains of hundreds of rounds, and a cell of more than 16
clusters.  The scenes and what they rest on: tests/mls_store_cases.py, tests/test_mls_store_cases.py."""
import numpy as np
import pytest

import mls_map_oracle as MO
import mls_store_cases as SC
from slam_amd import api
from test_gpu_mls_map import both, check_segmented

pytestmark = pytest.mark.gpu
S = SC.GROW_S
EMPTY = np.zeros((0, 3), np.float32)


def pair(size, **kw):
    dev = api.MlsMap(size, size, 1.0, params=SC.params(**kw))
    return dev, MO.OracleMls(size, size, 1.0, dev.params)


def pending(ora):
    return int(ora.read_cells(np.arange(ora.cells, dtype=np.int32), clusters=False)["pending"].sum())


def device_cloud(cloud):
    return api.DeviceArray.from_host(cloud if len(cloud) else np.zeros((1, 3), np.float32), np.float32)


def step(dev, ora, cloud, pose, what):
    """one synchronised call on both sides, the whole map compared, and the carried count with it"""
    both(dev, ora, "add_cloud", cloud, pose)
    MO.compare(dev, ora, what)
    assert dev.info()["pending_points"] == pending(ora), what
    return pending(ora)


def test_store_grows_with_carried_points_and_again():
    dev, ora = pair(S, **SC.GROW)
    assert step(dev, ora, SC.carried_cloud(), (0.0, 0.0), "carried") == 304
    # 2^20 points, 3 024 of them live: 304 + 2^20 exceeds the 2^20 of create, the store grows around the carried points
    assert step(dev, ora, SC.mostly_dropped_cloud(2 ** 20, 1), (0.0, 0.0), "first growth") == 304
    # the window moves over the carried cells; with no new point they are consumed, in the order they arrived in
    assert step(dev, ora, EMPTY, SC.CARRIED_POSE, "carried consumed") == 0
    # carried points again (cells x 225..234, outside the window x 180..219), and a second growth past 2^21
    assert step(dev, ora, SC.carried_cloud(x0=225), SC.CARRIED_POSE, "carried again") == 304
    big = SC.mostly_dropped_cloud(2 ** 21 + 1, 2, x_lo=182, x_hi=218, far=(-49.5, 0.5))     # 99.5 m from the pose
    assert step(dev, ora, big, SC.CARRIED_POSE, "second growth") == 304
    # an ordinary call: the window over the second carried batch, new points into some of its cells
    assert step(dev, ora, SC.flat_cloud(S, [(x, 150) for x in range(222, 240)], z=0.25), (80.0, 0.0), "after the growths") == 0
    check_segmented(dev, ora, "growth")
    dev.close()


def test_store_grows_with_calls_in_flight():
    dev, ora = pair(S, **SC.GROW)
    st = api.Stream()
    clouds = [SC.carried_cloud(), SC.flat_cloud(S, [(x, y) for x in range(140, 146) for y in range(160, 166)], z=0.5),
              SC.mostly_dropped_cloud(2 ** 20, 3)]
    bufs = [device_cloud(c) for c in clouds]
    dev.set_pose(0.0, 0.0)
    for c, d in zip(clouds, bufs):                          # the third finds 304 + 108 + 2^20 above the capacity
        dev.add_cloud_dev(d, len(c), 3, st)
    st.synchronize()
    for c in clouds:
        ora.add_cloud(c, (0.0, 0.0))
    MO.compare(dev, ora, "growth in flight")
    assert dev.info()["pending_points"] == pending(ora) == 304
    assert step(dev, ora, EMPTY, SC.CARRIED_POSE, "carried consumed") == 0
    check_segmented(dev, ora, "growth in flight")
    dev.close()


def test_bound_above_the_count_clear_in_flight_and_empty_clouds():
    """Calls enqueued without a wait, each consuming what the one before left pending: the host's bound (the last
    count it has seen plus the clouds still in flight) stays above the device's count, and the sort runs over
    padding.  A clear between them, then an empty cloud (n = 0), which finds the bound above a count of zero when
    the host is ahead at that moment (otherwise bound and count are both zero and the call returns at once).
    Every other cloud ends in 3 000 points of one cell of the window: a serial chain of 3 000 dependent updates, far
    longer than the host needs to enqueue a call, so that the host does run ahead (at most two calls, by design).
    On a host too slow for that the test checks less; it cannot fail for it."""
    dev, ora = pair(S, **SC.GROW)
    st = api.Stream()
    east, west = SC.carried_cloud(), SC.carried_cloud(x0=95)
    here, over_east, over_west = (0.0, 0.0), SC.CARRIED_POSE, (-50.0, 0.0)     # windows x 130..169, 180..219, 80..119
    ballast_only = east[:0]                                 # nothing but the 3 000 points appended below
    seq = [(here, east), (over_east, ballast_only),         # pending 304, then consumed while the bound says 304 + 3 000
           (here, west), (over_west, ballast_only), (here, east),
           (over_east, SC.flat_cloud(S, [(x, 150) for x in range(190, 215)], z=0.3)),
           "clear",
           (here, None),                                    # None: no point at all, n = 0 (bin_kernel is skipped)
           (here, west),
           (here, east[::-1].copy()),                       # 608 pending
           (over_west, ballast_only),                       # the western half of 608 consumed, the eastern moves down
           (over_east, ballast_only), (here, SC.flat_cloud(S, [(x, 140) for x in range(135, 165)]))]
    assert len(seq) == 13                                   # twelve calls and the clear
    calls = []
    for item in seq:
        if item != "clear":
            pose, cloud = item
            ballast = SC.cell_points(S, int(pose[0]) + S // 2 + 3, 135, [0.5] * 3000)
            cloud = EMPTY if cloud is None else np.concatenate([cloud, ballast])
            item = (pose, cloud, device_cloud(cloud))
        calls.append(item)
    for item in calls:                                      # everything is on the device: nothing below waits
        if item == "clear":
            dev.clear(st)
        else:
            dev.set_pose(*item[0])
            dev.add_cloud_dev(item[2], len(item[1]), 3, st)
    st.synchronize()
    for item in calls:
        ora.clear() if item == "clear" else ora.add_cloud(item[1], item[0])
    MO.compare(dev, ora, "bound above the count")
    assert dev.info()["pending_points"] == pending(ora) == 0
    check_segmented(dev, ora, "bound above the count")
    dev.close()


@pytest.mark.parametrize("field", ["ring", "corridor"])
def test_closure_rounds(field):
    """ring: a round with more open walks, and one with more claimed cells, than closure_kernel has threads;
    corridor: 256 rounds of one claim each"""
    cells, pose, u = SC.ring_field(S, 130) if field == "ring" else SC.corridor(S, 256)
    rounds = SC.schedule(S, cells, pose, u)
    dev, ora = pair(S, update_dist=u, max_clusters=2, **SC.FLAT)
    both(dev, ora, "add_cloud", SC.flat_cloud(S, cells), pose)
    MO.compare(dev, ora, field)
    assert ora.outside_updates() == sum(c for _, c in rounds) and ora.updates() == len(cells)
    assert dev.info()["pending_points"] == 0
    check_segmented(dev, ora, field)
    dev.close()


def test_more_than_sixteen_clusters_in_a_cell():
    dev, ora = pair(20, max_clusters=40)
    for part in (0, 1):
        both(dev, ora, "add_cloud", SC.tall_cell_cloud(20, 3, 3, part), (0.0, 0.0))
        MO.compare(dev, ora, "tall cell %d" % part)
    assert ora.read_cells([3 + 20 * 3])["n_clusters"][0] == 20
    # ten more points at one height give the cell a ground cluster: the pending points are consumed, the cell gets a state
    both(dev, ora, "add_cloud", SC.cell_points(20, 3, 3, [4.0] * 10), (0.0, 0.0))
    MO.compare(dev, ora, "tall cell ground")
    assert dev.info()["pending_points"] == pending(ora) == 0
    check_segmented(dev, ora, "tall cell")
    dev.close()
