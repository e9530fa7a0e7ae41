"""The conditions the device tests of tests/test_gpu_mls_map_store.py rest on, held on the restatement
(tests/cpp/mls_map_oracle.cpp) and the round-schedule model (tests/mls_store_cases.py) alone: no GPU."""
import numpy as np
import pytest

import mls_map_oracle as MO
import mls_store_cases as SC

S, RING_U, CORRIDOR_L = 300, 130, 256
CLOSURE_THREADS = 1024      # kClosureThreads of mls.hip: the stride of closure_kernel's two loops


def run_flat(cells, pose, u, max_clusters=2):
    ora = MO.OracleMls(S, S, 1.0, SC.params(update_dist=u, max_clusters=max_clusters, **SC.FLAT))
    ora.add_cloud(SC.flat_cloud(S, cells), pose)
    return ora


@pytest.fixture(scope="module")
def ring():
    cells, pose, u = SC.ring_field(S, RING_U)
    return cells, SC.schedule(S, cells, pose, u), run_flat(cells, pose, u)


@pytest.fixture(scope="module")
def corridor():
    cells, pose, u = SC.corridor(S, CORRIDOR_L)
    return cells, SC.schedule(S, cells, pose, u), run_flat(cells, pose, u)


def test_schedule_of_the_hand_chain():
    """test_out_of_window_closure_chain (S = 20): (11, 5) waits, (12..14, 5) are claimed one per round, (16, 5) never"""
    cells = [(x, 5) for x in (11, 12, 13, 14, 16)]
    assert SC.schedule(20, cells, (0.0, -5.0), 2) == [(1, 1), (2, 1), (2, 1), (2, 0)]


def test_ring_field_fills_both_loops_of_a_round(ring):
    cells, rounds, ora = ring
    assert len(cells) == 2080 and len(set(cells)) == 2080
    assert rounds[0][0] > CLOSURE_THREADS, rounds           # the first loop strides: more open walks than threads
    assert max(c for _, c in rounds) > CLOSURE_THREADS, rounds    # and the second: more claimed cells than threads


def test_corridor_is_a_chain_of_rounds(corridor):
    cells, rounds, ora = corridor
    assert len(cells) == CORRIDOR_L + 1
    assert sum(1 for _, c in rounds if c == 1) >= CORRIDOR_L and len(rounds) >= CORRIDOR_L >= 256


@pytest.mark.parametrize("which", ["ring", "corridor"])
def test_restatement_processes_what_the_model_claims(which, request):
    cells, rounds, ora = request.getfixturevalue(which)
    assert ora.outside_updates() == sum(c for _, c in rounds)
    assert ora.updates() == len(cells)                      # every cell of the field was reached
    r = ora.read_cells(np.array([x + S * y for x, y in cells], np.int32))
    assert (r["drivable"] == 1).all() and (r["pending"] == 0).all() and (r["updated"] == 0).all()
    assert (r["n_clusters"] == 1).all() and (r["clusters"][:, 0, 4] == 3.0).all()


def consumed_order_cell(reverse):
    ora = MO.OracleMls(SC.GROW_S, SC.GROW_S, 1.0, SC.params(**SC.GROW))
    ora.add_cloud(SC.carried_cloud(reverse), (0.0, 0.0))
    c = np.array([SC.ORDER_CELL[0] + SC.GROW_S * SC.ORDER_CELL[1]], np.int32)
    r = ora.read_cells(c)
    assert (r["updated"][0], r["pending"][0], r["n_clusters"][0]) == (1, len(SC.ORDER_Z), 0)   # carried, untouched
    assert ora.read_cells(np.arange(ora.cells, dtype=np.int32), clusters=False)["pending"].sum() == 304
    ora.add_cloud(np.zeros((0, 3), np.float32), SC.CARRIED_POSE)
    r = ora.read_cells(c)
    assert (r["updated"][0], r["pending"][0]) == (0, 0) and r["drivable"][0] != -1             # consumed
    return r["clusters"][0]


def test_the_order_cell_is_order_sensitive():
    """the carried points of ORDER_CELL replayed in reverse give a cluster of other bits: a store that permutes the
    carried points of that cell cannot pass the device comparison that follows their consumption"""
    a, b = consumed_order_cell(False), consumed_order_cell(True)
    assert (a.view(np.uint64) != b.view(np.uint64)).any(), (a, b)


def test_mostly_dropped_cloud_counts():
    n = 2 ** 20
    cloud = SC.mostly_dropped_cloud(n, 1)
    ora = MO.OracleMls(SC.GROW_S, SC.GROW_S, 1.0, SC.params(**SC.GROW))
    ora.add_cloud(cloud, (0.0, 0.0))
    live = 36 * 28
    assert len(cloud) == n and ora.updates() == live and ora.outside_updates() == 0
    assert ora.read_cells(np.arange(ora.cells, dtype=np.int32), clusters=False)["pending"].sum() == 0
    assert np.isfinite(cloud[-1]).all()                     # the last of the n points is a live one


def test_tall_cell_has_more_than_sixteen_clusters():
    ora = MO.OracleMls(20, 20, 1.0, SC.params(max_clusters=40))
    for part in (0, 1):
        ora.add_cloud(SC.tall_cell_cloud(20, 3, 3, part), (0.0, 0.0))
        r = ora.read_cells([3 + 20 * 3])
        z = r["clusters"][0, :20, 2]
        assert r["n_clusters"][0] == 20 and (np.abs(np.diff(z) - 2.0) < 1e-9).all(), z
    assert r["pending"][0] == len(SC.tall_cell_cloud(20, 3, 3, 0)) + len(SC.tall_cell_cloud(20, 3, 3, 1))
