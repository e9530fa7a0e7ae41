"""The occupancy grid's touched / changed rows through every operation that moves them, against a four-integer shadow that
restates slam_amd/csrc/grid_rows.hpp (the host check of the same rules: tests/test_grid_rows.py), and every finalize against the
finalize rule over the whole grid: a step that forgets a row leaves a stale cell there."""
import numpy as np
import pytest

import oracle_lib as O
from slam_amd import api

pytestmark = pytest.mark.gpu


def og(grid):
    p = grid.params
    return O.grid_params(grid.size_x, grid.size_y, grid.resolution, p.max_range, p.occupancy_increment, p.occupancy_decrement,
                         p.min_cluster_points, p.rolling, *grid.get_pose())


N = 0x7F7F7F7F                                  # kNoRow


def mark(r, lo, hi):
    return [min(r[0], lo), min(r[1], -hi), r[2], r[3]]


def retire(r):
    return [N, N, min(r[2], r[0]), min(r[3], r[1])]


def fold(r, lo, hi):
    covered = r[0] >= lo and -r[1] <= hi
    return [N if covered else r[0], N if covered else r[1], min(r[2], r[0], lo), min(r[3], r[1], -hi)]


def finalized(r):
    return [r[0], r[1], N, N]


def all_changed(r, sy):
    return [r[0], r[1], 0, -(sy - 1)]


def reported(r):
    return (0, -1) if r[0] > -r[1] else (r[0], -r[1])


def band(rs, sx, sy, row_lo, row_hi, n):
    """n points whose cells (grid_cell.hpp: trunc(p / res + size / 2), res = 1) lie in the window rows row_lo..row_hi"""
    p = np.empty((n, 2), np.float32)
    p[:, 0] = rs.uniform(-(sx // 2) + 1.2, sx - sx // 2 - 1.2, n)
    p[:, 1] = rs.uniform(row_lo + 0.1, row_hi + 0.9, n) - sy // 2
    p[0, 1], p[1, 1] = row_lo + 0.5 - sy // 2, row_hi + 0.5 - sy // 2      # both edges of the band are hit
    return p


@pytest.mark.parametrize("sx,roll", [(64, None), (63, None), (64, (1, 5))],
                         ids=["64x48_quads", "63x48_single_cells", "64x48_rolled_1_5"])
def test_row_ranges_through_every_operation(sx, roll):
    sy = 48
    rs = np.random.RandomState(sx + (7 if roll else 0))
    g = api.Grid(sx, sy, 1.0, min_cluster_points=0, rolling=1 if roll else 0)
    g.enable_accumulator()
    r = [N, N, N, N]

    def same_rows():
        api.synchronize()
        assert g.dirty_rows() == reported(r), (g.dirty_rows(), r)

    def add(row_lo, row_hi):
        """endpoints in the window rows row_lo..row_hi; the storage rows they touch, as the oracle bins them"""
        nonlocal r
        obs, gnd = band(rs, sx, sy, row_lo, row_hi, 300), band(rs, sx, sy, row_lo, row_hi, 400)
        eh, em, _, n = O.grid_add_endpoints(og(g), obs, gnd)
        assert n == 700
        rows = np.flatnonzero((eh | em).reshape(sy, sx).any(axis=1))
        assert rows[0] == row_lo and rows[-1] == row_hi
        srows = (rows + g.info()["origin_y"]) % sy
        g.add_endpoints(obs, gnd)
        r = mark(r, int(srows.min()), int(srows.max()))
        same_rows()
        return eh, em

    def finalize_and_compare(call, after):
        nonlocal r
        hits, misses = g.read_counts()
        num, occ = O.grid_finalize(og(g), hits, misses)
        call()
        r = after(r)
        same_rows()
        assert np.array_equal(g.read_occupancy(), occ)
        assert np.array_equal(g.read_num_pts(), num)
        return occ

    same_rows()
    if roll:
        g.set_pose(float(roll[0]), float(roll[1]))
        assert (g.info()["origin_x"], g.info()["origin_y"]) == roll
        r = all_changed(r, sy)
        same_rows()
    a = (38, 46) if roll else (8, 15)            # rolled: storage rows 43..47 and 0..3, the seam inside the band
    b = (20, 27)
    add(*a)                                                                         # 1
    occ = finalize_and_compare(g.finalize, finalized)                               # 2
    assert (occ == 100).any() and (occ == 0).any()
    g.reset_counts()                                                                # 3
    r = retire(r)
    same_rows()
    assert not g.read_counts()[0].any() and not g.read_counts()[1].any()
    occ = finalize_and_compare(g.finalize, finalized)                               # 4: the band is unknown again
    assert (occ == -1).all()
    eh, em = add(*b)                                                                # 5
    g.mark_rows(40, 41)                                                             # 6
    r = mark(r, 40, 41)
    same_rows()
    lo, hi = reported(r)
    g.fold(lo + 2, lo + 4)                                                          # 7: part of it, touched stays
    r = fold(r, lo + 2, lo + 4)
    assert reported(r) == (lo, hi)
    same_rows()
    g.fold(lo, hi)                                                                  # 8: all of it
    r = fold(r, lo, hi)
    assert reported(r) == (0, -1)
    same_rows()
    folded = g.read_counts()
    assert np.array_equal(folded[0], eh) and np.array_equal(folded[1], em)          # a fold moves counts, it loses none
    g.set_min_cluster_points(1)                                                     # 9
    g.params.min_cluster_points = 1
    r = all_changed(r, sy)
    same_rows()
    reset = lambda q: retire(finalized(q))
    occ = finalize_and_compare(g.finalize_reset, reset)                             # 10: one buffer ...
    assert (occ == 100).any()
    finalize_and_compare(g.finalize_reset, reset)                                   # ... and the other
    assert r == [N, N, N, N]
    add(*a)                                                                         # 11
    finalize_and_compare(g.finalize_reset, reset)                                   # 12
    after = g.read_counts()                                                         # the new counts are gone, the folded ones stay
    assert np.array_equal(after[0], folded[0]) and np.array_equal(after[1], folded[1])
    finalize_and_compare(g.finalize, finalized)                                     # and the rows just reset are due once more
    g.close()
