"""Each case of tests/grid_raycast_cases.py is shown to reach the edge it is built for, with the oracle alone -- no GPU.  A case
that drifts off its edge after a later edit of its builder fails here, not silently in tests/test_gpu_grid_raycast_edges.py."""
import numpy as np

import grid_raycast_cases as RC
import oracle_lib as O


def params(c):
    return O.grid_params(c.size_x, c.size_y, c.res, c.kwargs.get("max_range", 75.0), 1.0, 0.3, 0, c.kwargs["rolling"])


def updates_per_beam(c, idx=None):
    """cell updates of each beam alone (0: dropped; du + 1 otherwise), the planes shared"""
    g, h, m = params(c), np.zeros(c.size_x * c.size_y, np.int32), np.zeros(c.size_x * c.size_y, np.int32)
    idx = range(len(c.end)) if idx is None else idx
    return np.array([O.grid_raycast(g, c.origin[i:i + 1], c.end[i:i + 1], h, m)[2] for i in idx])


def test_counter_carry_passes_16_bits_in_one_tile():
    c = RC.counter_carry()
    assert (c.size_x, c.size_y) == (RC.TILE, RC.TILE) and len(c.end) == 1100 * RC.BLOCK > 1023 * RC.BLOCK
    h, m, _ = O.grid_raycast(params(c), c.origin, c.end)
    sensor, end = (x + c.size_x * y for x, y in (RC.CARRY_SENSOR, RC.CARRY_END))
    assert m[sensor] > 65535 and h[end] > 65535 and sensor != end
    assert h[sensor] > 0 and m[sensor] > 0                       # both halves of one packed word in use
    # ... and one full visit (1023 blocks) stays just inside 16 bits in both halves: nothing but the forced write-back does
    k = 1023 * RC.BLOCK
    h1, m1, _ = O.grid_raycast(params(c), c.origin[:k], c.end[:k])
    assert m1[sensor] == h1[end] == k == 65472
    for wg, seg in ((1, 8), (0, 511)):
        v = RC.counter_carry(wg, seg)
        assert v.kwargs["raycast_max_workgroups"] == wg and v.kwargs["raycast_seg_items"] == seg
        assert np.array_equal(v.end, c.end) and np.array_equal(v.origin, c.origin)


def test_short_and_staggered_lengths():
    for max_len, dropped in ((63, False), (12, False), (63, True)):
        c = RC.short_and_staggered(max_len, dropped)
        n = updates_per_beam(c).reshape(len(RC.STAGGER_DIRS), RC.BLOCK)
        want = np.tile(np.arange(RC.BLOCK) % (max_len + 1) + 1, (len(RC.STAGGER_DIRS), 1))   # lane j: j steps and the end cell
        if dropped:
            want[:, list(RC.STAGGER_DROPPED_LANES)] = 0
        assert np.array_equal(n, want)
    assert len(RC.STAGGER_DIRS) == 16 and len(set(RC.STAGGER_DIRS)) == 16


def test_merge_runs_blocks():
    c = RC.merge_runs()
    n = updates_per_beam(c).reshape(-1, RC.BLOCK)
    same = lambda b, lanes: len({(tuple(c.origin[b * 64 + j]), tuple(c.end[b * 64 + j])) for j in lanes}) == 1
    assert same(0, range(64)) and (n[0] > 1).all()                                   # 64 identical beams
    assert same(1, range(63)) and not same(1, (62, 63)) and same(2, range(1, 64)) and not same(2, (0, 1))
    assert n[3, 20] == 0 and (np.delete(n[3], 20) > 0).all()                         # an idle lane inside a run
    assert n[4, 25] == 0 and same(4, [j for j in range(10, 41) if j != 25])
    for k, r in enumerate((2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 63)):                     # runs of r that end at lane 63
        assert same(5 + k, range(64 - r, 64)) and not same(5 + k, (63 - r, 64 - r))
    assert (n[-6:] == 0).sum() == 3                                                  # one dropped lane in each of the last kind


def test_tile_corner_touches_a_tile_in_one_cell():
    c = RC.tile_corner()
    g, cells = params(c), c.size_x * c.size_y
    in_tile_11 = np.zeros((c.size_y, c.size_x), bool)
    in_tile_11[RC.TILE:2 * RC.TILE, RC.TILE:2 * RC.TILE] = True
    n_patch = len(RC.CORNER_PATCH) ** 4
    assert n_patch == 1296
    one_cell = one_cell_miss = 0
    for i in range(RC.CORNER_FIRST_PAIR, RC.CORNER_FIRST_PAIR + n_patch):
        h, m, n = O.grid_raycast(g, c.origin[i:i + 1], c.end[i:i + 1], np.zeros(cells, np.int32), np.zeros(cells, np.int32))
        inside = int((h + m)[in_tile_11.ravel()].sum())
        one_cell += inside == 1 and n > 1
        one_cell_miss += inside == 1 and n > 1 and int(m[in_tile_11.ravel()].sum()) == 1    # ... passing through, not ending there
    assert one_cell > 0 and one_cell_miss > 0
    n = updates_per_beam(c)
    assert (n > 0).all() and n.max() == 300                                          # border rows, corners: the whole side
    # whole blocks whose bounding box begins in the last column or row of a tile
    cells = np.array([O.grid_cell(g, *p)[1:] for p in np.concatenate([c.origin[:RC.CORNER_FIRST_PAIR], c.end[:RC.CORNER_FIRST_PAIR]], 1).reshape(-1, 2)])
    cells = cells.reshape(4, RC.BLOCK * 2, 2)
    assert [int(b[:, k].min()) for b, k in zip(cells, (0, 1, 0, 1))] == [127, 127, 299, 299]


def test_long_thin_reaches_the_largest_grid():
    for tall in (False, True):
        c = RC.long_thin(tall)
        assert sorted((c.size_x, c.size_y)) == [513, 32767]
        tiles = -(-c.size_x // RC.TILE) * -(-c.size_y // RC.TILE)
        assert 1024 < tiles == 1280 <= 2048                                          # two trips of the in-LDS prefix
        g = params(c)
        kept = np.array([O.grid_cell(g, *e)[0] >= 0 for e in c.end])                 # (origins are inside by construction)
        assert kept.all()
        du = updates_per_beam(c) - 1
        assert du.min() > 0 and du.max() == 32766 and set(du) == set(RC.LONG_DU)
        # the distance along the thin axis, from the oracle's cells of both ends (in the tall grid an origin's y may pass size_x,
        # which ogrid_cell refuses for a point: there the wide grid bins (y, x))
        wide = O.grid_params(32767, 513, 1.0, 1e9)
        thin_cell = (lambda p: O.grid_cell(wide, p[1], p[0])[2]) if tall else (lambda p: O.grid_cell(wide, p[0], p[1])[2])
        dv = {abs(thin_cell(o) - thin_cell(e)) for o, e in zip(c.origin, c.end)}
        assert dv == set(RC.LONG_DV)
        assert 1000 < len(c.end) < 2500


def test_pre_pass_every_drop_reason_drops_and_keeps_its_neighbour():
    for wide in (False, True):
        for rolling in (0, 1):
            c, marks = RC.pre_pass(wide, rolling), RC.pre_pass_marks(wide, rolling)
            assert (c.size_x, c.size_y) == ((257, 131) if wide else (131, 257))
            n = updates_per_beam(c)
            for reason, bad, ok in marks:
                assert n[bad] == 0 and n[ok] > 0, (wide, rolling, reason, n[bad], n[ok])
            reasons = {r for r, _, _ in marks}
            assert len(reasons) == (9 if not wide else 7) + 20
            # the beams off the axis at the gate: seven neighbouring floats each, some inside and some beyond
            gate = n[3:3 + 4 * 7].reshape(4, 7)
            assert ((gate > 0).any(axis=1) & (gate == 0).any(axis=1)).all(), gate
            assert n[2] > 0                                                           # one float inside the gate
            # cell coordinates in (-1, 0) are cell 0, not cell -1
            g = params(c)
            zero = [O.grid_cell(g, *e) for e in c.end]
            assert any(k >= 0 and x == 0 for k, x, y in zero) and any(k >= 0 and y == 0 for k, x, y in zero)


def test_ragged_counts_sizes():
    assert RC.RAGGED_N == (1, 63, 64, 65, 1023, 1024, 1025) and len(RC.ragged_prior().end) == 5000
    for n in RC.RAGGED_N:
        c = RC.ragged_counts(n)
        assert len(c.end) == n and (c.size_x, c.size_y) == (300, 300) and (updates_per_beam(c) > 0).all()


def test_many_blocks_keeps_beams_in_the_named_blocks_only():
    c = RC.many_blocks()
    assert len(c.end) == 4099 * RC.BLOCK == 262336
    g, h, m = params(c), np.zeros(90000, np.int32), np.zeros(90000, np.int32)
    per_block = [O.grid_raycast(g, c.origin[b * 64:b * 64 + 64], c.end[b * 64:b * 64 + 64], h, m)[2] for b in range(4099)]
    assert tuple(np.flatnonzero(per_block)) == RC.MANY_KEPT_BLOCKS == (0, 1023, 1024, 4095, 4096, 4098)
    # blocks of the first trip of the work-list kernel (below 4096) and of its second share tiles
    tiles = lambda b: set(((np.flatnonzero(O.grid_raycast(g, c.origin[b * 64:b * 64 + 64], c.end[b * 64:b * 64 + 64])[1]) // 300) // 128) * 3 +
                          ((np.flatnonzero(O.grid_raycast(g, c.origin[b * 64:b * 64 + 64], c.end[b * 64:b * 64 + 64])[1]) % 300) // 128))
    assert tiles(0) & tiles(4096) and tiles(4095) & tiles(4098)


def test_scans_rolling_is_what_it_says():
    s = RC.scans_rolling_inputs()
    c = RC.scans_rolling(O.transform_points)
    sizes = np.diff(s.scan_off)
    assert len(sizes) == 3 and (sizes == 0).sum() == 1 and np.isnan(s.pts).any(axis=1).sum() == 1
    n = updates_per_beam(c)
    assert (n == 0).sum() == 1 and len(n) == sizes.sum()                             # everything but the NaN point is kept
    # the moves are no whole numbers of cells, and leave the seam inside a tile on both axes
    x = y = 0.0
    ox = oy = 0
    for px, py in s.poses:
        dx, dy = (px - x) / c.res, (py - y) / c.res
        assert abs(dx - round(dx)) > 0.05 and abs(dy - round(dy)) > 0.05
        ox, oy = (ox + round(dx)) % c.size_x, (oy + round(dy)) % c.size_y
        x, y = x + round(dx) * c.res, y + round(dy) * c.res
    assert (c.size_x - ox) % RC.TILE not in (0,) and (c.size_y - oy) % RC.TILE != 0 and ox and oy
    # rows on both sides of the seam hold counts
    h, m, _ = O.grid_raycast(params(c), c.origin, c.end)
    rows = np.flatnonzero((h + m).reshape(c.size_y, c.size_x).any(axis=1))
    assert rows.min() < c.size_y - oy <= rows.max()
