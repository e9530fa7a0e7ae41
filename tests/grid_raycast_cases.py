"""The raycast's edges, as data: beams built on purpose for the places where the tiled raycast's arithmetic is tight
(slam_amd/csrc/grid_raycast.hpp, grid_clip.hpp), each case the smallest that reaches its edge.  A builder returns a Case
(size_x, size_y, res, grid kwargs, origin f32 [n, 2], end f32 [n, 2]); tests/test_grid_raycast_cases.py shows with the oracle alone
that each case reaches its edge, tests/test_gpu_grid_raycast_edges.py holds the three device forms to the oracle's sequential
Bresenham on every one.  docs/GRID_RAYCAST.md has the table of edges.

Beams are written in window cells and turned into the centres of those cells (cell = trunc(v / res + size // 2), res = 1: exact
in float32 up to the largest grid), except in pre_pass, which is about the conversion itself."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "size_x size_y res kwargs origin end")

BLOCK = 64            # beams per culling block = one wavefront (kBlock)
TILE = 128            # cells per tile side (kTile)
NAN = float("nan")
PLAIN = dict(rolling=0, max_range=1e9, min_cluster_points=0)      # no range gate, window = map frame


def centres(cells, sx, sy, res=1.0):
    """float32 centres of window cells [n, 2]"""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    return ((c - [sx // 2, sy // 2] + 0.5) * res).astype(np.float32)


def from_cells(sx, sy, beams, dropped=(), kwargs=PLAIN):
    """beams: [n, 4] integer (x0, y0, x1, y1) window cells; dropped: indices whose end becomes NaN (make_beam drops them)"""
    b = np.asarray(beams, np.int64).reshape(-1, 4)
    origin, end = centres(b[:, :2], sx, sy), centres(b[:, 2:], sx, sy)
    end[np.asarray(dropped, np.int64)] = NAN
    return Case(sx, sy, 1.0, dict(kwargs), origin, end)


# ---------------------------------------------------------------------------------------------------------------- counter_carry
CARRY_SENSOR, CARRY_END = (40, 64), (75, 80)
CARRY_BEAMS = 1100 * BLOCK


def counter_carry(max_workgroups=0, seg_items=0):
    """kMaxAccBlocks: a tile cell is hits << 16 | misses in LDS, and only the forced write-back after 1023 blocks keeps 64 * 1023
    adds from carrying.  1100 blocks in ONE tile: the first 66 000 beams are the same beam sensor -> CARRY_END (a full visit of
    1023 blocks puts 65 472 misses into the sensor's cell and 65 472 hits into the end's), 4 100 more leave the sensor for ends
    a few tens of cells away, 300 zero-length beams put hits into the sensor's cell."""
    sx = sy = 128
    rs = np.random.RandomState(70400)
    n_same, n_zero = 66000, 300
    n_fan = CARRY_BEAMS - n_same - n_zero
    b = np.empty((CARRY_BEAMS, 4), np.int64)
    b[:, 0], b[:, 1] = CARRY_SENSOR
    b[:n_same, 2:] = CARRY_END
    b[n_same:n_same + n_fan, 2] = CARRY_SENSOR[0] + rs.randint(-38, 60, n_fan)
    b[n_same:n_same + n_fan, 3] = CARRY_SENSOR[1] + rs.randint(-60, 60, n_fan)
    b[n_same + n_fan:, 2:] = CARRY_SENSOR
    return from_cells(sx, sy, b, kwargs=dict(PLAIN, raycast_max_workgroups=max_workgroups, raycast_seg_items=seg_items))


# ---------------------------------------------------------------------------------------------------------- short_and_staggered
# the four axis directions, the eight octants (major step 1, minor 5/8) and the four diagonals (dx == dy: x counts as major)
STAGGER_DIRS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)] + \
               [(sx, sy, xm) for xm in (1, 2) for sx in (1, -1) for sy in (1, -1)] + [(sx, sy, 3) for sx in (1, -1) for sy in (1, -1)]
STAGGER_DROPPED_LANES = (7, 8, 31, 63)


def short_and_staggered(max_len=63, dropped=False):
    """the walk's short ends: lane j takes j % 8 single steps before the lock-step trips of four and the three remainder steps.
    One origin per block, lane j's beam has length j % (max_len + 1) -- lengths 0, 1, 2, ... in neighbouring lanes, shorter than
    the stagger, shorter than a trip -- in every direction; `dropped` drops lanes in the middle of each block."""
    sx = sy = 300
    beams, drop = [], []
    for bi, (ux, uy, kind) in enumerate(STAGGER_DIRS):
        x0, y0 = 100 + (bi * 7) % 50, 100 + (bi * 11) % 50          # around the corner of the four tiles
        for j in range(BLOCK):
            ln = j % (max_len + 1)
            mn = (5 * ln) // 8
            d = {0: (ux * ln, uy * ln), 1: (ux * ln, uy * mn), 2: (ux * mn, uy * ln), 3: (ux * ln, uy * ln)}[kind]
            if dropped and j in STAGGER_DROPPED_LANES:
                drop.append(len(beams))
            beams.append((x0, y0, x0 + d[0], y0 + d[1]))
    return from_cells(sx, sy, beams, drop)


# ------------------------------------------------------------------------------------------------------------------- merge_runs
def merge_runs():
    """add_miss of the MERGE form: lanes on one cell are a run, its first lane adds its length (wave_shr:1, lead | ~on,
    64 - lane).  Runs that reach lane 63, runs broken by an idle lane, 64 identical beams, runs of 2, 3, ... ending at lane 63,
    neighbours that share their first cells and then part -- and beams set back by j % 8 cells along one line, so that after
    the stagger all 64 lanes stand on ONE cell in every lock-step trip."""
    sx = sy = 300
    same, other = (20, 30, 90, 50), (20, 30, 90, 90)
    blocks, drop = [], []

    def add(block, dropped=()):
        assert len(block) == BLOCK
        drop.extend(len(blocks) * BLOCK + j for j in dropped)
        blocks.append(block)

    fan = lambda j: (150, 150, 250, 100 + j)                                    # distinct beams that share their first cells
    add([same] * 64)                                                            # 64 identical beams
    add([same] * 63 + [other])                                                  # lanes 0-62 share a beam, lane 63 differs
    add([(25, 200, 100, 210)] + [same] * 63)                                    # ... and the other way round
    add([same] * 64, dropped=[20])                                              # a run with a dropped lane in its middle
    add([same if 10 <= j <= 40 else fan(j) for j in range(64)], dropped=[25])
    for r in (2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 63):                              # runs of r ending at lane 63
        add([fan(j) if j < 64 - r else (150, 150, 260, 170) for j in range(64)])
    add([(140, 20, 280, 20 + j) for j in range(64)])                            # share the first k cells, then part
    add([(140, 120, 280, 183 - j) for j in range(64)])                          # (across the tiles' border, lanes the other way)
    add([(120, 140, 120 + j // 2, 280) for j in range(64)])                     # (pairs of equal beams, y-major)
    for line in (lambda s: (60 - s, 200, 200, 200), lambda s: (200, 260 + s, 200, 60), lambda s: (60 - s, 60 - s, 250, 250)):
        block = [line(j % 8) for j in range(64)]
        add(block)                                                              # one cell for all 64 lanes in every trip
        short = list(block)
        x0, y0, x1, y1 = block[40]
        short[40] = (x0, y0, x0 + 5 * np.sign(x1 - x0), y0 + 5 * np.sign(y1 - y0))  # ... a lane that is done early: idle in the trips
        x0, y0, x1, y1 = block[63]
        short[63] = (x0, y0, x0 + 9 * np.sign(x1 - x0), y0 + 9 * np.sign(y1 - y0))
        add(short, dropped=[31])
    return from_cells(sx, sy, np.array(blocks).reshape(-1, 4), drop)


# ------------------------------------------------------------------------------------------------------------------ tile_corner
CORNER_PATCH = range(125, 131)                    # the 6 x 6 cells around the corner (127..128, 127..128) of the four tiles
CORNER_FIRST_PAIR = 4 * BLOCK                     # where the pairs of patch cells begin in the case


def tile_corner():
    """the exact clip (grid_clip.hpp: i_lo / i_hi, the start error e): beams that touch a tile in one corner cell, run along a
    tile's border row or column, or are exact diagonals through tile corners, and the partial tiles' last row and column."""
    sx = sy = 300
    # whole blocks whose bounding box BEGINS in a tile's last column or row (box_overlaps_tile: cb.x <= tx1, cb.y <= ty1), the
    # partial tiles' among them
    beams = [(127, 100 + j, 127 + j, 140) for j in range(BLOCK)] + [(100 + j, 127, 140, 127 + j) for j in range(BLOCK)]
    beams += [(299, 100 + j, 299, 290 - j) for j in range(BLOCK)] + [(100 + j, 299, 290 - j, 299) for j in range(BLOCK)]
    assert len(beams) == CORNER_FIRST_PAIR
    patch = [(x, y) for y in CORNER_PATCH for x in CORNER_PATCH]
    beams += [p + q for p in patch for q in patch]                               # every ordered pair: 1 296 beams
    th = 2 * np.pi * (np.arange(64) + 0.5) / 64
    ring = [(int(np.floor(128 + 100 * np.cos(a))), int(np.floor(128 + 100 * np.sin(a)))) for a in th]
    beams += [p + q for p in patch for q in ring] + [q + p for p in patch for q in ring]
    for k in (127, 128, 299):                                                    # border rows and columns, both ways
        beams += [(0, k, 299, k), (299, k, 0, k), (k, 0, k, 299), (k, 299, k, 0)]
    corners = [(0, 0), (299, 0), (0, 299), (299, 299)]
    mids = [(150, 0), (0, 150), (299, 150), (150, 299)]
    beams += [p + q for p in corners for q in corners + mids if p != q]
    return from_cells(sx, sy, beams)


# -------------------------------------------------------------------------------------------------------------------- long_thin
LONG_DU = (32766, 32765, 16384, 16383)
LONG_DV = (0, 1, 2, 255, 256, 511, 512)


def long_thin(tall=False):
    """the clip at the largest grid slam_grid_create admits: __mul24(den, k_hi + 1) up to 65 532 * 513, quotients of
    floor_div_small near 2^15, coordinates at 32 766 -- and 1 280 tiles, the two-trip prefix of scan_tile_counts in LDS.
    Wide (32767 x 513): every sign pair, from the grid's ends, the minor axis placed from corner to corner.  Tall (513 x 32767):
    an end cell with y >= size_x is dropped (point_cell's quirk), so the beams run down to rows below 513."""
    long_, thin = 32767, 513
    beams = []
    for du in LONG_DU:
        for dv in LONG_DV:
            for sv in (1, -1):
                v_lo = 0 if sv > 0 else dv
                starts = sorted(set(int(v) for v in np.linspace(v_lo, v_lo + thin - 1 - dv, 20)))
                if not tall:
                    for su in (1, -1):
                        u0 = 0 if su > 0 else long_ - 1
                        beams += [(u0, v0, u0 + su * du, v0 + sv * dv) for v0 in starts]
                else:
                    for u1 in (0, 1, 127, 128, 511, 512):
                        if u1 + du <= long_ - 1:
                            beams += [(v0, u1 + du, v0 + sv * dv, u1) for v0 in starts[::3]]
    sx, sy = (thin, long_) if tall else (long_, thin)
    return from_cells(sx, sy, beams)


# --------------------------------------------------------------------------------------------------------------------- pre_pass
PRE_RES = 0.25
PRE_RANGE = 32.125     # (0, -32.125) is AT the gate and its cell coordinate -32.125 / 0.25 + 128 = -0.5 truncates to cell 0


def _pre_pass(wide, rolling):
    """-> Case, marks: (reason, index of a beam the pre-pass must drop, index of its nearest neighbour, which it must keep)"""
    sx, sy = (257, 131) if wide else (131, 257)
    f32 = np.float32
    up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))
    # the long axis l (half = 128) and the short one s (half = 65); a point is (l, s) here and put in (x, y) order at the end
    O, E, marks = [], [], []
    origin0 = (f32(1.3), f32(-2.1))

    def beam(o, e):
        O.append(o), E.append(e)
        return len(O) - 1

    def pair(reason, o_bad, e_bad, o_ok, e_ok):
        marks.append((reason, beam(o_bad, e_bad), beam(o_ok, e_ok)))

    gate = f32(-PRE_RANGE)
    # the range gate: AT it (kept), one float beyond (dropped), one float inside (kept); on the axis the sums are exact
    pair("range gate, on the axis", origin0, (down(gate), f32(0)), origin0, (gate, f32(0)))
    beam(origin0, (up(gate), f32(0)))
    for s in (-12.0, -5.5, 3.25, 9.0):      # off the axis: float sqrt (rolling) and double sqrt (not) round their own way
        l = f32(-np.sqrt(PRE_RANGE ** 2 - s ** 2))
        near = [l]
        for _ in range(3):
            near = [down(near[0])] + near + [up(near[-1])]
        for v in near:
            beam(origin0, (v, f32(s)))
    # cell coordinates in (-1, 0) truncate to cell 0: kept, for ends and for origins, on both axes
    in_l, in_s = f32(-128.5 * PRE_RES), f32(-65.75 * PRE_RES)
    pair("end beyond the low side of the short axis", origin0, (f32(-3.0), f32(-66.0 * PRE_RES)), origin0, (f32(-3.0), in_s))
    pair("origin one cell outside, low side of the short axis", (f32(3.0), f32(-66.0 * PRE_RES)), (f32(-1.0), f32(1.0)), (f32(3.0), in_s),
         (f32(-1.0), f32(1.0)))
    pair("origin one cell outside, low side of the long axis", (f32(-129.0 * PRE_RES), f32(0.5)), (f32(-1.0), f32(1.0)), (in_l, f32(0.5)),
         (f32(-1.0), f32(1.0)))
    beam(origin0, (in_l, f32(0.5)))                                               # end in (-1, 0) of the long axis, inside the gate
    hi_l, hi_s = f32((257 - 128) * PRE_RES), f32((131 - 65) * PRE_RES)          # the first coordinate of cell `size`
    pair("origin one cell outside, high side of the long axis", (hi_l, f32(0.5)), (f32(-1.0), f32(1.0)), (down(hi_l), f32(0.5)),
         (f32(-1.0), f32(1.0)))
    pair("origin one cell outside, high side of the short axis", (f32(0.5), hi_s), (f32(-1.0), f32(1.0)), (f32(0.5), down(hi_s)),
         (f32(-1.0), f32(1.0)))
    pair("end beyond the high side of the short axis", origin0, (f32(0.5), hi_s), origin0, (f32(0.5), down(hi_s)))
    if not wide:
        # y is the long axis and is tested against size_x: end rows 131 .. 256 are dropped, row 130 is kept; origins are not
        row131 = f32((131 - 128) * PRE_RES)
        pair("end with its y cell in [size_x, size_y)", origin0, (row131, f32(0.5)), origin0, (down(row131), f32(0.5)))
        pair("end with its y cell in [size_x, size_y) (an origin there is kept)", origin0, (f32(20.0), f32(-3.0)), (f32(20.0), f32(-3.0)),
             (f32(-20.0), f32(-3.0)))
    # NaN, infinities and coordinates no int can hold, in each of the four coordinates in turn
    good = [f32(-7.3), f32(4.1), f32(-9.9), f32(-11.2)]                           # origin (l, s), end (l, s)
    for k, name in enumerate(("origin, long axis", "origin, short axis", "end, long axis", "end, short axis")):
        for bad in (NAN, np.inf, -np.inf, 3e9 * PRE_RES, -3e9 * PRE_RES):
            v = list(good)
            v[k] = f32(bad)
            pair("%s in the %s" % (bad, name), (v[0], v[1]), (v[2], v[3]), (good[0], good[1]), (good[2], good[3]))
    O, E = np.array(O, np.float32), np.array(E, np.float32)
    if not wide:
        O, E = O[:, ::-1].copy(), E[:, ::-1].copy()
    return Case(sx, sy, PRE_RES, dict(rolling=rolling, max_range=PRE_RANGE, min_cluster_points=0), O, E), marks


def pre_pass(wide=False, rolling=0):
    """make_beam for rays: the range gate at, one float inside and one float beyond it, the `y >= size_x` quirk of a grid with
    size_x < size_y (ends only: origins are tested against size_y), truncation toward zero of coordinates in (-1, 0), NaN /
    infinite / beyond-int coordinates in each of the four places, origins one cell outside each side."""
    return _pre_pass(wide, rolling)[0]


def pre_pass_marks(wide=False, rolling=0):
    return _pre_pass(wide, rolling)[1]


# ---------------------------------------------------------------------------------------------------------------- ragged_counts
RAGGED_N = (1, 63, 64, 65, 1023, 1024, 1025)


def _random_beams(seed, n, sx, sy):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, sx, n), rs.randint(0, sy, n), rs.randint(0, sx, n), rs.randint(0, sy, n)], 1)


def ragged_prior():
    """the 5 000 other beams a ragged_counts handle has raycast just before: what lies behind n in its scratch"""
    return from_cells(300, 300, _random_beams(5000, 5000, 300, 300))


def ragged_counts(n):
    """the partial last block: `bi < n` in grab and the in_range store of store_beam_and_box, with live stale beams behind n"""
    return from_cells(300, 300, _random_beams(n, n, 300, 300))


# ----------------------------------------------------------------------------------------------------------------- many_blocks
MANY_BLOCKS = 4099
MANY_KEPT_BLOCKS = (0, 1023, 1024, 4095, 4096, 4098)


def many_blocks():
    """the work list past 4 096 blocks: the second trip of tile_items_wg_kernel (s_base += total) and the last, partial, group
    of 1 024 boxes.  Everything dropped but a handful of beams in the first and last block of each trip."""
    sx = sy = 300
    n = MANY_BLOCKS * BLOCK
    b = np.zeros((n, 4), np.int64)
    kept = []
    for k, blk in enumerate(MANY_KEPT_BLOCKS):
        for lane, beam in ((0, (5 + k, 7, 290, 280 - 9 * k)), (17, (150 + k, 150, 150 + k, 150)), (63, (299, 20 * k, 0, 299 - 31 * k)),
                           (40, (130 - k, 295, 127, 3 + k))):
            b[blk * BLOCK + lane] = beam
            kept.append(blk * BLOCK + lane)
    return from_cells(sx, sy, b, np.setdiff1d(np.arange(n), kept))


# --------------------------------------------------------------------------------------------------------------- scans_rolling
ScanInputs = namedtuple("ScanInputs", "poses pts scan_off R t")


def _scans_rolling():
    sx = sy = 300
    res = 0.25
    # set_pose rounds the move to whole cells: (3.3, -1.9) -> 13 and -8 cells, pose (3.25, -2.0); then 117 and -132 cells more:
    # origin (130, 160), the seam at window column 170 and row 140 -- inside the tiles, and in the middle of the scans
    poses = [(3.3, -1.9), (3.25 + 117 * res + 0.1, -2.0 - 132 * res - 0.1)]
    final = (3.25 + 117 * res, -2.0 - 132 * res)
    rs = np.random.RandomState(3)
    sizes = [700, 0, 500]
    # everything dyadic, so that R p + t - pose is exact in double however it is associated
    pts = rs.randint(-96, 97, (sum(sizes), 2)) / 8.0
    pts[123] = NAN
    scan_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R = np.array([[1.0, 0.0, 0.0, 1.0], [0.5, -0.75, 0.75, 0.5], [0.0, -1.0, 1.0, 0.0]])
    t = np.array([[final[0] + 2.125, final[1] - 3.5], [0.0, 0.0], [final[0] - 6.375, final[1] + 4.625]])
    return sx, sy, res, dict(rolling=1, min_cluster_points=0), final, ScanInputs(poses, pts, scan_off, R, t)


def scans_rolling_inputs():
    """what the device is given: the poses the grid is moved to, then the scans (points, offsets, one R and t per scan)"""
    return _scans_rolling()[5]


def scans_rolling(transform_points):
    """slam_grid_raycast_scans_dev on a rolled window: points relative to the pose, the toroidal seam inside a tile (flush's
    storage rows, the global form's `wraps` rule), an empty scan, a NaN point.  The Case holds the rays the scans amount to:
    end = transform_points(points, R, t - pose) (the oracle's own), origin = (float)(t - pose)."""
    sx, sy, res, kw, final, s = _scans_rolling()
    origin, end = [], []
    for k in range(len(s.scan_off) - 1):
        a, b = s.scan_off[k], s.scan_off[k + 1]
        rel = s.t[k] - np.array(final)
        end.append(transform_points(s.pts[a:b], s.R[k], rel).reshape(-1, 2))
        origin.append(np.tile(rel.astype(np.float32), (b - a, 1)))
    return Case(sx, sy, res, kw, np.concatenate(origin), np.concatenate(end))


# every device case: id -> builder (called without arguments)
CASES = {
    "counter_carry-wg1-seg8": lambda: counter_carry(1, 8),
    "counter_carry-wg1-seg16": lambda: counter_carry(1, 16),
    "counter_carry-wg1-seg511": lambda: counter_carry(1, 511),
    "counter_carry-seg8": lambda: counter_carry(0, 8),
    "counter_carry-seg16": lambda: counter_carry(0, 16),
    "counter_carry-seg511": lambda: counter_carry(0, 511),
    "short_and_staggered-0to63": lambda: short_and_staggered(63),
    "short_and_staggered-0to12": lambda: short_and_staggered(12),
    "short_and_staggered-dropped_lanes": lambda: short_and_staggered(63, dropped=True),
    "merge_runs": merge_runs,
    "tile_corner": tile_corner,
    "long_thin-32767x513": lambda: long_thin(False),
    "long_thin-513x32767": lambda: long_thin(True),
    "pre_pass-131x257": lambda: pre_pass(False, 0),
    "pre_pass-131x257-rolling": lambda: pre_pass(False, 1),
    "pre_pass-257x131": lambda: pre_pass(True, 0),
    "pre_pass-257x131-rolling": lambda: pre_pass(True, 1),
    "many_blocks": many_blocks,
}
