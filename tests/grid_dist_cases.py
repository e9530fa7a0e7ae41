"""The definition of the occupancy grid's distance field and costmap (docs/GRID_DIST.md, slam_gdist_*) restated in numpy, and the
planes it is checked on.  No GPU, no library.

Planes are flat, window order: data[x + sx * y], int8 in {-1 unknown, 0 free, 100 obstacle}.

  brute(occ, sx, sy, R, unknown_is_obstacle)     the definition itself: the minimum over every obstacle cell, directly
  two_pass(occ, sx, sy, R, unknown_is_obstacle)  independently: the distance along the row first, then the minimum over the column
  cost_of(dist2, occ, T, params)                 the table look-up and the unknown rule

TILE_H is the height of the device's column tile (kTileH in slam_amd/csrc/grid_dist.hip): the planes of 700 and TILE_H + 2 * 254 + 3
rows reach an interior tile with both halos inside the plane, the halos that stick out above and below, and a ragged last tile.
"""
import functools

import numpy as np

FAR = 0xFFFF
TILE_H = 128
UNKNOWN, FREE, OBSTACLE = -1, 0, 100


def obstacle_mask(occ, unknown_is_obstacle):
    occ = np.asarray(occ, np.int8)
    m = occ == OBSTACLE
    if unknown_is_obstacle:
        m |= occ == UNKNOWN
    return m


def brute(occ, sx, sy, R, unknown_is_obstacle=0, chunk=1 << 22):
    m = obstacle_mask(occ, unknown_is_obstacle).reshape(sy, sx)
    oy, ox = np.nonzero(m)
    out = np.full(sx * sy, FAR, np.uint16)
    if len(ox) == 0:
        return out
    ox, oy = ox.astype(np.int64), oy.astype(np.int64)
    cells = np.arange(sx * sy, dtype=np.int64)
    step = max(1, chunk // len(ox))
    for a in range(0, sx * sy, step):
        c = cells[a:a + step]
        x, y = c % sx, c // sx
        d = ((x[:, None] - ox[None, :]) ** 2 + (y[:, None] - oy[None, :]) ** 2).min(axis=1)
        out[a:a + step] = np.where(d <= R * R, d, FAR).astype(np.uint16)
    return out


def row_distance(m, R):
    """g[y, x] = min |x - x'| over the obstacles of row y, capped at R + 1"""
    sy, sx = m.shape
    g = np.full((sy, sx), R + 1, np.int64)
    xs = np.arange(sx)
    for y in range(sy):
        pos = np.nonzero(m[y])[0]
        if len(pos) == 0:
            continue
        k = np.searchsorted(pos, xs)
        left = np.where(k > 0, xs - pos[np.maximum(k - 1, 0)], R + 1)
        right = np.where(k < len(pos), pos[np.minimum(k, len(pos) - 1)] - xs, R + 1)
        g[y] = np.minimum(np.minimum(left, right), R + 1)
    return g


def two_pass(occ, sx, sy, R, unknown_is_obstacle=0):
    g = row_distance(obstacle_mask(occ, unknown_is_obstacle).reshape(sy, sx), R)
    g2 = g * g
    pad = np.full((sy + 2 * R, sx), (R + 1) ** 2, np.int64)     # rows above 0 and below sy - 1 enter as R + 1
    pad[R:R + sy] = g2
    best = np.full((sy, sx), R * R + 1, np.int64)
    for dy in range(-R, R + 1):
        best = np.minimum(best, pad[R + dy:R + dy + sy] + dy * dy)
    return np.where(best <= R * R, best, FAR).astype(np.uint16).ravel()


def cost_of(dist2, occ, T, R, unknown_is_obstacle=0, unknown_cost=255, unknown_keep_from=253):
    T = np.asarray(T, np.uint8)
    assert len(T) == R * R + 2
    c = T[np.minimum(np.asarray(dist2, np.int64), R * R + 1)].astype(np.int64)
    if not unknown_is_obstacle:
        unk = np.asarray(occ, np.int8).ravel() == UNKNOWN
        c = np.where(unk & (c < unknown_keep_from), unknown_cost, c)
    return c.astype(np.uint8)


def inflation_table_np(resolution, inscribed, inflation, scaling, R):
    """the table of slam_grid_inflation_table by numpy, and the real-valued curve before truncation (for the ulp band)"""
    k = np.arange(R * R + 2, dtype=np.float64)
    d = np.sqrt(k) * resolution
    real = 252.0 * np.exp(-scaling * (d - inscribed))
    t = np.where(d <= inscribed, 253.0, np.where(d > inflation, 0.0, np.floor(real)))
    t[0], t[R * R + 1] = 254, 0
    real[0], real[R * R + 1] = 0.5, 0.5
    exact = (d <= inscribed) | (d > inflation)
    exact[0] = exact[R * R + 1] = True
    return t.astype(np.uint8), real, exact


# ------------------------------------------------------------------------------------------------------------- the planes
def plane(sx, sy, fill=FREE):
    return np.full(sx * sy, fill, np.int8)


def with_obstacles(sx, sy, cells, fill=FREE):
    p = plane(sx, sy, fill)
    for x, y in cells:
        p[x + sx * y] = OBSTACLE
    return p


def random_plane(sx, sy, density, seed, unknown_share=1.0 / 3):
    rs = np.random.RandomState(seed)
    p = plane(sx, sy)
    p[rs.rand(sx * sy) < unknown_share] = UNKNOWN
    n = max(1, int(round(density * sx * sy)))
    p[rs.choice(sx * sy, n, replace=False)] = OBSTACLE
    return p


def _case(name, sx, sy, R, occ, unk=0):
    return dict(name=name, sx=sx, sy=sy, R=R, unk=unk, occ=occ)


WORD_EDGE_X = (0, 63, 64, 127, 128, 129)
RANDOM_DENSITIES = (0.001, 0.05, 0.5)
RANDOM_R = (1, 7, 32, 254)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for what, v in (("obstacle", OBSTACLE), ("free", FREE), ("unknown", UNKNOWN)):
        for unk in (0, 1):
            out.append(_case("1x1_%s_unk%d" % (what, unk), 1, 1, 5, plane(1, 1, v), unk))
    for R in (32, 254):
        out.append(_case("1x300_R%d" % R, 1, 300, R, random_plane(1, 300, 0.02, 11)))
        out.append(_case("300x1_R%d" % R, 300, 1, R, random_plane(300, 1, 0.02, 12)))
    for sx, sy in ((63, 5), (64, 64), (65, 67)):                      # one word, exactly one word, one cell into the second
        for R in (7, 100):
            out.append(_case("%dx%d_R%d" % (sx, sy, R), sx, sy, R, random_plane(sx, sy, 0.02, sx + R)))
        out.append(_case("%dx%d_last_column" % (sx, sy), sx, sy, 100, with_obstacles(sx, sy, [(sx - 1, 2)])))
    # the nearest obstacle across a word boundary, from both sides: rows ten apart, so at R = 3 each row stands alone
    edge = with_obstacles(130, 70, [(x, 5 + 10 * i) for i, x in enumerate(WORD_EDGE_X)])
    out.append(_case("130x70_word_edges_R3", 130, 70, 3, edge))
    out.append(_case("130x70_word_edges_R254", 130, 70, 254, edge))
    out.append(_case("130x70_word_edges_one_row", 130, 70, 200, with_obstacles(130, 70, [(x, 33) for x in WORD_EDGE_X])))
    # column tiles: interior tile, both halos, ragged last tile
    for sy in (700, TILE_H + 2 * 254 + 3):
        out.append(_case("70x%d_R254" % sy, 70, sy, 254, random_plane(70, sy, 0.0005, sy)))
        out.append(_case("70x%d_R254_top" % sy, 70, sy, 254, with_obstacles(70, sy, [(40, 0)])))
        out.append(_case("70x%d_R254_bottom" % sy, 70, sy, 254, with_obstacles(70, sy, [(66, sy - 1)])))
    out.append(_case("70x700_R32_top", 70, 700, 32, with_obstacles(70, 700, [(3, 0)])))         # the tiles further down skip
    # ... and obstacles in the outermost halo row of a tile: exactly R rows below tile 1's last row and above tile 3's first
    out.append(_case("70x700_R32_tile_edges", 70, 700, 32,
                     with_obstacles(70, 700, [(1, TILE_H - 1), (68, TILE_H), (30, 2 * TILE_H - 1 + 32), (5, 3 * TILE_H - 32)])))
    out.append(_case("70x700_R254_halo_edge", 70, 700, 254, with_obstacles(70, 700, [(9, 2 * TILE_H - 254), (60, 3 * TILE_H - 1 + 254)])))
    # the bound itself around a single obstacle
    out.append(_case("single_R5", 13, 13, 5, with_obstacles(13, 13, [(6, 6)])))
    out.append(_case("single_R1", 5, 5, 1, with_obstacles(5, 5, [(2, 2)])))
    out.append(_case("single_R254", 600, 5, 254, with_obstacles(600, 5, [(300, 2)])))
    out.append(_case("empty", 70, 130, 32, plane(70, 130)))
    out.append(_case("empty_unknown", 70, 130, 32, plane(70, 130, UNKNOWN)))
    out.append(_case("full", 70, 130, 32, plane(70, 130, OBSTACLE)))
    out.append(_case("full_unknown_is_obstacle", 70, 130, 32, plane(70, 130, UNKNOWN), 1))
    # nothing wraps across the window's edge
    out.append(_case("column_x0", 200, 5, 100, with_obstacles(200, 5, [(0, y) for y in range(5)])))
    out.append(_case("row_y0", 5, 200, 100, with_obstacles(5, 200, [(x, 0) for x in range(5)])))
    for di, dens in enumerate(RANDOM_DENSITIES):
        for R in RANDOM_R:
            for unk in (0, 1):
                out.append(_case("random_97x83_d%d_R%d_unk%d" % (di, R, unk), 97, 83, R, random_plane(97, 83, dens, 100 + di), unk))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement of a case, computed once and shared (read-only)"""
    c = case(name)
    d = brute(c["occ"], c["sx"], c["sy"], c["R"], c["unk"])
    d.setflags(write=False)
    return d


RANDOM_CASES = tuple(n for n in (c["name"] for c in cases()) if n.startswith("random_"))
INFLATION = dict(resolution=0.05, inscribed_radius=0.3, inflation_radius=1.2, cost_scaling=3.0)   # fits R = 32 at 0.05 m (1.6 m)


def inflation_for(R):
    """an inflation curve that fits R cells: the default one where R * resolution allows it, else scaled to the cap"""
    p = dict(INFLATION)
    cap = R * p["resolution"]
    if p["inflation_radius"] > cap:
        p["inflation_radius"] = cap
        p["inscribed_radius"] = min(p["inscribed_radius"], cap / 2)
    return p


def random_table(R, seed=5):
    return np.random.RandomState(seed).permutation(np.arange(R * R + 2) % 256).astype(np.uint8)
