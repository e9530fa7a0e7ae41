"""The definition of the occupancy grid's navigation field and path (docs/GRID_NAV.md, slam_gnav_*) restated in numpy, and the
planes it is checked on.  No GPU, no library.

Planes are flat, window order: data[x + sx * y], uint8 cost bytes.  S is the step table, uint32[256]: S[c] == 0 closes a cell.

  dijkstra(cost, sx, sy, S, goals, orth_w, diag_w)      a binary heap over Python integers, clamped at the end
  bellman_ford(cost, sx, sy, S, goals, orth_w, diag_w)  independently: whole-plane sweeps, np.minimum over the eight shifted
                                                        planes, until nothing changes
  walk(cost, sx, sy, S, pot, start, max_len, ...)       the path rule: the allowed neighbour of lowest d with
                                                        pot[v] + m(u, v) == pot[u]

TILE is the edge of the device's tile (kTile in slam_amd/csrc/grid_nav.hip): the planes of 130 x 70 cells are three by two tiles
with ragged last ones, the walls and goals sit on the tile borders x = 63 | 64 and y = 63 | 64, and the corner cases open only
the diagonal (63, 63) - (64, 64) between four tiles.
"""
import functools
import heapq

import numpy as np

FAR = 0xFFFFFFFF
TILE = 64
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
ORTH_W, DIAG_W, NEUTRAL, LETHAL_FROM, UNKNOWN_STEP = 12, 17, 50, 253, 0
REACHED, NO_START, CUT, NOT_CONVERGED = 0, 1, 2, 3
LETHAL, UNKNOWN = 254, 255


def step_table(neutral=NEUTRAL, lethal_from=LETHAL_FROM, unknown_step=UNKNOWN_STEP):
    c = np.arange(256, dtype=np.int64)
    t = np.where(c < lethal_from, neutral + c, 0)
    t[255] = unknown_step
    return t.astype(np.uint32)


def split_goals(cost, sx, sy, S, goals):
    """(the valid goals as (x, y) tuples in order, duplicates kept; how many were skipped)"""
    cost = np.asarray(cost, np.uint8).reshape(sy, sx)
    ok = [(int(x), int(y)) for x, y in np.asarray(goals, np.int64).reshape(-1, 2)
          if 0 <= x < sx and 0 <= y < sy and S[cost[y, x]] != 0]
    return ok, len(np.asarray(goals).reshape(-1, 2)) - len(ok)


def allowed(step, sx, sy, x, y, d):
    """may a path move from (x, y) in direction d?  step: the plane's S[cost], (sy, sx)"""
    dx, dy = DIRS[d]
    vx, vy = x + dx, y + dy
    if not (0 <= vx < sx and 0 <= vy < sy) or step[y, x] == 0 or step[vy, vx] == 0:
        return False
    return not (dx and dy) or (step[y, vx] != 0 and step[vy, x] != 0)


def move_cost(step, x, y, d, orth_w, diag_w):
    dx, dy = DIRS[d]
    return (diag_w if dx and dy else orth_w) * (int(step[y, x]) + int(step[y + dy, x + dx]))


def dijkstra(cost, sx, sy, S, goals, orth_w=ORTH_W, diag_w=DIAG_W):
    step = np.asarray(S, np.int64)[np.asarray(cost, np.uint8).reshape(sy, sx)]
    dist = {}
    heap = [(0, x, y) for x, y in set(split_goals(cost, sx, sy, S, goals)[0])]
    heapq.heapify(heap)
    while heap:
        du, x, y = heapq.heappop(heap)
        if (x, y) in dist:
            continue
        dist[(x, y)] = du
        for d in range(8):
            if allowed(step, sx, sy, x, y, d):
                v = (x + DIRS[d][0], y + DIRS[d][1])
                if v not in dist:
                    heapq.heappush(heap, (du + move_cost(step, x, y, d, orth_w, diag_w), v[0], v[1]))
    out = np.full(sx * sy, FAR, np.uint32)
    for (x, y), du in dist.items():
        out[x + sx * y] = du if du < FAR else FAR
    return out


def bellman_ford(cost, sx, sy, S, goals, orth_w=ORTH_W, diag_w=DIAG_W):
    INF = np.int64(1) << 62
    step = np.zeros((sy + 2, sx + 2), np.int64)                      # a closed frame around the plane: nothing wraps
    step[1:-1, 1:-1] = np.asarray(S, np.int64)[np.asarray(cost, np.uint8).reshape(sy, sx)]
    opn = step != 0
    pot = np.full((sy + 2, sx + 2), INF, np.int64)
    for x, y in split_goals(cost, sx, sy, S, goals)[0]:
        pot[y + 1, x + 1] = 0
    inner = (slice(1, sy + 1), slice(1, sx + 1))

    def shifted(a, dx, dy):
        return a[1 + dy:sy + 1 + dy, 1 + dx:sx + 1 + dx]

    moves = []
    for dx, dy in DIRS:
        ok = opn[inner] & shifted(opn, dx, dy)
        if dx and dy:
            ok = ok & shifted(opn, dx, 0) & shifted(opn, 0, dy)
        moves.append((dx, dy, ok, (diag_w if dx and dy else orth_w) * (step[inner] + shifted(step, dx, dy))))
    while True:
        best = pot[inner].copy()
        for dx, dy, ok, m in moves:
            pv = shifted(pot, dx, dy)
            best = np.minimum(best, np.where(ok & (pv < INF), pv + m, INF))
        if np.array_equal(best, pot[inner]):
            break
        pot[inner] = best
    return np.where(pot[inner] < FAR, pot[inner], FAR).astype(np.uint32).ravel()


def walk(cost, sx, sy, S, pot, start, max_len, orth_w=ORTH_W, diag_w=DIAG_W, converged=True):
    """(the path as int32 [len, 2], status)"""
    none = np.zeros((0, 2), np.int32)
    if not converged:
        return none, NOT_CONVERGED
    step = np.asarray(S, np.int64)[np.asarray(cost, np.uint8).reshape(sy, sx)]
    pot = np.asarray(pot, np.uint32).reshape(sy, sx)
    x, y = int(start[0]), int(start[1])
    if not (0 <= x < sx and 0 <= y < sy) or step[y, x] == 0 or pot[y, x] == FAR:
        return none, NO_START
    path = []
    while len(path) < max_len:
        path.append((x, y))
        if pot[y, x] == 0:
            return np.array(path, np.int32), REACHED
        if len(path) == max_len:
            break
        for d in range(8):
            if allowed(step, sx, sy, x, y, d):
                vx, vy = x + DIRS[d][0], y + DIRS[d][1]
                if pot[vy, vx] != FAR and int(pot[vy, vx]) + move_cost(step, x, y, d, orth_w, diag_w) == int(pot[y, x]):
                    x, y = vx, vy
                    break
        else:
            raise AssertionError("no neighbour continues the path at (%d, %d): the field is not exact" % (x, y))
    return np.array(path, np.int32), CUT


def check_path(cost, sx, sy, S, pot, path, goals, orth_w=ORTH_W, diag_w=DIAG_W):
    """consecutive cells adjacent, every move allowed, the sum of m equals pot[start], the last cell a goal"""
    step = np.asarray(S, np.int64)[np.asarray(cost, np.uint8).reshape(sy, sx)]
    total = 0
    for (x, y), (vx, vy) in zip(path[:-1], path[1:]):
        assert (vx - x, vy - y) in DIRS, ((x, y), (vx, vy))
        d = DIRS.index((vx - x, vy - y))
        assert allowed(step, sx, sy, x, y, d), ((x, y), d)
        total += move_cost(step, x, y, d, orth_w, diag_w)
    assert total == int(pot[path[0][0] + sx * path[0][1]]), (total, pot[path[0][0] + sx * path[0][1]])
    assert tuple(path[-1]) in split_goals(cost, sx, sy, S, goals)[0]


# ------------------------------------------------------------------------------------------------------------------- planes
def plane(sx, sy, fill=0):
    return np.full(sx * sy, fill, np.uint8)


def random_plane(sx, sy, lethal, unknown, seed):
    """random cost bytes 0..252, a share `lethal` of the cells at 254 and a share `unknown` at 255"""
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 253, sx * sy).astype(np.uint8)
    u = rs.uniform(size=sx * sy)
    c[u < lethal] = LETHAL
    c[(u >= lethal) & (u < lethal + unknown)] = UNKNOWN
    return c


def random_table(seed=5):
    """any table that obeys the range: a fifth of the bytes closed, the rest 1 .. 2^20, the extremes present"""
    rs = np.random.RandomState(seed)
    t = rs.randint(1, (1 << 20) + 1, 256).astype(np.uint32)
    t[rs.uniform(size=256) < 0.2] = 0
    t[3], t[4] = 1, 1 << 20
    return t


def wall_130x70(gap_y):
    """lethal columns x = 63 and 64, with a gap at row gap_y (None: closed)"""
    c = plane(130, 70).reshape(70, 130)
    c[:, 63:65] = LETHAL
    if gap_y is not None:
        c[gap_y, 63:65] = 0
    return c.ravel()


def corner_130x70(side_lethal):
    """Two open quadrants, (x <= 63, y <= 63) and (x >= 64, y >= 64), in four different tiles' reach: the other two quadrants
    are lethal but for the two cells (64, 63) and (63, 64), the side cells of the diagonal move (63, 63) - (64, 64) across the
    tile corner.  Open, they carry cost 200, so that the diagonal (17 * 100) is far cheaper than the way round through either
    (12 * 300 twice): the far quadrant is exact only if the tile (1, 1) reads (63, 63) from its corner halo.  side_lethal
    closes (64, 63): the diagonal is forbidden then, and the only way is round through (63, 64)."""
    c = plane(130, 70).reshape(70, 130)
    c[:63, 64:] = LETHAL                                             # the north-east quadrant, but for row 63
    c[63, 65:] = LETHAL                                              # row 63 east of the side cell (64, 63)
    c[65:, :64] = LETHAL                                             # the south-west quadrant, but for row 64
    c[64, :63] = LETHAL                                              # row 64 west of the side cell (63, 64)
    c[63, 64] = c[64, 63] = 200
    if side_lethal:
        c[63, 64] = LETHAL
    return c.ravel()


def room_130x70():
    """a closed room of lethal walls around (70..90, 20..40) -- FAR inside"""
    c = plane(130, 70).reshape(70, 130)
    c[20, 70:91] = c[40, 70:91] = LETHAL
    c[20:41, 70] = c[20:41, 90] = LETHAL
    return c.ravel()


def maze(sx, sy, seed=None):
    """a serpentine: every odd row is a lethal wall with one gap, at the right and at the left end in turn, so that the
    corridors run the plane's length and the shortest path to the far end re-enters every tile column once per corridor.
    seed: random cost bytes 0..99 in the corridors instead of 0"""
    c = plane(sx, sy).reshape(sy, sx)
    if seed is not None:
        c[:] = np.random.RandomState(seed).randint(0, 100, (sy, sx))
    for k, y in enumerate(range(1, sy, 2)):
        c[y, :] = LETHAL
        c[y, sx - 1 if k % 2 == 0 else 0] = 0
    return c.ravel()


# --- Two planes of one-cell corridors in a lethal plane, weights 1 and 1, for what a tile owes its neighbours when a border cell
# falls LATE -- many rounds after the neighbours have settled, so that nothing else re-flags them (docs/GRID_NAV.md section 5).
# The lateness comes from a corridor that crosses the border between the tiles (0, 0) and (0, 1), y = 63 | 64, ten times.
def _hline(c, y, x0, x1, v=0):
    c[y, min(x0, x1):max(x0, x1) + 1] = v


def _vline(c, x, y0, y1, v=0):
    c[min(y0, y1):max(y0, y1) + 1, x] = v


def _late_corridor(c):
    """down column 10 from the main corridor (row 10) to row 65, then four times: right 4 along row 65, up to row 62, right 4
    along row 62, down to row 65; then right 4 along row 65.  Returns the x it ends at, (46, 65)"""
    _vline(c, 10, 11, 65)
    x = 10
    for _ in range(4):
        _hline(c, 65, x, x + 4)
        _vline(c, x + 4, 62, 65)
        _hline(c, 62, x + 4, x + 8)
        _vline(c, x + 8, 62, 65)
        x += 8
    _hline(c, 65, x, x + 4)
    return x + 4


LATE_DROP_STEP = 32903                                               # the step of the cell X (cost byte 1) of late_drop_130x70
LATE_SIDE_STEP = 100000                                              # the step of the side cells (cost byte 2) of late_corner_130x70


def late_table():
    t = np.zeros(256, np.uint32)
    t[0], t[1], t[2] = 1, LATE_DROP_STEP, LATE_SIDE_STEP
    return t


def late_drop_130x70(x_open=True, detour_open=True):
    """The goal is (0, 10) on a corridor along row 10 that runs through all three tile columns.  Inside tile (0, 0) it passes the
    expensive cell X = (30, 10); a detour leaves the corridor at x = 10, takes the late corridor and comes back up column 50.
    The tile's east border cell (63, 10) gets 126 + 2 (LATE_DROP_STEP - 1) through X in round 1 and, ten border crossings later,
    394 through the detour: a fall of exactly 65 536, whose low 16 bits are those of the old value."""
    c = np.full((70, 130), LETHAL, np.uint8)
    _hline(c, 10, 0, 129)
    c[10, 30] = 1 if x_open else LETHAL
    x = _late_corridor(c)
    _vline(c, x, 62, 65)
    _hline(c, 62, x, x + 4)
    _vline(c, x + 4, 11, 62)
    if not detour_open:
        c[11, 10] = LETHAL
    return c.ravel()


def late_corner_130x70():
    """The same goal and main corridor.  The corner cell (63, 63) of tile (0, 0) is the end of the late corridor; (64, 64) in tile
    (1, 1) starts a corridor along row 64 and is reached from (63, 63) by the diagonal, whose side cells (64, 63) and (63, 64) are
    open at LATE_SIDE_STEP and are fed early, from column 64 and from row 68 through (63, 65): they settle in round 2 and do
    not move when (63, 63) falls, so only the tile (0, 0) itself can tell the tile (1, 1) to read its corner halo again."""
    c = np.full((70, 130), LETHAL, np.uint8)
    _hline(c, 10, 0, 129)
    _vline(c, 64, 11, 62)
    c[63, 64] = 2
    _vline(c, 0, 11, 68)
    _hline(c, 68, 0, 63)
    _vline(c, 63, 65, 67)
    c[64, 63] = 2
    x = _late_corridor(c)
    _vline(c, x, 63, 65)
    _hline(c, 63, x, 63)
    _hline(c, 64, 64, 100)
    return c.ravel()


def corridor_130x70():
    """a one-cell corridor along row 10 of a lethal plane, through all three tile columns"""
    c = np.full((70, 130), LETHAL, np.uint8)
    _hline(c, 10, 0, 129)
    return c.ravel()


def corner_goal_130x70():
    """random costs, and the two neighbours of the corner cell (63, 63) inside its own tile that share an edge with it closed:
    from a goal there every way out leads through another tile first ((62, 62) is cut off by the corner rule)"""
    c = random_plane(130, 70, 0.0, 0, 4).reshape(70, 130).copy()
    c[62, 63] = c[63, 62] = LETHAL
    return c.ravel()


SATURATION_MOVE = 255 * (2 * (1 << 19))                            # cost byte 0, neutral 2^19, weight 255: 16 moves fit below FAR


def _case(name, sx, sy, cost, goals, starts=(), S=None, orth_w=ORTH_W, diag_w=DIAG_W):
    cost = np.ascontiguousarray(cost, np.uint8)
    assert cost.size == sx * sy
    cost.setflags(write=False)
    S = step_table() if S is None else S
    return dict(name=name, sx=sx, sy=sy, cost=cost, goals=np.array(goals, np.int32).reshape(-1, 2), starts=tuple(starts), S=S,
                orth_w=orth_w, diag_w=diag_w)


@functools.lru_cache(maxsize=None)
def cases():
    L = [
        _case("1x1", 1, 1, plane(1, 1), [(0, 0)], [(0, 0)]),
        _case("1x300", 1, 300, plane(1, 300, 7), [(0, 150)], [(0, 0), (0, 299)]),
        _case("300x1", 300, 1, plane(300, 1, 7), [(299, 0)], [(0, 0), (130, 0)]),
        _case("63x5", 63, 5, random_plane(63, 5, 0.1, 0, 1), [(62, 4)], [(0, 0), (31, 2)]),
        _case("64x64", 64, 64, random_plane(64, 64, 0.1, 0, 2), [(63, 63)], [(0, 0), (63, 0)]),
        _case("65x67", 65, 67, random_plane(65, 67, 0.1, 0, 3), [(64, 64)], [(0, 0), (64, 66), (0, 66)]),
    ]
    open130 = random_plane(130, 70, 0.0, 0, 4)
    for gx, gy in ((0, 0), (63, 63), (64, 64), (129, 69)):
        L.append(_case("130x70_goal_%d_%d" % (gx, gy), 130, 70, open130, [(gx, gy)], [(129 - gx, 69 - gy), (64, 0), (63, 69)]))
    five = [(5, 5), (100, 10), (129, 69), (20, 66), (70, 64)]
    L.append(_case("130x70_five_goals", 130, 70, random_plane(130, 70, 0.05, 0, 5), five, [(64, 30), (0, 69), (129, 0)]))
    lethal_goal = random_plane(130, 70, 0.0, 0, 6).copy()
    lethal_goal[40 + 130 * 30] = LETHAL
    L.append(_case("130x70_goal_on_lethal", 130, 70, lethal_goal, [(5, 5), (40, 30), (-1, 3), (130, 0), (3, 70), (100, 60)], [(64, 64)]))
    L.append(_case("130x70_only_invalid_goals", 130, 70, lethal_goal, [(40, 30), (-1, 0), (0, -1), (130, 69)], [(64, 64)]))
    L.append(_case("130x70_wall_gap", 130, 70, wall_130x70(40), [(3, 3)], [(129, 0), (65, 39), (65, 69)]))
    L.append(_case("130x70_wall_closed", 130, 70, wall_130x70(None), [(3, 3)], [(129, 0), (62, 69)]))
    L.append(_case("130x70_corner_open", 130, 70, corner_130x70(False), [(3, 3)], [(64, 64), (129, 69), (64, 63)]))
    L.append(_case("130x70_corner_side_lethal", 130, 70, corner_130x70(True), [(3, 3)], [(64, 64), (63, 64)]))
    L.append(_case("130x70_corner_open_back", 130, 70, corner_130x70(False), [(129, 69)], [(0, 0), (63, 63)]))
    L.append(_case("130x70_room", 130, 70, room_130x70(), [(3, 3)], [(80, 30), (91, 41), (129, 69)]))
    L.append(_case("130x70_maze", 130, 70, maze(130, 70), [(0, 0)], [(129, 68), (0, 68), (64, 34)]))
    L.append(_case("130x70_maze_costs", 130, 70, maze(130, 70, seed=7), [(129, 68)], [(0, 0), (64, 32)]))
    # saturation: 16 moves of SATURATION_MOVE fit below FAR, 17 do not -- the far end (0, 299) is FAR, the cell before it is not
    L.append(_case("1x300_saturation", 1, 300, plane(1, 300), [(0, 282)], [(0, 298), (0, 299), (0, 266), (0, 265)],
                   S=step_table(neutral=1 << 19), orth_w=255, diag_w=255))
    for k, lethal in enumerate((0.05, 0.15, 0.3)):
        L.append(_case("random_97x83_d%d" % k, 97, 83, random_plane(97, 83, lethal, 0, 10 + k), [(48, 41), (2, 80)],
                       [(0, 0), (96, 82), (96, 0), (50, 50)]))
    third = random_plane(97, 83, 0.02, 1.0 / 3, 20)
    L.append(_case("random_97x83_unknown_closed", 97, 83, third, [(48, 41), (90, 3)], [(0, 0), (96, 82), (20, 70)]))
    L.append(_case("random_97x83_unknown_400", 97, 83, third, [(48, 41), (90, 3)], [(0, 0), (96, 82), (20, 70)], S=step_table(unknown_step=400)))
    L.append(_case("random_97x83_random_table", 97, 83, random_plane(97, 83, 0.0, 0.02, 21), [(48, 41)], [(0, 0), (96, 82), (5, 77)],
                   S=random_table()))
    L.append(_case("130x70_late_drop", 130, 70, late_drop_130x70(), [(0, 10)], [(129, 10), (64, 10), (63, 10), (46, 63)], S=late_table(),
                   orth_w=1, diag_w=1))
    L.append(_case("130x70_late_corner", 130, 70, late_corner_130x70(), [(0, 10)], [(100, 64), (64, 64), (64, 63), (63, 64)], S=late_table(),
                   orth_w=1, diag_w=1))
    # a goal never falls, so nothing but the seeding itself tells the tiles that hold it in their halo to read it: goals on a tile's
    # border cell whose neighbours inside the tile are closed (or do not exist)
    L.append(_case("1x300_goal_0_63", 1, 300, plane(1, 300, 7), [(0, 63)], [(0, 0), (0, 64), (0, 299)]))
    L.append(_case("1x300_goal_0_64", 1, 300, plane(1, 300, 7), [(0, 64)], [(0, 0), (0, 63), (0, 299)]))
    for gx in (63, 64):
        L.append(_case("130x70_corridor_goal_%d_10" % gx, 130, 70, corridor_130x70(), [(gx, 10)], [(0, 10), (129, 10), (63, 10), (64, 10)]))
    L.append(_case("130x70_corner_goal_closed_in", 130, 70, corner_goal_130x70(), [(63, 63)], [(0, 0), (62, 62), (129, 69), (64, 64)]))
    L.append(_case("65x67_open_ties", 65, 67, plane(65, 67), [(32, 33)], [(0, 0), (64, 66), (64, 0), (0, 66), (32, 0), (0, 33), (64, 40), (10, 66)]))
    return tuple(L)


def case(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case's potential (the heap form), read-only and shared"""
    c = case(name)
    p = dijkstra(c["cost"], c["sx"], c["sy"], c["S"], c["goals"], c["orth_w"], c["diag_w"])
    p.setflags(write=False)
    return p


def starts_of(name):
    """the case's starts, and three read off its field: the cell furthest from the goals, and the first and the last cell
    that reach one"""
    c, p = case(name), expected(name)
    finite = np.flatnonzero(p != FAR)
    if len(finite) == 0:
        return c["starts"]
    picks = (finite[np.argmax(p[finite])], finite[0], finite[-1])
    return c["starts"] + tuple((int(i % c["sx"]), int(i // c["sx"])) for i in picks)


def expected_path(name, start, max_len=None):
    c = case(name)
    return walk(c["cost"], c["sx"], c["sy"], c["S"], expected(name), start, c["sx"] * c["sy"] if max_len is None else max_len,
                c["orth_w"], c["diag_w"])


def expected_goal_counts(name):
    c = case(name)
    ok, skipped = split_goals(c["cost"], c["sx"], c["sy"], c["S"], c["goals"])
    return len(ok), skipped
