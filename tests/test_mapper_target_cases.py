"""tests/mapper_target_cases.py, the numpy restatement of the streaming mapper's sliding-window target, checked without a
GPU: against the helper the pose test already uses (first index of np.unique), against a brute-force double loop, against
a per-point loop, on hand-worked cases whose expected values stand HERE, and that every GPU case whose edge is a count
decided by its inputs reaches that count.  docs/MAPPER_TARGET.md."""
import math

import numpy as np
import pytest

import mapper_target_cases as T
from test_gpu_mapper import thin_points


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def random_window(rs, n, extent, spread):
    """points clustered on a few walls so that cells are shared, some outside the extent"""
    wall = rs.randint(0, 4, n)
    u = rs.uniform(-0.6 * extent, 0.6 * extent, n)
    v = 0.3 * extent * (wall - 1.5) + rs.normal(0, spread, n)
    return np.where((wall % 2 == 0)[:, None], np.stack([u, v], 1), np.stack([v, u], 1))


@pytest.mark.parametrize("seed,n,size,res,pitch,cap", [(1, 3000, 400, 0.1, 0.1, 4000), (2, 5000, 200, 0.05, 0.1, 300), (3, 700, 120, 0.1, 0.25, 64),
                                                       (4, 50, 100, 0.1, 0.1, 64), (5, 4000, 333, 0.07, 0.13, 157)])
def test_thin_is_the_pose_tests_helper(seed, n, size, res, pitch, cap):
    pts = random_window(np.random.RandomState(seed), n, size * res, 0.02)
    a, b = T.thin(pts, pitch, size, res, cap), thin_points(pts, pitch, size * res, cap)
    assert 0 < len(b) <= cap and np.array_equal(bits(a.points), bits(b))
    assert len(a.points) == -(-a.kept // a.stride)


def brute_thin(pts, pitch, size, res, cap):
    """every point against every earlier one: a point is a winner when no earlier point shares its cell"""
    inv, x0 = 1.0 / pitch, -0.5 * size * res
    n = int(math.ceil(size * res * inv))

    def cell(p):
        v = ((float(p[0]) - x0) * inv, (float(p[1]) - x0) * inv)
        if not (math.isfinite(v[0]) and math.isfinite(v[1])):
            return None
        c = (math.floor(v[0]), math.floor(v[1]))
        return c if 0 <= c[0] < n and 0 <= c[1] < n else None
    win = []
    for i in range(len(pts)):
        ci = cell(pts[i])
        if ci is None:
            continue
        if all(cell(pts[j]) != ci for j in range(i)):
            win.append(i)
    stride = max(1, -(-len(win) // cap))
    return pts[win[::stride]], len(win), stride


@pytest.mark.parametrize("seed,n,cap", [(11, 300, 64), (12, 257, 1000), (13, 120, 7), (14, 300, 29)])
def test_thin_is_the_brute_force_loop(seed, n, cap):
    rs = np.random.RandomState(seed)
    pts = random_window(rs, n, 12.0, 0.05)
    pts[rs.randint(0, n, 5)] = [[np.nan, 0.0], [0.0, np.inf], [-np.inf, 1.0], [1e308, 0.0], [np.nan, np.nan]]
    a = T.thin(pts, 0.25, 120, 0.1, cap)
    want, kept, stride = brute_thin(pts, 0.25, 120, 0.1, cap)
    assert (a.kept, a.stride) == (kept, stride) and np.array_equal(bits(a.points), bits(want))


def loop_window_points(c, R, t, stride_ga, stride_nga):
    """point by point, as the kernel takes them: the scan of point i, its rank in its class, its slot"""
    ga_before = [0]
    for s in range(c.n_scans):
        ga_before.append(ga_before[-1] + int(c.scan_nga[s]))
    out = ({}, {})
    for i in range(c.n_points):
        s = max(k for k in range(c.n_scans) if c.scan_off[k] <= i)          # the last scan that begins at or before i
        j, g = i - int(c.scan_off[s]), int(c.scan_nga[s])
        is_ga = j < g
        rank = ga_before[s] + j if is_ga else (int(c.scan_off[s]) - ga_before[s]) + (j - g)
        stride = stride_ga if is_ga else stride_nga
        if rank % stride:
            continue
        x, y = float(c.pts[i, 0]), float(c.pts[i, 1])
        q = ((float(R[s, 0]) * x + float(R[s, 1]) * y) + float(t[s, 0]), (float(R[s, 2]) * x + float(R[s, 3]) * y) + float(t[s, 1]))
        slot = out[0 if is_ga else 1]
        assert rank // stride not in slot
        slot[rank // stride] = q
    for d in out:
        assert sorted(d) == list(range(len(d)))                              # no hole, no slot twice
    return tuple(np.array([d[k] for k in range(len(d))], np.float64).reshape(-1, 2) for d in out)


@pytest.mark.parametrize("name,k,sg,sn", [("empty scans, prior kept", 0, 1, 2), ("empty scans, prior kept", 1, 3, 1),
                                          ("strides 1, 2, 3 around per_chunk", 2, 3, 2), ("six rebuilds in a row", 0, 1, 1),
                                          ("six rebuilds in a row", 1, 4, 7)])
def test_window_points_is_the_per_point_loop(name, k, sg, sn):
    c = T.case(name).chunks()[k]
    rs = np.random.RandomState(k)
    R, t = c.R + rs.normal(0, 0.01, c.R.shape), c.t + rs.normal(0, 0.1, c.t.shape)
    a, b = T.window_points(c, R, t, sg, sn), loop_window_points(c, R, t, sg, sn)
    n_ga, n_nga = T.class_totals(c)
    assert len(a[0]) == -(-n_ga // sg) and len(a[1]) == -(-n_nga // sn)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


# ------------------------------------------------------------------ hand-worked: the expected values stand here
# a lattice of pitch 0.25 over 16 cells of 0.25 m: extent 4, origin -2, inv = 4 -- every product below is exact
HAND = dict(thin_res=0.25, grid_size=16, res=0.25)


def test_hand_four_points_in_one_cell_the_oldest_wins():
    chunk_a = [(0.10, 0.10), (0.20, 0.05)]          # all four in cell (8, 8): [0, 0.25) x [0, 0.25)
    chunk_b = [(0.01, 0.24), (0.15, 0.15)]
    got = T.thin(np.array(chunk_a + chunk_b), cap=64, **HAND)
    assert got.kept == 1 and got.stride == 1 and got.points.tolist() == [[0.10, 0.10]]
    got = T.thin(np.array(chunk_b + chunk_a), cap=64, **HAND)      # the other chunk older: its first point
    assert got.points.tolist() == [[0.01, 0.24]]


def test_hand_lattice_lines_and_the_extent():
    below = np.nextafter
    pts = np.array([
        (0.25, -1.9),                    # 0 on the line between cells 8 and 9: (0.25 + 2) * 4 = 9 exactly -> cell 9, row 0: kept
        (below(0.25, 0.0), -1.6),        # 1 one ulp below the line: q + 2 rounds to 2.25 -> cell 9 too (row 1): kept
        (-2.0, -1.3),                    # 2 at -extent/2: (q + 2) * 4 = 0 -> cell 0: inside, kept
        (below(-2.0, -3.0), -1.0),       # 3 one ulp beyond -extent/2: -2^-51 * 4, floor -1: outside
        (2.0, -0.7),                     # 4 at +extent/2: 16 = nx: outside
        (below(2.0, 0.0), -0.4),         # 5 one ulp inside +extent/2: q + 2 = 4 - 2^-52 ties to 4.0 -> 16: outside
        (1.99, -0.1),                    # 6 cell 15: kept
        (0.26, -1.6),                    # 7 cell 9 of row 1: point 1 is there already -> dropped (so point 1 IS in cell 9)
        (0.24, -1.6),                    # 8 cell 8 of row 1: free -> kept
        (0.0, below(2.0, 0.0)),          # 9 the same tie along y: outside
        (0.0, 1.9999),                   # 10 row 15: kept
    ])
    got = T.thin(pts, cap=64, **HAND)
    assert got.index.tolist() == [0, 1, 2, 6, 8, 10] and got.kept == 6
    assert np.array_equal(bits(got.points), bits(pts[[0, 1, 2, 6, 8, 10]]))


def test_hand_nan_and_infinity_take_no_part():
    pts = np.array([(np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0), (1e308, 0.0), (0.0, np.nan), (0.5, 0.5), (np.inf, np.inf)])
    got = T.thin(pts, cap=64, **HAND)
    assert got.kept == 1 and got.index.tolist() == [5] and got.points.tolist() == [[0.5, 0.5]]


def test_hand_cap_and_cap_plus_one():
    row = [(-1.9 + 0.25 * k, 0.1) for k in range(6)]             # six cells of one row, in order
    got = T.thin(np.array(row[:4]), cap=4, **HAND)
    assert (got.kept, got.stride) == (4, 1) and got.index.tolist() == [0, 1, 2, 3]          # kept == cap: all
    got = T.thin(np.array(row[:5]), cap=4, **HAND)
    assert (got.kept, got.stride) == (5, 2) and got.index.tolist() == [0, 2, 4]             # cap + 1: ceil(5 / 2) = 3
    got = T.thin(np.array(row + [row[0]]), cap=4, **HAND)
    assert (got.kept, got.stride) == (6, 2) and got.index.tolist() == [0, 2, 4]
    got = T.thin(np.array(row), cap=2, **HAND)
    assert (got.kept, got.stride) == (6, 3) and got.index.tolist() == [0, 3]


class HandChunk:
    """five scans: both classes | no GA | EMPTY | no NGA | EMPTY last; integer coordinates"""
    pts = np.array([(1, 0), (2, 0), (3, 0),          # scan 0: GA (1,0) (2,0), NGA (3,0)
                    (4, 0), (5, 0),                  # scan 1: NGA (4,0) (5,0)
                    (6, 0), (7, 0)], np.float64)     # scan 3: GA (6,0) (7,0)
    scan_off = np.array([0, 3, 5, 5, 7, 7], np.int32)
    scan_nga = np.array([2, 0, 0, 2, 0], np.int32)
    n_scans, n_points = 5, 7
    # scan s: a quarter turn and t = (s, 10 s): q = (-y + s, x + 10 s)
    R = np.tile([0.0, -1.0, 1.0, 0.0], (5, 1))
    t = np.array([(s, 10.0 * s) for s in range(5)])


def test_hand_window_points_over_empty_scans():
    c = HandChunk
    ga, nga = T.window_points(c, c.R, c.t, 1, 1)
    assert ga.tolist() == [[0, 1], [0, 2], [3, 36], [3, 37]]          # scan 0's two, then scan 3's two
    assert nga.tolist() == [[0, 3], [1, 14], [1, 15]]                 # scan 0's one, scan 1's two
    ga, nga = T.window_points(c, c.R, c.t, 2, 2)
    assert ga.tolist() == [[0, 1], [3, 36]] and nga.tolist() == [[0, 3], [1, 15]]     # ranks 0 and 2 of either class
    ga, nga = T.window_points(c, c.R, c.t, 3, 4)
    assert ga.tolist() == [[0, 1], [3, 37]] and nga.tolist() == [[0, 3]]
    for sg, sn in ((1, 1), (2, 2), (3, 4)):
        a, b = T.window_points(c, c.R, c.t, sg, sn), loop_window_points(c, c.R, c.t, sg, sn)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_hand_strides():
    assert T.per_chunk_of(256, 2) == 64 and T.per_chunk_of(8000, 2) == 2000 and T.per_chunk_of(100, 8) == 64 and T.per_chunk_of(600, 2) == 150
    assert [T.stride_for(n, 0.0, 256, 2) for n in (0, 1, 63, 64, 65, 128, 129)] == [1, 1, 1, 1, 2, 2, 3]
    assert T.stride_for(10 ** 6, 0.1, 256, 2) == 1                    # thinned at rebuild time instead


def test_hand_target_and_the_five_point_rule():
    prm = dict(window_chunks=2, keep_prior=1, thin_res=0.0, target_points=256, grid_size=16, resolution=0.25)
    prior_ga, prior_nga = np.array([(9.0, 9.0)]), np.array([(8.0, 8.0), (7.0, 7.0)])
    e = [(np.array([(0.0, 0.0)]), np.zeros((0, 2))), (np.array([(1.0, 1.0)]), np.array([(1.5, 1.5)])), (np.zeros((0, 2)), np.array([(0.1, 0.1)]))]
    ga, nga, _ = T.target(prior_ga, prior_nga, e, prm)                # the newest two, oldest first, behind the prior
    assert ga.tolist() == [[9, 9], [1, 1]] and nga.tolist() == [[8, 8], [7, 7], [1.5, 1.5], [0.1, 0.1]]
    assert T.target(prior_ga, prior_nga, e, dict(prm, keep_prior=0)) is None              # three points: the previous target stays
    assert T.target(prior_ga, prior_nga, e[:1], prm) is None                              # 1 + 3 = four points
    ga, nga, info = T.target(prior_ga, prior_nga, e, dict(prm, thin_res=0.25))            # (0.1, 0.1) and (1.5, 1.5): two cells
    assert ga.tolist() == [[9, 9], [1, 1]] and nga.tolist() == [[8, 8], [7, 7], [1.5, 1.5], [0.1, 0.1]] and info["nga"]["kept"] == 2
    assert T.target(prior_ga, prior_nga, [e[0], e[0]], dict(prm, thin_res=0.25)) is None   # 1 + 1 cell + 2: four points
    more = np.array([(8.0, 8.0), (7.0, 7.0), (6.0, 6.0)])
    ga, nga, info = T.target(prior_ga, more, [e[0], e[0]], dict(prm, thin_res=0.25))       # no NGA point in the window
    assert ga.tolist() == [[9, 9], [0, 0]] and nga.tolist() == [[8, 8], [7, 7], [6, 6]] and info["nga"]["kept"] == 0


def test_hand_schedule():
    s = T.Schedule(2, 1)
    assert [s.push(k) for k in range(4)] == [None, [0], [0, 1], [1, 2]]
    s = T.Schedule(2, 3)                    # due when k - max(last, 0) >= 3: pushes 3, 6, 9
    assert [s.push(k) for k in range(10)] == [None, None, None, [1, 2], None, None, [4, 5], None, None, [7, 8]]
    s = T.Schedule(8, 1)
    assert s.push(0) is None and s.push(1) == [0] and [s.push(k) for k in range(2, 10)][-1] == list(range(1, 9))
    assert T.Schedule(0, 1).push(5) is None


# ------------------------------------------------------------------ the GPU cases reach their edges
def test_cases_reach_the_edges():
    pc = T.per_chunk_of(T.STRIDE_TARGET, 2)
    tot = [T.class_totals(c) for c in T.case("strides 1, 2, 3 around per_chunk").chunks()]
    assert pc == 64 and tot == T.STRIDE_TOTALS
    assert {n for _, n in tot} >= {pc - 1, pc, pc + 1} and {n for n, _ in tot} >= {2 * pc - 1, 2 * pc, 2 * pc + 1, pc, pc + 1}
    assert [T.stride_for(n, 0.0, T.STRIDE_TARGET, 2) for _, n in tot] == [1, 1, 2, 3, 2]
    assert [T.stride_for(n, 0.0, T.STRIDE_TARGET, 2) for n, _ in tot] == [2, 2, 3, 1, 2]

    for name in ("empty scans, prior kept", "empty scans, no prior"):
        for c in T.case(name).chunks():
            n = np.diff(c.scan_off)
            assert n.tolist() == [61, 61, 0, 61, 0] and c.scan_nga.tolist() == [20, 0, 0, 61, 0]
            assert T.class_totals(c) == (81, 102)
        assert T.stride_for(81, 0.0, 400, 2) == 1 and T.stride_for(102, 0.0, 400, 2) == 2

    tot = [T.class_totals(c) for c in T.case("class totals 255, 256, 257, 513").chunks()]
    assert tot == T.BLOCK_TOTALS
    for cls in (0, 1):
        assert {t[cls] for t in tot} >= {255, 256, 257, 513}

    ch = T.case("more than 65 536 points").chunks()
    n = [T.class_totals(c) for c in ch]
    assert n[0][0] == n[1][0] == 0 and n[0][1] + n[1][1] > 65536              # one class, two chunks
    blocks = (n[0][1] + n[1][1] + 255) // 256
    assert blocks > 256 + 4                                                   # more than kThinGrid blocks, and the scan's second round
    assert max(c.n_points for c in ch) <= T.MANY_SCANS * 1081

    c = T.case("eight segments and the ring's wrap")
    assert c.params["window_chunks"] == 8 and len(c.chunks()) == 13 and all(min(T.class_totals(k)) > 0 for k in c.chunks())
    assert len(T.case("six rebuilds in a row").chunks()) == 7
    assert all(T.class_totals(k)[0] == 0 for k in T.case("no GA point in the window").chunks())
    for name in ("fewer than five points, not thinned", "fewer than five points, thinned"):
        ch = T.case(name).chunks()
        assert T.class_totals(ch[0]) == (3, 1) and ch[0].n_scans == 1 and T.case(name).params["keep_prior"] == 0
    c = T.case("a rebuild every third chunk")
    assert len(c.chunks()) == 10 and c.params["rebuild_every"] == 3 and c.params["window_chunks"] == 2
    for c in T.CASES:
        assert c.params["grid_size"] <= 400
        for k in c.chunks():
            assert k.scan_off[0] == 0 and k.scan_off[-1] == len(k.pts) and np.all(np.diff(k.scan_off) >= k.scan_nga) and np.isfinite(k.pts).all()
