"""The correlative matcher over a byte plane and the pose-set scorer (docs/GRID_MATCH.md) restated in numpy, and the cases they
are checked on.  No GPU, no library.  The angle pairs (cos, sin) are inputs -- what slam_csm_angles returned -- so libm is not in
question; every product and sum below is a numpy operation of its own, rounded on its own.

  likelihood_table_np(res, sigma, R)        the table of slam_grid_likelihood_table and the real curve before rounding
  tables(plane, D)                          T (the plane itself) and W, its D x D slide-maximum, D - 1 cells larger towards 0
  cells(pts, c, s, tx, ty, res)             the lattice cell of every point at a pose, and which points have one
  volume_direct / volume_slices             every score of a window, two independent forms; both return (vol, counted)
  match(vol, counted, ...)                  the first maximum in (k, b, a) order: the lowest flat index
  score_poses(tabs, pts, n_ga, poses, res)  the scorer: (score, counted)

A plane is u8 [h, w]; (ox, oy) is the lattice cell of element (0, 0); a table is (ox, oy, array).
"""
import functools

import numpy as np

CELL_LIMIT = float(2 ** 30)


def likelihood_table_np(res, sigma, R):
    k = np.arange(R * R + 2, dtype=np.float64)
    real = 255.0 * np.exp(-(k * (res * res)) / (2.0 * (sigma * sigma)))
    t = np.rint(real)
    t[R * R + 1] = 0
    return t.astype(np.uint8), real


def tables(plane, D):
    T = np.ascontiguousarray(plane, np.uint8)
    h, w = T.shape
    pad = np.zeros((h + 2 * (D - 1), w + 2 * (D - 1)), np.uint8)
    pad[D - 1:D - 1 + h, D - 1:D - 1 + w] = T
    W = np.zeros((h + D - 1, w + D - 1), np.uint8)
    for j in range(D):
        for i in range(D):
            W = np.maximum(W, pad[j:j + h + D - 1, i:i + w + D - 1])
    return T, W


def cells(pts, c, s, tx, ty, res):
    """(cx, cy int64, ok): q = (c px - s py) + tx, (s px + c py) + ty; cell = floor(q / res); ok: finite and within +-2^30"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    px, py = pts[:, 0], pts[:, 1]
    with np.errstate(all="ignore"):
        qx = (c * px - s * py) + tx
        qy = (s * px + c * py) + ty
        fx, fy = np.floor(qx / res), np.floor(qy / res)
        ok = (np.abs(fx) <= CELL_LIMIT) & (np.abs(fy) <= CELL_LIMIT)          # NaN compares false
    cx = np.where(ok, fx, 0).astype(np.int64)
    cy = np.where(ok, fy, 0).astype(np.int64)
    return cx, cy, ok


def lookup(table, cx, cy):
    """table bytes at lattice cells, 0 outside the window"""
    ox, oy, T = table
    h, w = T.shape
    col, row = cx - ox, cy - oy
    inside = (col >= 0) & (col < w) & (row >= 0) & (row < h)
    out = np.zeros(len(cx), np.int64)
    out[inside] = T[row[inside], col[inside]]
    return out


def volume_direct(table, pts, cs, t0, res, half_x, half_y):
    """per candidate, directly: vol[k, b, a] = sum over the points with a cell of T[cell + (a - half_x, b - half_y)]"""
    nth, ny, nx = len(cs), 2 * half_y + 1, 2 * half_x + 1
    vol, counted = np.zeros((nth, ny, nx), np.int32), np.zeros(nth, np.int32)
    for k in range(nth):
        cx, cy, ok = cells(pts, cs[k][0], cs[k][1], t0[0], t0[1], res)
        cx, cy = cx[ok], cy[ok]
        counted[k] = len(cx)
        for b in range(ny):
            for a in range(nx):
                vol[k, b, a] = lookup(table, cx + (a - half_x), cy + (b - half_y)).sum()
    return vol, counted


def volume_slices(table, pts, cs, t0, res, half_x, half_y):
    """per angle: for every distinct scan cell, the slice of the plane its candidates read, added once with its multiplicity"""
    ox, oy, T = table
    h, w = T.shape
    nth, ny, nx = len(cs), 2 * half_y + 1, 2 * half_x + 1
    vol, counted = np.zeros((nth, ny, nx), np.int64), np.zeros(nth, np.int32)
    T64 = T.astype(np.int64)
    for k in range(nth):
        cx, cy, ok = cells(pts, cs[k][0], cs[k][1], t0[0], t0[1], res)
        counted[k] = int(ok.sum())
        if not counted[k]:
            continue
        uniq, mult = np.unique(np.stack([cx[ok], cy[ok]], axis=1), axis=0, return_counts=True)
        for (ux, uy), m in zip(uniq, mult):
            c0, r0 = int(ux) - half_x - ox, int(uy) - half_y - oy             # plane column / row that candidate (0, 0) reads
            a0, a1 = max(0, -c0), min(nx, w - c0)
            b0, b1 = max(0, -r0), min(ny, h - r0)
            if a0 < a1 and b0 < b1:
                vol[k, b0:b1, a0:a1] += int(m) * T64[r0 + b0:r0 + b1, c0 + a0:c0 + a1]
    return vol.astype(np.int32), counted


def bounds(table, D, pts, cs, t0, res, half_x, half_y):
    """U[k, B, A] = sum over the points with a cell of W[cell + (A D - half_x, B D - half_y)]: what the two-level search prunes by"""
    ox, oy, T = table
    Wt = (ox - (D - 1), oy - (D - 1), tables(T, D)[1])
    nbx, nby = (2 * half_x + D) // D, (2 * half_y + D) // D
    U = np.zeros((len(cs), nby, nbx), np.int32)
    for k in range(len(cs)):
        cx, cy, ok = cells(pts, cs[k][0], cs[k][1], t0[0], t0[1], res)
        for B in range(nby):
            for A in range(nbx):
                U[k, B, A] = lookup(Wt, cx[ok] + (A * D - half_x), cy[ok] + (B * D - half_y)).sum()
    return U


def match(vol, counted, n_points, cs, t0, res, half_x, half_y, R0=None):
    """(R [2, 2], t [2], dict(k, a, b, score, n_points, max_score)); fewer than 5 points: the pose kept, score -1"""
    if n_points < 5:
        return (None if R0 is None else np.reshape(R0, (2, 2)).copy()), np.array(t0, np.float64), dict(k=0, a=0, b=0, score=-1, n_points=0, max_score=0)
    k, b, a = (int(v) for v in np.unravel_index(int(np.argmax(vol)), vol.shape))
    c, s = float(cs[k][0]), float(cs[k][1])
    t = np.array([t0[0] + float(a - half_x) * res, t0[1] + float(b - half_y) * res], np.float64)
    return np.array([[c, -s], [s, c]]), t, dict(k=k, a=a, b=b, score=int(vol[k, b, a]), n_points=int(counted[k]), max_score=255 * int(counted[k]))


def score_poses(tabs, pts, n_ga, poses, res):
    """tabs: (table of class GA, table of class NGA), either None = the class has none.  (score int32 [P], counted int32 [P])"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    poses = np.asarray(poses, np.float64).reshape(-1, 4)
    score, counted = np.zeros(len(poses), np.int32), np.zeros(len(poses), np.int32)
    for p, (c, s, tx, ty) in enumerate(poses):
        for cl, part in ((0, pts[:n_ga]), (1, pts[n_ga:])):
            if tabs[cl] is None or len(part) == 0:
                continue
            cx, cy, ok = cells(part, c, s, tx, ty, res)
            counted[p] += int(ok.sum())
            score[p] += int(lookup(tabs[cl], cx[ok], cy[ok]).sum())
    return score, counted


# --------------------------------------------------------------------------------------------------------------- the cases
PLANE_SIZES = ((1, 1), (63, 5), (64, 64), (65, 67), (130, 70), (97, 83))      # (w, h)
ORIGINS = ((-40, -33), (0, 0), (17, 5), (-3, 12), (-70, -20), (5, -60))
BLOCKS = (1, 8, 16, 8, 16, 8)
RES = 0.125                                                                     # dyadic: the cell of a dyadic coordinate is exact


def random_plane(w, h, seed, density=0.35):
    rs = np.random.RandomState(seed)
    p = rs.randint(1, 256, size=(h, w)).astype(np.uint8)
    p[rs.rand(h, w) > density] = 0
    p[h // 2, w // 2] = 200                                                    # never all zero, however small
    return p


def angle_pairs(theta0, half_theta, step):
    th = theta0 + (np.arange(2 * half_theta + 1) - half_theta) * step
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def scan_for(w, h, ox, oy, n, seed, where):
    """n points (sensor frame = lattice frame at the start pose) spread over the plane's window: wholly inside it, half of them
    outside, or wholly outside (far enough that no candidate of a window of half 10 reaches it)"""
    rs = np.random.RandomState(seed)
    x = (ox + rs.rand(n) * w) * RES
    y = (oy + rs.rand(n) * h) * RES
    if where == "half":
        x[::2] += (w + 40) * RES
    if where == "outside":
        x += (w + 40) * RES
        y -= (h + 40) * RES
    return np.stack([x, y], axis=1)


def _case(name, plane, ox, oy, D, pts, n_ga, half=(6, 5, 2), step=0.02, theta0=0.05, t0=(0.0625, -0.03125)):
    return dict(name=name, plane=plane, ox=ox, oy=oy, D=D, pts=np.ascontiguousarray(pts, np.float64), n_ga=n_ga, half_x=half[0],
                half_y=half[1], half_theta=half[2], theta_step=step, theta0=theta0, t0=np.array(t0, np.float64), res=RES)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, ((w, h), (ox, oy), D) in enumerate(zip(PLANE_SIZES, ORIGINS, BLOCKS)):
        plane = random_plane(w, h, 40 + i)
        for where in ("inside", "half", "outside"):
            out.append(_case("%dx%d_%s" % (w, h, where), plane, ox, oy, D, scan_for(w, h, ox, oy, 150, 7 * i, where), 60))
    big, (bx, by) = random_plane(97, 83, 45), (-3, 12)
    out.append(_case("four_points", big, bx, by, 8, scan_for(97, 83, bx, by, 4, 3, "inside"), 2))
    for n in (1023, 1024, 1025):
        out.append(_case("chunk_%d" % n, big, bx, by, 8, scan_for(97, 83, bx, by, n, n, "inside"), n // 3, half=(10, 10, 5)))
    out.append(_case("wide_D16", random_plane(130, 70, 50), -70, -20, 16, scan_for(130, 70, -70, -20, 200, 9, "half"), 0, half=(10, 9, 5)))
    # an exact tie: a plane of one value everywhere, a scan well inside -- every candidate that keeps all points inside scores the same
    flat = np.full((64, 64), 9, np.uint8)
    out.append(_case("tie", flat, 0, 0, 8, scan_for(20, 20, 22, 22, 50, 5, "inside"), 10, half=(5, 5, 1), theta0=0.0, t0=(0.0, 0.0)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def case_angles(c):
    return angle_pairs(c["theta0"], c["half_theta"], c["theta_step"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """(vol, counted) of a case by the slice form with the numpy angle pairs, computed once and shared (read-only)"""
    c = case(name)
    vol, cnt = volume_slices((c["ox"], c["oy"], c["plane"]), c["pts"], case_angles(c), c["t0"], c["res"], c["half_x"], c["half_y"])
    vol.setflags(write=False), cnt.setflags(write=False)
    return vol, cnt


N_GA_SPLITS = (0, 37, 150)           # of a 150-point scan: the class split makes no difference on a plane-built handle
POSE_COUNTS = (1, 63, 64, 65, 257)
POINT_COUNTS = (0, 4, 1023, 1024, 1025)


def pose_set(n_poses, seed, w=97, h=83, ox=-3, oy=12):
    """random poses about the plane's window, one of them NaN, one infinite (where there is room)"""
    rs = np.random.RandomState(seed)
    th = rs.uniform(-np.pi, np.pi, n_poses)
    poses = np.stack([np.cos(th), np.sin(th), (ox + rs.uniform(-0.3, 0.6, n_poses) * w) * RES, (oy + rs.uniform(-0.3, 0.6, n_poses) * h) * RES], axis=1)
    if n_poses > 2:
        poses[1, 3] = np.nan
        poses[2, 2] = np.inf
    return np.ascontiguousarray(poses)


# what the two create calls refuse before they touch the device: w, h, origin_x, origin_y, parameters, a word of the message
BAD_PLANES = [
    (0, 5, 0, 0, {}, "plane of 0 x 5"), (5, 0, 0, 0, {}, "plane of 5 x 0"), (-1, 5, 0, 0, {}, "plane of"), (5, -7, 0, 0, {}, "plane of"),
    (16384, 16384, 0, 0, {}, "bytes of table"), (1 << 20, 300, 0, 0, {}, "bytes of table"), (2147483647, 2147483647, 0, 0, {}, "bytes of table"),
    (10, 10, (1 << 30) - 8, 0, {}, "beyond"), (10, 10, 0, (1 << 30) - 8, {}, "beyond"), (10, 10, -(1 << 30) + 6, 0, {}, "beyond"),
    (10, 10, 0, -(1 << 30) + 6, {}, "beyond"), (10, 10, 2147483647, 0, {}, "beyond"), (10, 10, 0, -2147483648, {}, "beyond"),
    (10, 10, 0, 0, dict(resolution=0.0), "resolution"), (10, 10, 0, 0, dict(resolution=float("nan")), "resolution"),
    (10, 10, 0, 0, dict(block=0), "block"), (10, 10, 0, 0, dict(block=17), "block"), (10, 10, 0, 0, dict(half_x=-1), "half_x"),
    (10, 10, 0, 0, dict(half_theta=16384), "half_x"), (10, 10, 0, 0, dict(half_x=16383, half_y=16383, half_theta=100), "31-bit"),
    (10, 10, 0, 0, dict(theta_step=float("inf")), "theta_step"),
]


# ------------------------------------------------------------------------------------------- the grid -> field -> plane chain
def grid_cells(points, size_x, size_y, res):
    """the window cells of map-frame points by the grid's own rule: f32 points, (int)(v / res + size / 2) truncated"""
    p = np.asarray(points, np.float32).astype(np.float64)
    x = np.trunc(p[:, 0] / res + size_x // 2).astype(np.int64)
    y = np.trunc(p[:, 1] / res + size_y // 2).astype(np.int64)
    ok = (x >= 0) & (y >= 0) & (x < size_x) & (y < size_y)
    return x[ok], y[ok]


def likelihood_plane(occ, size_x, size_y, res, sigma, R):
    """the plane a GridMatcher's field computes from an occupancy plane: two_pass + cost_of with unknown_keep_from = 0"""
    import grid_dist_cases as G
    t, _ = likelihood_table_np(res, sigma, R)
    d2 = G.two_pass(occ, size_x, size_y, R)
    return G.cost_of(d2, occ, t, R, unknown_keep_from=0).reshape(size_y, size_x)
