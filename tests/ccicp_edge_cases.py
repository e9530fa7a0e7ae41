"""Edge cases of the CCICP chain's device entry points and their plain references.  Not a test file:
tests/test_ccicp_edge_cases.py holds the references below to the oracle on the CPU, tests/test_gpu_ccicp_edges.py the
device to them, on the same inputs.  numpy and Python integers only; slam_amd is not imported here.

The two arithmetic bounds of a voxel centroid (docs/CCICP_EDGES.md):
  A. The device sums rint(float64(p) * 2^24) of a voxel's points as 64-bit integers (exact, order-free) and stores
     float32(float64(sum) * (1 / (count * 2^24))).  |sum| < 2^53 converts exactly; the reciprocal and the product are one
     float64 rounding each (2^-53 relative), the store one float32 rounding.  So against the fixed-point mean
     sum / (count * 2^24) -- `voxel_exact`'s `fix` --
         |got - exact| <= ulp32(exact) / 2 * (1 + 2^-20):
     a correctly rounded float plus slack for the double arithmetic (2^-52 relative is 2^-28 of an ulp32: the slack also
     covers the float64 in which the tests form the difference).
  B. A float32 coordinate that is no multiple of 2^-24 moves by at most 2^-25 when it is quantised, and so does the mean.
     Against the TRUE mean of such points -- `voxel_exact`'s `true` -- the bound is A + 2^-25.
Most cases are built from multiples of 2^-10 within +-300 m, for which the fixed-point mean IS the true mean and only A
applies."""
import math
from fractions import Fraction

import numpy as np

FIX = 1 << 24
QUANT = 2.0 ** -25
SLACK = 1.0 + 2.0 ** -20
SENTINEL = 0xA5  # the byte every output buffer holds before a call


# ------------------------------------------------------------------ bounds
def ulp32(x):
    """spacing of float32 in the binade of |x| (the smallest subnormal at and around 0)"""
    e = np.frexp(np.abs(np.asarray(x, np.float64)))[1]           # |x| = m * 2^e, m in [0.5, 1)
    return np.where(np.asarray(x) == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def centroid_bound(exact, dyadic=True):
    return ulp32(exact) / 2 * SLACK + (0.0 if dyadic else QUANT)


# ------------------------------------------------------------------ ordered floats
def order_f32(f):
    u = int(np.float32(f).view(np.uint32))
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def unorder_f32(u):
    u = int(u)
    v = (u & 0x7fffffff) if u & 0x80000000 else (~u & 0xffffffff)
    return np.uint32(v).view(np.float32)


def extent_words(pts, flags):
    """the six words slam_gseg_classify_ga_extent_dev leaves: minima and maxima over the finite points whose flag is not
    255, decoded (None where nothing was kept: the words stay 0xffffffff / 0)"""
    p = np.asarray(pts, np.float32)[:, :3]
    keep = np.isfinite(p).all(1) & (np.asarray(flags) != 255)
    if not keep.any():
        return None
    return np.concatenate([p[keep].min(0), p[keep].max(0)])


# ------------------------------------------------------------------ the exact voxel filter
def voxel_exact(pts, flags=None, leaf=(0.5, 0.5, 2.0)):
    """pcl::VoxelGrid as setSceneCloud uses it, restated (voxel_grid.hpp): membership floorf(float32(x) * float32(1 / leaf))
    minus the lattice minimum taken from the extent of the kept finite points; per voxel the sum of rint(float64(p) * 2^24) as
    Python ints.  pts [n, >= 3] f32; flags uint8 (1 GA, 0 NGA, 255 dropped) or None (the class is column 3 > 0.5, NGA without
    one).  Returns dict: idx (voxel index, increasing, x fastest), count, n_ga, frac (the exact fixed-point means as
    Fractions, [m][3]), fix and true ([m, 3] f64: that mean and the mean of the unquantised coordinates, both correctly
    rounded), flag ([m] f32: uint16(float32(n_ga) / float32(count)), which truncates)."""
    pts = np.asarray(pts, np.float32)
    p = pts[:, :3]
    keep = np.isfinite(p).all(1)
    if flags is not None:
        keep &= np.asarray(flags) != 255
        ga = np.asarray(flags) == 1
    elif pts.shape[1] > 3:
        ga = pts[:, 3] > np.float32(0.5)
    else:
        ga = np.zeros(len(pts), bool)
    empty = dict(idx=np.zeros(0, np.int64), count=np.zeros(0, np.int64), n_ga=np.zeros(0, np.int64), frac=[],
                 fix=np.zeros((0, 3)), true=np.zeros((0, 3)), flag=np.zeros(0, np.float32))
    if not keep.any():
        return empty
    q, ga = p[keep], ga[keep]
    inv = np.float32(1) / np.asarray(leaf, np.float32)
    min_b = np.floor(q.min(0) * inv)                               # float32 throughout, as PCL
    div_b = (np.floor(q.max(0) * inv) - min_b).astype(np.int64) + 1
    ijk = (np.floor(q * inv) - min_b).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]
    order = np.argsort(idx, kind="stable")
    fixed = np.rint(q.astype(np.float64) * FIX).astype(np.int64)[order].tolist()   # Python ints from here on
    raw = q.astype(np.float64)[order]
    sidx, sga = idx[order], ga[order]
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    ends = np.r_[starts[1:], len(sidx)]
    out = dict(idx=sidx[starts], count=ends - starts, n_ga=np.array([int(sga[a:b].sum()) for a, b in zip(starts, ends)]), frac=[])
    fix, true = np.zeros((len(starts), 3)), np.zeros((len(starts), 3))
    for v, (a, b) in enumerate(zip(starts.tolist(), ends.tolist())):
        row = []
        for d in range(3):
            s = sum(r[d] for r in fixed[a:b])
            row.append(Fraction(s, (b - a) * FIX))
            fix[v, d] = float(row[-1])
            true[v, d] = math.fsum(raw[a:b, d]) / (b - a)
        out["frac"].append(row)
    out["fix"], out["true"] = fix, true
    out["flag"] = (out["n_ga"].astype(np.float32) / out["count"].astype(np.float32)).astype(np.uint16).astype(np.float32)
    return out


def for_oracle(pts, flags=None):
    """the same cloud as oracle_lib.voxel_downsample takes it: dropped points gone, the class as 0 / 1 in column 3"""
    pts = np.asarray(pts, np.float32)
    if flags is not None:
        keep, ga = np.asarray(flags) != 255, np.asarray(flags) == 1
    else:
        keep, ga = np.ones(len(pts), bool), (pts[:, 3] > np.float32(0.5)) if pts.shape[1] > 3 else np.zeros(len(pts), bool)
    return np.concatenate([pts[keep, :3], ga[keep, None].astype(np.float32)], 1)


# ------------------------------------------------------------------ voxel cases
def _in_cells(cells, leaf, rs, spread=True):
    """one point per row of `cells` [m, 3] (voxel coordinates) on multiples of 2^-10 inside its voxel (dyadic leaves)"""
    leaf = np.asarray(leaf, np.float64)
    steps = np.round(leaf * 1024).astype(np.int64)
    off = np.stack([rs.randint(0, s, len(cells)) for s in steps], 1) if spread else np.zeros((len(cells), 3), np.int64)
    return (np.asarray(cells) * leaf + off / 1024.0).astype(np.float32)


def _cell(c):
    """the c-th of a supply of distinct voxels: 400 x 400 columns around the origin (negative coordinates too), three layers"""
    return [c % 400 - 200, (c // 400) % 400 - 200, c // 160000 - 1]


RUN_LENGTHS = (1, 2, 63, 64, 65, 128, 255, 256, 257, 300)
RUN_OFFSETS = (0, 1, 62, 63)
LEAF = (0.5, 0.5, 2.0)


def run_cloud(seed=21):
    """runs of equal voxels of every length in RUN_LENGTHS, each starting on every lane in RUN_OFFSETS (points alone in their
    voxel in front set the lane); returns (pts, flags, runs) with runs = [(first index, length)]"""
    rs = np.random.RandomState(seed)
    cells, runs, c = [], [], 0
    for length in RUN_LENGTHS:
        for off in RUN_OFFSETS:
            while len(cells) % 64 != off:
                cells.append(_cell(c)); c += 1
            runs.append((len(cells), length))
            cells += [_cell(c)] * length; c += 1
    cells.append(_cell(c))
    pts = _in_cells(np.array(cells), LEAF, rs)
    return pts, rs.randint(0, 2, len(pts)).astype(np.uint8), runs


def voxel_cases():
    """dicts: name, pts [n, stride] f32, flags (uint8 or None), leaf, dyadic (every coordinate a multiple of 2^-24: bound A alone)"""
    rs = np.random.RandomState(22)
    out = []

    def add(name, pts, flags=None, leaf=LEAF, dyadic=True):
        out.append(dict(name=name, pts=np.ascontiguousarray(pts, np.float32), flags=None if flags is None else np.asarray(flags, np.uint8),
                        leaf=leaf, dyadic=dyadic))

    pts, flags, _ = run_cloud()
    add("runs of every length on every lane", pts, flags)
    a, b = _cell(7), _cell(3001)
    add("1000 points in one voxel", _in_cells([a] * 1000, LEAF, rs), rs.randint(0, 2, 1000))
    add("ABAB", _in_cells([a, b] * 200, LEAF, rs), rs.randint(0, 2, 400))
    add("A-run B-run A-run", _in_cells([a] * 70 + [b] * 70 + [a] * 70, LEAF, rs), rs.randint(0, 2, 210))
    # dropped points inside a run: they break it and add nothing (the flag-255 point lies in another voxel, far off: counted,
    # it would be a second output row)
    pts = _in_cells([a] * 100, LEAF, rs)
    flags = np.ones(100, np.uint8)
    flags[10] = 255
    pts[10] = [250.0, -250.0, 3.0]
    pts[20, 0], pts[30, 1], pts[40, 2] = np.nan, np.inf, -np.inf
    flags[63], flags[64] = 255, 255                                   # ... and on a wavefront's last and first lane
    add("dropped points inside a run", pts, flags)
    neg = np.array([[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-2.0 ** -10, -2.0 ** -10, -2.0 ** -10], [-0.5, -0.5, -2.0],
                    [-0.5 - 2.0 ** -10, -0.5, -2.0], [-299.5, -299.5, -9.0], [-1.0, 2.0, -0.0]])
    add("negative coordinates and -0.0", neg, [1, 0, 1, 1, 0, 1, 0])
    for leaf in ((0.5, 0.5, 2.0), (0.25, 0.3, 1.0), (0.5, 0.5, 5.0)):
        k = np.arange(-5, 6)
        face = np.stack(np.meshgrid(k, k, [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3) * np.asarray(leaf, np.float32)
        add("points on voxel faces, leaf %s" % (leaf,), np.concatenate([face, face]), rs.randint(0, 2, 2 * len(face)), leaf)
    # below 0.5 m a float32 has bits under 2^-24: the one kind of coordinate the fixed point quantises (bound B)
    add("coordinates that are no multiples of 2^-24", rs.uniform(-0.5, 0.5, (600, 3)), rs.randint(0, 2, 600), (0.25, 0.3, 1.0), dyadic=False)
    add("one point", [[1.25, -3.5, 0.75]], [1])
    add("two identical points", [[1.25, -3.5, 0.75]] * 2, [1, 0])
    add("flag truncation: all GA", _in_cells([a] * 10, LEAF, rs), [1] * 10)
    add("flag truncation: all but one GA", _in_cells([a] * 10, LEAF, rs), [1] * 9 + [0])
    g = np.float32([0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0, np.nan, 2.0, -1.0])
    cells = [_cell(i) for i in range(len(g))]
    add("class from float [3], stride 4", np.concatenate([_in_cells(cells, LEAF, rs), g[:, None]], 1))
    add("class from float [3], stride 6", np.concatenate([_in_cells(cells, LEAF, rs), g[:, None], np.full((len(g), 2), np.nan)], 1))
    add("stride 3 without flags: every voxel NGA", _in_cells([a, a, b], LEAF, rs))
    wide = np.stack([rs.randint(-300 * 1024, 300 * 1024, 3000), rs.randint(-300 * 1024, 300 * 1024, 3000), rs.randint(-4096, 4096, 3000)], 1) / 1024.0
    add("cloud over 300 m", wide, rs.randint(0, 2, 3000))
    tiny = np.stack([rs.randint(-1024, 1024, 500), rs.randint(-1024, 1024, 500), rs.randint(-512, 512, 500)], 1) / 1024.0
    add("cloud over 2 m", tiny, rs.randint(0, 2, 500))
    return out


# ------------------------------------------------------------------ compaction cases
BLOCK = 1024  # items per block of the one-launch compaction
COMPACT_SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65 * 1024, 65 * 1024 + 1, 68 * 1024 + 7)


def shrink_and_grow(sizes=COMPACT_SIZES):
    """largest, smallest, second largest, second smallest, ...: on one handle every call meets words a larger call left"""
    s = sorted(sizes)
    out = []
    while s:
        out.append(s.pop())
        if s:
            out.append(s.pop(0))
    return out


def patterns(n, seed=0):
    """(name, selection [n] bool)"""
    i = np.arange(n)
    nb = (n + BLOCK - 1) // BLOCK
    yield "all", np.ones(n, bool)
    yield "none", np.zeros(n, bool)
    yield "first only", i == 0
    yield "last only", i == n - 1
    yield "alternating", i % 2 == 1
    yield "first block", i // BLOCK == 0
    yield "middle block", i // BLOCK == nb // 2
    yield "last block", i // BLOCK == nb - 1
    yield "random 0.5", np.random.RandomState(1000 + n + seed).rand(n) < 0.5


def cloud_of(n, seed=0):
    """n distinct rows on multiples of 2^-10: a row names its index"""
    rs = np.random.RandomState(2000 + seed)
    return np.stack([np.arange(n) / 1024.0 - 30.0, rs.randint(-40960, 40960, n) / 1024.0, rs.randint(-2048, 2048, n) / 1024.0], 1).astype(np.float32)


def strided(rows, stride):
    """rows [n, k] as [n, stride] with NaN in the padding"""
    out = np.full((len(rows), stride), np.nan, np.float32)
    out[:, :rows.shape[1]] = rows
    return out


CROP_BOX = (0.0, 5.0, -5.0, 0.0)   # = ccicp_crop(cur = (2.5, -2.5), crop = 2.5): the float limits are these exactly
CROP_CUR = (2.5, -2.5, 2.5)


def box_keep(pts, box):
    """pcl::PassThrough on x then y with float limits, closed; non-finite points go"""
    p = np.asarray(pts, np.float32)
    b = np.asarray(box, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p[:, :3]).all(1) & (p[:, 0] >= b[0]) & (p[:, 0] <= b[1]) & (p[:, 1] >= b[2]) & (p[:, 1] <= b[3])


def split_reference(pts, box=None, cap=None):
    """(ga, nga, totals): f64 xy of each class in cloud order, cut to cap - 1 rows; totals are uncapped"""
    p = np.asarray(pts, np.float32)
    keep = box_keep(p, box) if box is not None else np.ones(len(p), bool)
    with np.errstate(invalid="ignore"):
        ga = keep & (p[:, 3] > np.float32(0.5))
    nga = keep & ~ga
    lim = None if cap is None else cap - 1
    return p[ga][:lim, :2].astype(np.float64), p[nga][:lim, :2].astype(np.float64), (int(ga.sum()), int(nga.sum()))


def face_cloud():
    """points on every face of CROP_BOX (kept), one step outside each (dropped), -0.0 against the 0.0 faces, non-finite
    points, and the flag values either side of isGA's 0.5; [n, 4] f32"""
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    x_lo, x_hi, y_lo, y_hi = (f(v) for v in CROP_BOX)
    half_up = np.nextafter(f(0.5), f(1))
    rows = [[x_lo, -1, 0, 1], [dn(x_lo), -1, 0, 1], [x_hi, -1, 0, 0], [up(x_hi), -1, 0, 0],
            [1, y_lo, 0, 1], [1, dn(y_lo), 0, 1], [1, y_hi, 0, 0], [1, up(y_hi), 0, 0],
            [-0.0, -1, 0, 1], [1, -0.0, 0, 0], [-0.0, -0.0, -0.0, 1], [x_lo, y_lo, 0, 1], [x_hi, y_hi, 0, 0],
            [np.nan, -1, 0, 1], [1, np.inf, 0, 0], [1, -1, np.nan, 1], [1, -1, -np.inf, 0], [-np.inf, -1, 0, 1],
            [1, -1, 0, 0.5], [1, -1, 0, half_up], [1, -1, 0, np.nan], [2, -2, 0, np.nextafter(f(0.5), f(0))], [2, -2, 0, np.inf]]
    return np.array(rows, np.float32)


def cap_cloud(n=5000, seed=31):
    """about half GA, most inside the box of CROP_WIDE: more than 1026 of each class inside, so that every cap of CAP_VALUES bites"""
    rs = np.random.RandomState(seed)
    xy = rs.randint(-12 * 1024, 12 * 1024, (n, 2)) / 1024.0
    return np.concatenate([xy, np.zeros((n, 1)), rs.randint(0, 2, (n, 1))], 1).astype(np.float32)


CROP_WIDE = (0.0, 0.0, 10.0)   # cur_x, cur_y, crop: the box [-10, 10]^2


def cap_values(total):
    return (1, 2, total, total + 1, total + 2, 1025, 1026)


# ------------------------------------------------------------------ height cases
def quat_rpy(roll, pitch, yaw):
    """tf::createQuaternionFromRPY (tf::Quaternion::setRPY), float64: (x, y, z, w)"""
    hy, hp, hr = yaw * 0.5, pitch * 0.5, roll * 0.5
    cy, sy, cp, sp, cr, sr = math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr), math.sin(hr)
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def yaw_of(R):
    """the yaw doICPMatch takes from the matched rotation (icpTools.cpp:195-197); R: 2 x 2, row major"""
    R = np.asarray(R, np.float64).reshape(4)
    return math.atan2(R[2], R[0])


def pose_of(R, t, z0, roll, pitch):
    return [float(t[0]), float(t[1]), float(z0)] + quat_rpy(roll, pitch, yaw_of(R))


def wheel_points(pose7):
    """doHeightInterpolate's four wheel points (icpTools.cpp:303-332): tf::Matrix3x3(q) in double stored to a float matrix,
    float matrix times float point; [4, 3] f32"""
    x, y, z, w = pose7[3:]
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    M = np.array([[1.0 - (yy + zz), xy - wz, xz + wy, pose7[0]], [xy + wz, 1.0 - (xx + zz), yz - wx, pose7[1]],
                  [xz - wy, yz + wx, 1.0 - (xx + yy), pose7[2]]]).astype(np.float32)
    out = []
    for i in (-1, 1):
        for j in (-1, 1):
            p = np.float32([i * 0.5, j * 0.5, -1.45])
            out.append([M[r, 0] * p[0] + M[r, 1] * p[1] + M[r, 2] * p[2] + M[r, 3] for r in range(3)])
    return np.array(out, np.float32)


def neighbour_margin(ground, pose7):
    """per wheel point: distance to the second-nearest finite ground point minus distance to the nearest (inf with fewer than two)"""
    g = np.asarray(ground, np.float64)[:, :3]
    g = g[np.isfinite(g).all(1)]
    out = []
    for q in wheel_points(pose7).astype(np.float64):
        d = np.sort(np.sqrt(((g - q) ** 2).sum(1)))
        out.append(d[1] - d[0] if len(d) > 1 else np.inf)
    return np.array(out)


ROLL_PITCH = (0.0, 0.03, -0.03, 0.1, -0.1)


def rot2(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, -s, s, c]


YAW_R = (("-3.0", rot2(-3.0)), ("-pi/2", [0.0, 1.0, -1.0, 0.0]), ("-0.7", rot2(-0.7)), ("0", [1.0, 0.0, 0.0, 1.0]), ("0.4", rot2(0.4)),
         ("pi/2 exactly", [0.0, -1.0, 1.0, 0.0]), ("2.5", rot2(2.5)), ("pi exactly", [-1.0, 0.0, 0.0, -1.0]))


def ground_patch(seed=41, side=28, pitch=0.25):
    """a tilted, slightly rough patch of ground under the robot: side^2 jittered lattice points, [n, 4] f32 (x, y, z, 0)"""
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[(np.arange(side) - (side - 1) / 2) * pitch] * 2, indexing="ij"), -1).reshape(-1, 2)
    g = g + rs.uniform(-0.09, 0.09, g.shape)
    z = -1.62 + 0.05 * g[:, 0] - 0.03 * g[:, 1] + rs.uniform(-0.01, 0.01, len(g))
    out = np.concatenate([g, z[:, None], np.zeros((len(g), 1))], 1).astype(np.float32)
    return out[rs.permutation(len(out))]


def rpy_cases():
    """(name, R[4], t[2], z0, roll, pitch) over ROLL_PITCH^2 x YAW_R, the position moving with the case.  A position is
    drawn again until every wheel point's second-nearest ground point is more than 2e-3 m farther than its nearest (the
    neighbour margin tests/test_ccicp_edge_cases.py then checks at 1e-3): a condition on the reference's inputs alone."""
    rs = np.random.RandomState(42)
    ground = ground_patch()
    for roll in ROLL_PITCH:
        for pitch in ROLL_PITCH:
            for name, R in YAW_R:
                for _ in range(50):
                    t, z0 = rs.uniform(-1.0, 1.0, 2).tolist(), float(rs.uniform(-0.2, 0.2))
                    if neighbour_margin(ground, pose_of(R, t, z0, roll, pitch)).min() > 2e-3:
                        break
                yield "roll %g pitch %g yaw %s" % (roll, pitch, name), R, t, z0, roll, pitch


UNDER = np.float32([[-0.5, -0.5], [-0.5, 0.5], [0.5, -0.5], [0.5, 0.5]])   # the wheel points of the identity pose, in their order
IDENTITY = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def indexed_ground(n, k, seed=43):
    """n ground points, the one nearest wheel point 0 of the identity pose at index k; the points under the other wheels
    follow wherever there is room (n = 1: the one point is everybody's nearest).  The other points lie 2.2 to 3.2 m from the centre."""
    rs = np.random.RandomState(seed + n)
    ang, rad = rs.uniform(0, 2 * np.pi, n), rs.uniform(2.2, 3.2, n)
    g = np.stack([rad * np.cos(ang), rad * np.sin(ang), -1.6 + rs.uniform(-0.05, 0.05, n)], 1)
    near = np.concatenate([UNDER + rs.uniform(-0.1, 0.1, (4, 2)), -1.6 + rs.uniform(-0.05, 0.05, (4, 1))], 1)
    g[k] = near[0]
    slots = [i for i in rs.permutation(n) if i != k][:3]
    for w, i in enumerate(slots):
        g[i] = near[1 + w]
    return g.astype(np.float32)


GROUND_SIZES = (1, 255, 256, 257, 1025)


def index_cases():
    for n in GROUND_SIZES:
        for k in sorted({0, 255, 256, n - 1}):
            if k < n:
                yield n, k


def gate_ground(inward, z0=0.0):
    """the 3 m gate (dd < 9.0f): wheel point 3 of the identity pose, (0.5, 0.5, float32(-1.45)), has its nearest ground point
    exactly 3 m away -- (3.5, 0.5, float32(-1.45)): the difference (3, 0, 0) and its square 9 are exact in float -- or one
    step of x nearer.  The other wheel points have theirs 2.5 m away, farther than 3 m from wheel point 3.  With a pose at
    height z0 the wheel points and the ground lie at float32(-1.45) + float32(z0), the sum the transform forms."""
    z = np.float32(-1.45) + np.float32(z0)
    x = np.nextafter(np.float32(3.5), np.float32(0)) if inward else np.float32(3.5)
    return np.array([[-3.0, -0.5, z], [-3.0, 0.5, z], [0.5, -3.0, z], [x, 0.5, z]], np.float32)


def degenerate_grounds():
    yield "one ground point under all four wheels", np.float32([[0.0625, -0.125, -1.5]])
    yield "four collinear points along x", np.float32([[-0.5, 0.0, -1.5], [-0.25, 0.0, -1.5], [0.25, 0.0, -1.5], [0.5, 0.0, -1.5]])
    yield "four collinear points, oblique", np.float32([[-0.5, -0.5, -1.625], [-0.25, -0.25, -1.5625], [0.25, 0.25, -1.4375], [0.5, 0.5, -1.375]])


# ------------------------------------------------------------------ GA classification cases
def ga_cases():
    """(name, pts [cap, 4] f32, count on the device)"""
    rs = np.random.RandomState(51)

    def blob(n, cx, cy, r=6.0):
        return np.concatenate([rs.uniform(-r, r, (n, 2)) + [cx, cy], rs.uniform(-2, 1, (n, 1)), np.zeros((n, 1))], 1).astype(np.float32)

    yield "all-negative coordinates", blob(700, -40.0, -30.0) - np.float32([0, 0, 5, 0]), 700
    yield "mixed signs", blob(700, 0.0, 0.0), 700
    z = blob(300, 0.0, 0.0, 1.0)
    z[:100, :3] = np.float32([0.0, -0.0, 0.0])
    z[100:200, :3] = np.float32([-0.0, 0.0, -0.0])
    z[200:, :3] = np.minimum(z[200:, :3], np.float32(-0.0))          # nothing above zero: the maxima are +-0.0
    yield "+-0.0", z, 300
    nz = blob(400, 10.0, -10.0)
    nz[::7, 2] = np.nan
    nz[3::7, 2] = np.inf
    nz[5, :3] = [250.0, 250.0, -np.inf]                               # flagged, and outside everybody else's extent
    yield "finite xy, non-finite z", nz, 400
    gone = blob(300, 0.0, 0.0)
    gone[:100, 0] += 400.0                                            # outside the 600 m lattice
    gone[100:200, 0] = np.nan
    gone[200:, 1] = np.float32(299.75)                                # an edge cell
    yield "every point dropped", gone, 300
    tail = blob(600, 5.0, 5.0)
    tail[400:, :2] += np.float32(200.0)
    yield "count below the capacity, outliers behind it", tail, 400
    yield "count 0", blob(300, 0.0, 0.0), 0
    for n in (255, 256, 257, 511, 512, 513):
        yield "n = %d" % n, blob(n, -3.0, 7.0, 2.5), n


def ga_disjoint_pair():
    """a block of 10 x 10 occupied cells, then points in the two rings of cells around it: were the first cloud's cells still
    occupied, the inner ring's points would count no empty neighbour (NGA) where alone they count three (GA)"""
    k = np.arange(10)
    a = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(-1, 2) * 0.5 + 0.25
    r = np.array([(i, j) for i in range(-2, 12) for j in range(-2, 12) if not (0 <= i < 10 and 0 <= j < 10)]) * 0.5 + 0.25
    f = lambda xy: np.concatenate([xy, np.zeros((len(xy), 2))], 1).astype(np.float32)
    return f(a), f(r)


# ------------------------------------------------------------------ packing cases
PACK_SIZES = (0, 1, 255, 4095, 4096, 4097, 9000)   # 4096 = one sweep of the pack kernel's grid (16 x 256)


def pack_cases():
    """(name, [(size, n_ga)] per scene)"""
    rs = np.random.RandomState(61)
    yield "one scene of 9000", [(9000, 0)]
    yield "one scene of 4097", [(4097, 4097)]
    yield "one empty scene", [(0, 0)]
    yield "two scenes", [(4096, 0), (4097, 4097)]
    yield "empty first, middle and last", [(0, 0), (255, 255), (0, 0), (4097, 0), (0, 0)][:5]
    sizes = [0] + [int(s) for s in rs.choice(PACK_SIZES, 30)] + [0]
    sizes[15] = 0
    yield "32 scenes", [(s, s if i % 2 else 0) for i, s in enumerate(sizes)]


# ------------------------------------------------------------------ the chain
CHAIN_RINGS = dict(k=0, rings=16, n_az=512)   # synth.make_cloud3d: 8192 rays
CHAIN_CLOUDS = ("rings", "rings and block")
CHAIN_CROPS = (None, (4.0, -3.0))
CHAIN_CROP_DIST = 12.0


def chain_block(seed=71, n=3000):
    """a filled block of obstacle points, 6 x 6 x 1.5 m, appended to the 16-ring cloud: its thin walls leave next to no voxel
    that is not ground adjacent, and the NGA class of the split would never meet a cap"""
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (n, 3)) * [6.0, 6.0, 1.5] + [8.0, -3.0, -1.0]).astype(np.float32)


FAR_RMAX = 1000.0   # ground segmentation's range for far_cloud (its default, 100 m, drops everything beyond)


def far_cloud(seed=81):
    """a ground disc around the sensor (the segmentation's seeds) and points 450 to 600 m out, outside the 600 m classification
    lattice: with FAR_RMAX some of them are obstacle points, and the classification drops every one"""
    rs = np.random.RandomState(seed)
    ang, rad = rs.uniform(0, 2 * np.pi, 3000), rs.uniform(450, 600, 3000)
    far = np.stack([rad * np.cos(ang), rad * np.sin(ang), rs.uniform(-1.0, 1.0, 3000)], 1)
    far = far[(np.abs(far[:, :2]) > 301).any(1)]
    ang, rad = rs.uniform(0, 2 * np.pi, 4000), rs.uniform(2, 60, 4000)
    gnd = np.stack([rad * np.cos(ang), rad * np.sin(ang), -1.73 + rs.normal(0, 0.01, 4000)], 1)
    return np.concatenate([gnd, far]).astype(np.float32)


def bin_order(obs, flags):
    """classifyPoints' order (icpTools.cpp:64-101): x bin major, y bin minor, cloud order inside a bin, dropped points gone;
    [n_kept, 4] f32 = x, y, z, ground_adj"""
    bx = np.floor((obs[:, 0].astype(np.float64) + 300.0) / 0.5).astype(np.int64)
    by = np.floor((obs[:, 1].astype(np.float64) + 300.0) / 0.5).astype(np.int64)
    kept = np.flatnonzero(flags != 255)
    order = kept[np.argsort((bx * 1200 + by)[kept], kind="stable")]
    return np.concatenate([obs[order, :3], (flags[order] == 1)[:, None].astype(np.float32)], 1)


def chain_reference(O, rings_xyz, cloud, voxel, crop):
    """the chain of slam_ccicp_scene_dev from oracle pieces (O: tests/oracle_lib, handed in; rings_xyz: the cloud of
    synth.make_cloud3d(**CHAIN_RINGS)): labels, obstacle and ground cloud, classification, the exact voxel filter or the bin
    order, crop and split -- uncapped (the tests cut it)"""
    xyz = np.concatenate([rings_xyz, chain_block()]) if cloud == "rings and block" else rings_xyz
    lab = O.gseg_segment(xyz)[0]
    obs, gnd = xyz[lab >= O.GSEG_OBSTACLE], xyz[lab == O.GSEG_GROUND]
    flags = O.classify_ga(obs)
    vox = voxel_exact(obs, flags) if voxel else None
    flt = np.concatenate([vox["fix"].astype(np.float32), vox["flag"][:, None]], 1) if voxel else bin_order(obs, flags)
    keep = O.ccicp_crop(flt, crop[0], crop[1], CHAIN_CROP_DIST) if crop is not None else np.ones(len(flt), bool)
    ga = flt[:, 3] > 0.5
    return dict(xyz=xyz, n_obs=len(obs), gnd=gnd, flt=flt, vox=vox, keep=keep, ga=np.flatnonzero(keep & ga), nga=np.flatnonzero(keep & ~ga))


def chain_caps(n_ga):
    return (1, 2, 50, n_ga, n_ga + 1, n_ga + 2)
