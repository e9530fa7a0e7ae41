"""Inputs shared by tests/test_vmap_oracle.py (the restatement against hand-worked values) and tests/test_gpu_vmap.py
(the device against the restatement).  LEAF = 0.25 is dyadic, so every voxel boundary below is an exact float."""
import numpy as np

LEAF = 0.25
F = np.float32
ULP_BELOW_LEAF = np.nextafter(F(0.25), F(0))       # 0.25 - ulp
U = 2.0 ** -20                                      # the unit of the sums


def boundary_points():
    """x at -0.25, -0.0, 0.0, 0.25 - ulp and 0.25 (y = z = 0.1): cells -1, 0, 0, 0, 1 on x; -0.0 and 0.0 share a voxel."""
    xs = np.array([-0.25, -0.0, 0.0, ULP_BELOW_LEAF, 0.25], F)
    pts = np.stack([xs, np.full(5, 0.1, F), np.full(5, 0.1, F)], axis=1)
    return pts, [-1, 0, 0, 0, 1]


def negative_points():
    """floor against truncation: -0.1 lies in cell -1 (truncation says 0), -0.3 in -2 (truncation: -1), 0.3 in 1 (both)."""
    xs = np.array([-0.1, -0.3, 0.3], F)
    pts = np.stack([xs, xs, xs], axis=1)
    return pts, [-1, -2, 1]


def rounding_points():
    """Three points of one voxel whose fixed-point values need both rounding rules.  x = 1/2, 3/2 and 5/2 units of 2^-20:
    rint to nearest even gives 0, 2 and 2 (half up would give 1, 2, 3; truncation 0, 1, 2), so S = 4 and the centroid is
    (float)((4.0 / 3.0) * 2^-20), a quotient that double rounds.  y = 1, 1, 2 units: S = 4 again.  z = 0.125 exactly."""
    xs = np.array([0.5 * U, 1.5 * U, 2.5 * U], F)
    ys = np.array([1 * U, 1 * U, 2 * U], F)
    pts = np.stack([xs, ys, np.full(3, 0.125, F)], axis=1)
    want_sums = (4, 4, 3 * (1 << 17))
    want_centroid = (F((4.0 / 3.0) * U), F((4.0 / 3.0) * U), F(0.125))
    return pts, want_sums, want_centroid


def dropped_points():
    """One good point and eight that the contract drops, each for its own reason."""
    big = F(2.0 ** 22)
    edge = F(2.0 ** 20 * LEAF)                       # its cell is 2^20: dropped; one ulp below is cell 2^20 - 1: kept
    rows = [(0.1, 0.1, 0.1),                         # kept
            (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf),
            (big, 0, 0), (0, -big, 0),
            (edge, 0, 0), (0, 0, -edge),             # cell -2^20: |cell| >= 2^20 as well
            (np.nextafter(edge, F(0)), 0, 0)]        # kept: the last cell
    return np.array(rows, F), 7


def cloud(n, seed, spread=12.0):
    """n points of a scene that fills voxels unevenly: a ground sheet, two walls, a dense blob and clutter; a tenth of the points are
    repeats of earlier ones (equal keys in neighbouring lanes, as a ring-ordered scan has)."""
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3), np.float64)
    p[:, 0] = rng.uniform(-spread, spread, n)
    p[:, 1] = rng.uniform(-spread, spread, n)
    p[:, 2] = rng.uniform(-1.5, 3.0, n)
    k = n // 3
    p[:k, 2] = -1.5 + 0.02 * rng.standard_normal(k)          # ground
    p[k:k + k // 2, 0] = spread * 0.8                          # a wall
    p[k + k // 2:2 * k, 1] = -spread * 0.6                     # another
    p[2 * k:2 * k + n // 5] = (1.1, -0.7, 0.4) + 0.15 * rng.standard_normal((n // 5, 3))   # a dense blob: voxels of many points
    if n >= 10:
        rep = rng.integers(0, n, n // 10)
        p[rep] = p[(rep + 1) % n]
    return p.astype(F)


def one_voxel(n, seed=3):
    """n points inside the voxel [0.5, 0.75)^3"""
    rng = np.random.default_rng(seed)
    return (0.5 + 0.2499 * rng.random((n, 3))).astype(F)


def transform(k):
    """A rigid transform (R [3, 3], t [3], f64) that is no special case: yaw, a little roll and pitch, metres of offset."""
    yaw, pitch, roll = 0.3 + 0.7 * k, 0.02 * (k + 1), -0.015 * (k + 1)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx, np.array([1.7 * k - 2.0, 0.9 - 1.3 * k, 0.11 * k])


SIZES = (0, 1, 63, 64, 65, 257)       # nothing, one lane, around a wavefront, more than one workgroup of 256
FOUR_CLOUDS = [(cloud(700 + 37 * k, 40 + k), transform(k)) for k in range(4)]
ORDERS = ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1))


def same_map(a, b):
    """two (xyz4, count, key[, sums]) extractions with the same bits"""
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                                    for x, y in zip(a, b))
