"""Inputs shared by tests/test_vmap_gicp_oracle.py (the restatement against hand-worked values) and
tests/test_gpu_vmap_gicp.py (the device against the restatement): docs/VOXEL_MAP.md section 9."""
import numpy as np

import vmap_cases as K

F = np.float32
LEAVES = (0.25, 1.0)          # dyadic: every coordinate below is an exact float and L = leaf 2^20 exactly
EPS = 1e-3


def L_of(leaf):
    return int(np.rint(leaf * 2.0 ** 20))


def key_of(ix, iy, iz):
    return ((int(iz) + (1 << 20)) << 42) | ((int(iy) + (1 << 20)) << 21) | (int(ix) + (1 << 20))


def python_moments(points, leaf):
    """(E [3], M [6]) of points that all lie in one voxel, in Python's integers: fx = rint(v 2^20), d = fx - cell L,
    e = d >> 4 (Python's shift floors)."""
    L = L_of(leaf)
    E, M = [0, 0, 0], [0] * 6
    for p in np.asarray(points, F):
        e = []
        for v in p:
            fx = int(np.rint(np.float64(v) * 2.0 ** 20))
            cell = int(np.floor(np.float64(v) / leaf))
            e.append((fx - cell * L) >> 4)
        for k in range(3):
            E[k] += e[k]
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            M[k] += e[a] * e[b]
    return E, M


# ------------------------------------------------------------------ hand-worked voxels, each in a cell of its own
def negative_point(leaf):
    """One point at (-1/2, -5/4, -11/4) leaf: cells (-1, -2, -3), d = (1/2, 3/4, 1/4) L, e = d / 16."""
    L = L_of(leaf)
    p = np.array([[-0.5 * leaf, -1.25 * leaf, -2.75 * leaf]], F)
    e = (L // 32, 3 * L // 64, L // 64)
    M = (e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2], e[2] * e[2])
    return p, key_of(-1, -2, -3), e, M


def corner_point(leaf):
    """A point exactly on the corner of cell (1, -1, 0): d = 0 on every axis, so every moment is zero."""
    return np.array([[leaf, -leaf, 0.0]], F), key_of(1, -1, 0)


def square(leaf, cell=(4, 0, 0)):
    """Four coplanar axis-aligned points in z = cell + 1/2: C = diag(leaf^2 / 16, leaf^2 / 16, 0), no rotation is ever
    applied (every off-diagonal entry is zero), the normal is (0, 0, 1) and C' = diag(1, 1, eps) to the bit."""
    o = np.array(cell, np.float64) * leaf
    q = [(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)]
    return (o + np.array([(a * leaf, b * leaf, 0.5 * leaf) for a, b in q])).astype(F), key_of(*cell)


def line(leaf, cell=(6, 0, 0)):
    """Six points on a line along x: l1 = l2 = 0 < line_ratio l0, not a plane."""
    o = np.array(cell, np.float64) * leaf
    return (o + np.array([((1 + i) / 8.0 * leaf, 0.5 * leaf, 0.5 * leaf) for i in range(6)])).astype(F), key_of(*cell)


def blob(leaf, cell=(8, 0, 0)):
    """Six points at +- leaf / 4 on each axis about the cell's centre: C = leaf^2 / 48 I, l1 < flat_ratio l2, not a plane."""
    o = (np.array(cell, np.float64) + 0.5) * leaf
    d = 0.25 * leaf
    return (o + np.array([(d, 0, 0), (-d, 0, 0), (0, d, 0), (0, -d, 0), (0, 0, d), (0, 0, -d)])).astype(F), key_of(*cell)


def too_few(leaf, min_points=6, cell=(10, 0, 0)):
    """min_points - 1 coplanar points (a square and points on its diagonal): a plane by its shape, not by its count."""
    o = np.array(cell, np.float64) * leaf
    q = [(0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75), (0.5, 0.5), (0.375, 0.375), (0.625, 0.625)][:min_points - 1]
    return (o + np.array([(a * leaf, b * leaf, 0.5 * leaf) for a, b in q])).astype(F), key_of(*cell)


def negative_d_point():
    """Where floor differs from truncation in e: d < 0 needs cell L to lie beyond the point, which a dyadic leaf never
    gives (L is exact and fx >= cell L).  At leaf 0.7, L = rint(734003.2) = 734003 is short of the true edge, so for
    cell -10 the corner cell L = -7340030 lies above the true corner -7340032: the first float above -7.0 has cell -10,
    fx = rint(-7340031.5) = -7340032 (to even), d = -2, e = floor(-2 / 16) = -1 where truncation gives 0."""
    leaf = 0.7
    v = np.nextafter(F(-7.0), F(0))
    return leaf, np.array([[v, v, v]], F), key_of(-10, -10, -10), (-1, -1, -1)


def plane_patch(cell, normal_axis, leaf=1.0, n=3, offset=0.5):
    """n x n points of a plane perpendicular to an axis, inside the cell, at `offset` of the cell along that axis"""
    o = np.array(cell, np.float64) * leaf
    g = (np.arange(n) + 0.5) / n * leaf
    pts = []
    for a in g:
        for b in g:
            p = [a, b]
            p.insert(normal_axis, offset * leaf)
            pts.append(o + p)
    return np.array(pts, F)


SIZES = K.SIZES
FOUR_CLOUDS = K.FOUR_CLOUDS
ORDERS = K.ORDERS
