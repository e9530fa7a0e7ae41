"""Inputs shared by tests/test_vmap_carve_oracle.py (the carve restatement against hand-worked rays) and the GPU tests that
hold the device to the restatement: the rays, with the cells each must visit, and the mover scene.  LEAF = 0.25 is dyadic."""
import numpy as np

import vmap_carve_oracle as VC
from slam_amd import synth

LEAF = 0.25
F = np.float32


def centre(cell, leaf=LEAF):
    """the centre of a cell as an f32 point"""
    return ((np.asarray(cell, np.float64) + 0.5) * leaf).astype(F)


def line(n, axis, sign):
    """the first n cells from cell 0 along +-axis"""
    out = np.zeros((n, 3), np.int64)
    out[:, axis] = sign * np.arange(n)
    return out


def diag(cells):
    return np.array(cells, np.int64).reshape(-1, 3)


# name -> (origin point, end point, parameters, the cells visited in order or None for a skipped ray), worked by hand from
# docs/VOXEL_MAP.md section 8: n = max |c1 - c0|, T = max(end_margin, ceil(n tail_num / tail_den)), steps 0 .. n - T - 1
RAYS = {}
for _k, _name in enumerate("xyz"):
    for _s, _sn in ((1, "plus"), (-1, "minus")):
        _c1 = np.zeros(3, np.int64)
        _c1[_k] = 4 * _s
        RAYS["axis_%s_%s" % (_sn, _name)] = (centre((0, 0, 0)), centre(_c1), VC.params(), line(3, _k, _s))      # n 4, T 1
RAYS.update({
    "diagonal": (centre((0, 0, 0)), centre((4, 4, 4)), VC.params(), diag([(0, 0, 0), (1, 1, 1), (2, 2, 2)])),
    # a_x = a_y = 4 > a_z = 2: x drives, y steps with it; z: e = 0 before step 1 (no move), 4 before step 2 (move)
    "tie_xy": (centre((0, 0, 0)), centre((4, 4, 2)), VC.params(), diag([(0, 0, 0), (1, 1, 0), (2, 2, 1)])),
    # the origin at -0.1: cell -1 by floor, 0 by truncation; the end at 0.8: cell 3.  n 4, T 1
    "through_zero": (np.full(3, -0.1, F), np.full(3, 0.8, F), VC.params(), diag([(-1, -1, -1), (0, 0, 0), (1, 1, 1)])),
    "n0": (centre((2, 1, 0)), centre((2, 1, 0)), VC.params(), diag([])),
    "n1": (centre((0, 0, 0)), centre((0, 1, 0)), VC.params(), diag([])),                                  # T 1 >= n
    "n_margin_plus_1": (centre((0, 0, 0)), centre((0, 0, 2)), VC.params(), diag([(0, 0, 0)])),            # n 2, T 1
    "n8": (centre((0, 0, 0)), centre((8, 0, 0)), VC.params(), line(7, 0, 1)),                             # T max(1, 1) = 1
    "n9": (centre((0, 0, 0)), centre((9, 0, 0)), VC.params(), line(7, 0, 1)),                             # T ceil(9 / 8) = 2
    "n16": (centre((0, 0, 0)), centre((16, 0, 0)), VC.params(), line(14, 0, 1)),                          # T 2
    "margin_eats_all": (centre((0, 0, 0)), centre((4, 0, 0)), VC.params(end_margin=5), diag([])),         # T 5 >= n 4
    "no_tail": (centre((0, 0, 0)), centre((16, 0, 0)), VC.params(tail_num=0), line(15, 0, 1)),            # T 1
    "n_max": (centre((0, 0, 0)), centre((512, 0, 0)), VC.params(), line(448, 0, 1)),                      # T 64
    "n_max_plus_1": (centre((0, 0, 0)), centre((513, 0, 0)), VC.params(), None),                          # skipped
})


def box_points(o, q, leaf=LEAF, pad=1):
    """one point at the centre of every cell of the box that holds the cells of o and q, padded by `pad` cells"""
    c0, c1 = np.floor(np.asarray(o, np.float64) / leaf).astype(np.int64), np.floor(np.asarray(q, np.float64) / leaf).astype(np.int64)
    lo, hi = np.minimum(c0, c1) - pad, np.maximum(c0, c1) + pad
    g = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
    return centre(g, leaf)


def skew_ray(n):
    """origin and end of a ray of n steps that moves on all three axes: cells (0, 0, 0) -> (n, n // 3, -(n // 5))"""
    return centre((0, 0, 0)), centre((n, n // 3, -(n // 5)))


# visited lengths at the edges of the 64-step chunks, with tail_num 0 and end_margin 1: L = n - 1
CHUNK_EDGE_LENGTHS = (63, 64, 65, 128, 129)


def crossed_cells(m):
    """the cells (sorted rows) of a map's voxels with miss > 0"""
    seen, miss, key = m.read_carve()
    import vmap_oracle as V
    c = np.stack(V.cells_of(key[miss > 0]), axis=1).reshape(-1, 3)
    return c[np.lexsort(c.T[::-1])] if len(c) else c


def sorted_rows(c):
    c = np.asarray(c, np.int64).reshape(-1, 3)
    return c[np.lexsort(c.T[::-1])] if len(c) else c


# ------------------------------------------------------------------ the mover scene
MOVER_SIZE, MOVER_HEIGHT = 1.0, 1.8
N_SCANS, RINGS, N_AZ, N_LOOP = 8, 16, 512, 50


def mover_centre(k):
    """where the moving pillar stands during scan k: 1.2 m further along x every scan, clear of the static pillars"""
    return -2.0 + 1.2 * k, -9.0


def mover_cloud(k, seed_base=9000, max_range=100.0):
    """synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512) in a world that also holds the mover (four segments, 1.8 m
    high above the ground): the same ray-cast, with a height per segment.  (xyz [n, 3] f32 in the sensor frame, pose)"""
    segs, _ = synth.world_segments()
    cx, cy = mover_centre(k)
    h = MOVER_SIZE / 2
    segs = np.concatenate([segs, np.array([(cx - h, cy - h, cx + h, cy - h), (cx + h, cy - h, cx + h, cy + h),
                                           (cx + h, cy + h, cx - h, cy + h), (cx - h, cy + h, cx - h, cy - h)])])
    top = np.full(len(segs), synth.GROUND_Z + synth.WALL_HEIGHT)
    top[-4:] = synth.GROUND_Z + MOVER_HEIGHT
    x, y, th = synth.true_pose(k, N_LOOP)
    rs = np.random.RandomState(seed_base + k)
    el = np.deg2rad(np.linspace(synth.RING_EL_DEG[0], synth.RING_EL_DEG[1], RINGS))
    az = np.deg2rad(np.arange(N_AZ) * (360.0 / N_AZ))
    EL, AZ = np.meshgrid(el, az, indexing="ij")
    EL, AZ = EL.ravel(), AZ.ravel()
    ce, se = np.cos(EL), np.sin(EL)
    dx, dy = np.cos(AZ + th), np.sin(AZ + th)
    px, py = segs[:, 0][None, :], segs[:, 1][None, :]
    ex, ey = (segs[:, 2] - segs[:, 0])[None, :], (segs[:, 3] - segs[:, 1])[None, :]
    den = dx[:, None] * ey - dy[:, None] * ex
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = ((px - x) * ey - (py - y) * ex) / den
        s = ((px - x) * dy[:, None] - (py - y) * dx[:, None]) / den
    r = rho / ce[:, None]
    z = r * se[:, None]
    ok = (np.abs(den) > 1e-12) & (rho > 1e-9) & (s >= 0) & (s <= 1) & (z >= synth.GROUND_Z) & (z <= top[None, :])
    r_wall = np.where(ok, r, np.inf).min(axis=1)
    with np.errstate(divide="ignore"):
        r_ground = np.where(se < 0, synth.GROUND_Z / se, np.inf)
    rng = np.minimum(r_wall, r_ground) + rs.normal(0.0, synth.NOISE_SIGMA, size=len(EL))
    keep = np.isfinite(rng) & (rng > 0.5) & (rng < max_range)
    rng, ce, se, AZ = rng[keep], ce[keep], se[keep], AZ[keep]
    xyz = np.stack([rng * ce * np.cos(AZ), rng * ce * np.sin(AZ), rng * se], axis=1).astype(F)
    return np.ascontiguousarray(xyz), (x, y, th)


_scene = None


def mover_scene():
    """[(cloud, pose, T)] for k = 0 .. 7, computed once: T is the truth transform into the first scan's frame, 4 x 4 f64"""
    global _scene
    if _scene is None:
        import vmap_oracle as V
        clouds = [mover_cloud(k) for k in range(N_SCANS)]
        _scene = [(c, p, V.truth_in_first_frame(clouds[0][1], p)) for c, p in clouds]
    return _scene


def ghost_mask(xyz, pose0, margin=0.1):
    """Which map points (first scan's frame) are ghosts: inside the mover's box at one of the scans 0 .. 6 and not inside
    its box at the last scan, boxes widened by `margin` for the range noise, from one voxel layer above the ground up (the
    ground under the mover is static: it is seen once the mover has gone)."""
    import vmap_oracle as V
    W = V.truth_in_first_frame((0.0, 0.0, 0.0), pose0)        # the first frame -> the world
    w = np.asarray(xyz, np.float64)[:, :3] @ W[:3, :3].T + W[:3, 3]
    h = MOVER_SIZE / 2 + margin

    def inside(k):
        cx, cy = mover_centre(k)
        return (np.abs(w[:, 0] - cx) <= h) & (np.abs(w[:, 1] - cy) <= h)
    body = (w[:, 2] > synth.GROUND_Z + 0.30) & (w[:, 2] <= synth.GROUND_Z + MOVER_HEIGHT + margin)
    earlier = np.zeros(len(w), bool)
    for k in range(N_SCANS - 1):
        earlier |= inside(k)
    return earlier & ~inside(N_SCANS - 1) & body
