"""The clouds that the scan-context descriptor and search (docs/SCAN_CONTEXT.md) are held to their restatement on, shared by
tests/test_sc_oracle.py (CPU: the restatement against plain numpy, the mutations) and tests/test_gpu_sc.py (the device
against the restatement).  Every cloud is the smallest that reaches its edge; points keep more than 5 cm from each other
where they must survive a voxel filter of that leaf one by one."""
import numpy as np

from sc_oracle import Params

LEAF = 0.05                      # the leaf of the stores the edge clouds go into
# Small ranges: the store's voxel filter works on a dense lattice over the cloud's extent.  Ring widths are dyadic, so that
# f32 coordinates reach the ring edges exactly; coordinates of magnitude >= 0.5 pass the filter's 2^-24 fixed point unchanged.
_Z = dict(z_min=-0.5, z_step=0.005)
PARAM_SETS = {"twenty_by_64": Params(n_rings=20, n_sectors=64, max_range=5.0, **_Z),
              "one_ring_four_sectors": Params(n_rings=1, n_sectors=4, max_range=4.0, **_Z),
              "most": Params(n_rings=32, n_sectors=128, max_range=4.0, **_Z), "sixty": Params(n_rings=20, n_sectors=60, max_range=5.0, **_Z)}
VARIANTS = ("exact", "below", "above")


def _step(v, variant):
    v = np.float32(v)
    if variant == "below":
        return np.nextafter(v, np.float32(0.0))
    if variant == "above":
        return np.nextafter(v, np.float32(np.inf))
    return v


def _turn(px, py, q):
    """the point of quadrant q that the contract turns into (px, py) of the first"""
    return [(px, py), (-py, px), (-px, -py), (py, -px)][q]


def sector_ties(c, s, k, count=2):
    """f32 v in [1, 2) with v c[k] == v s[k] after rounding although c[k] != s[k]: px = py = v ties on the diagonal"""
    out = []
    for j in range(1, 1024):
        v = np.float32(1.0 + j / 1024.0)
        if float(v) * c[k] == float(v) * s[k]:
            out.append(v)
            if len(out) == count:
                break
    return out


def edge_cloud(p, tabs, variant):
    """[n, 3] f32: ring edges, axes, diagonals, the origin, table boundaries, range, non-finite, heights.  `variant` moves
    the ring-edge radii and the boundary points' py by one f32 ulp.  Each group has a height of its own."""
    edge2, c, s = tabs
    per = p.n_sectors // 4
    pts = []
    dr = p.max_range / p.n_rings
    for k in range(p.n_rings):                                # r2 on the ring edge: along the axes in turn
        e = _step((k + 1) * dr, variant)
        pts.append(_turn(e, np.float32(0.0), k % 4) + (0.0,))
    for k in range(3, p.n_rings, 4):                          # 3-4-5: x^2 + y^2 = e^2 without rounding where e / 5 is short
        e = (k + 1) * dr
        pts.append((_step(0.6 * e, variant), np.float32(0.8 * e), 0.1))
    h = 0.37 * dr                                             # inside ring 0 whatever the parameters
    for x, y in ((h, 0), (0, h), (-h, 0), (0, -h), (h, h), (-h, h), (-h, -h), (h, -h), (-0.0, 0.5 * h), (0.5 * h, -0.0),
                 (-0.0, -0.5 * h), (-0.5 * h, -0.0)):
        pts.append((np.float32(x), np.float32(y), 0.2))
    pts.append((0.0, 0.0, 0.3))                               # the origin: sector 0
    rad = 2.0                                                 # table boundaries: (c[k], s[k]) scaled by a power of two
    for k in range(1, per):
        px, py = np.float32(c[k] * rad), _step(s[k] * rad, variant)
        for q in range(4):
            pts.append(_turn(px, py, q) + (0.4,))
    if per % 2 == 0 and variant == "exact":                   # 45 degrees: products that tie exactly
        for n, v in enumerate(sector_ties(c, s, per // 2)):
            for q in range(4):
                pts.append(_turn(v * np.float32(0.5 + 0.5 * n), v * np.float32(0.5 + 0.5 * n), q) + (0.6,))
    pts.append((1.25 * p.max_range, 0.0, 0.0))                # beyond the last ring
    pts.append((0.0, np.float32(p.max_range), 0.0))           # on the last edge: dropped too
    pts += [(np.nan, 1.0, 0.0), (1.0, np.inf, 0.0), (1.0, 1.0, np.nan), (-np.inf, 1.0, 0.0)]
    top = p.z_min + 255 * p.z_step
    for n, z in enumerate((p.z_min - 0.5, p.z_min, p.z_min + 0.5 * p.z_step, p.z_min + 254 * p.z_step, top, top + 0.5)):
        a = 2.0 * np.pi * (n + 0.5) / 8.0                     # between the axes and the diagonals, two per quadrant
        pts.append((0.8 * p.max_range * np.cos(a), 0.8 * p.max_range * np.sin(a), z))
    return np.array(pts, dtype=np.float32)


def random_cloud(seed, n, p, spread=1.2):
    """n points in the disc of spread * max_range, heights around the descriptor's window"""
    rs = np.random.RandomState(seed)
    r = spread * p.max_range * np.sqrt(rs.uniform(0, 1, n))
    a = rs.uniform(0, 2 * np.pi, n)
    z = rs.uniform(p.z_min - 20 * p.z_step, p.z_min + 300 * p.z_step, n)
    return np.stack([r * np.cos(a), r * np.sin(a), z], axis=1).astype(np.float32)


def descriptor_clouds(p, tabs):
    """[(name, cloud)]: the three edge clouds, one of fewer points than a wavefront, one of more than a workgroup's threads"""
    out = [("edges_" + v, edge_cloud(p, tabs, v)) for v in VARIANTS]
    out.append(("ten_points", random_cloud(11, 10, p)))
    out.append(("two_thousand_points", random_cloud(12, 2000, p)))
    return out


def rotate_z(xyz, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return (np.asarray(xyz, np.float64) @ R.T).astype(np.float32)


def sector_point(p, ring, sector, z=0.0):
    """the middle of a cell"""
    r, a = (ring + 0.5) * p.max_range / p.n_rings, 2.0 * np.pi * (sector + 0.5) / p.n_sectors
    return (r * np.cos(a), r * np.sin(a), z)


def match_sets(p):
    """{name: [cloud, ...]}: the keyframes of one store each; every pair of a set is searched"""
    sets = {"one": [random_cloud(21, 300, p)], "two": [random_cloud(22, 300, p), random_cloud(23, 300, p)],
            "seventy": [random_cloud(100 + k, 200 + k, p, spread=0.5 + 0.01 * k) for k in range(70)]}
    same = random_cloud(24, 400, p)
    sets["identical"] = [same, same.copy()]
    # one occupied cell against two equal ones: the shifts that lay either on it tie, the lowest wins
    sets["tie"] = [np.array([sector_point(p, 2, 0)], np.float32), np.array([sector_point(p, 2, 2), sector_point(p, 2, p.n_sectors - 3)], np.float32)]
    sets["empty"] = [np.array([[2.0 * p.max_range, 0.0, 0.0], [0.0, -3.0 * p.max_range, 1.0]], np.float32), random_cloud(25, 300, p)]
    base = random_cloud(26, 500, p, spread=0.9)
    sets["rolled"] = [base, rotate_z(base, 5 * 2.0 * np.pi / p.n_sectors), rotate_z(base, -7 * 2.0 * np.pi / p.n_sectors)]
    return sets


# ---------------------------------------------------------------- plain numpy, nothing shared with the restatement
def numpy_descriptor(xyz, p, tabs):
    edge2, c, s = tabs
    a = np.asarray(xyz, np.float32).reshape(-1, 3)
    a = a[np.isfinite(a).all(axis=1)]
    x, y, z = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64), a[:, 2].astype(np.float64)
    ring = (edge2[None, :] <= (x * x + y * y)[:, None]).sum(axis=1)
    q = np.select([(x > 0) & (y >= 0), (x <= 0) & (y > 0), (x < 0) & (y <= 0), (x >= 0) & (y < 0)], [0, 1, 2, 3], default=-1)
    px = np.select([q == 0, q == 1, q == 2, q == 3], [x, y, -x, -y], default=1.0)
    py = np.select([q == 0, q == 1, q == 2, q == 3], [y, -x, -y, x], default=0.0)
    j = (py[:, None] * c[None, 1:] >= px[:, None] * s[None, 1:]).sum(axis=1)
    sector = np.where(q < 0, 0, np.maximum(q, 0) * (p.n_sectors // 4) + j)
    with np.errstate(over="ignore", invalid="ignore"):
        h = 1 + np.clip(np.floor((z - p.z_min) * (1.0 / p.z_step)), 0, 254).astype(np.int64)
    out = np.zeros((p.n_rings, p.n_sectors), np.int64)
    keep = ring < p.n_rings
    np.maximum.at(out, (ring[keep], sector[keep]), h[keep])
    return out.astype(np.uint8)


def numpy_distances(a, b):
    """D(s) for every shift"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.array([np.abs(a - np.roll(b, s, axis=1)).sum() for s in range(a.shape[1])])


def numpy_match(a, b):
    d = numpy_distances(a, b)
    s = int(np.argmin(d))                                     # the first minimum
    rb = np.roll(np.asarray(b), s, axis=1)
    return int(d[s]), s, int((np.asarray(a) != 0).sum()), int((rb != 0).sum()), int(((np.asarray(a) != 0) & (rb != 0)).sum())


# ---------------------------------------------------------------- place recognition on the synthetic loop
PLACE_LOOP, PLACE_MAX_RANGE = 48, 40.0


def place_clouds():
    """The loop of slam_amd.synth at 48 poses, 32 rings x 512 azimuths: the even poses are keyframes 0 .. 23; the odd ones, from
    other noise seeds and each turned about z by a seeded yaw, are the queries 24 .. 47, about 0.7 m from their two
    neighbours.  -> (keyframe clouds, their poses, query clouds, their poses, the yaws)"""
    from slam_amd import synth
    rs = np.random.RandomState(4711)
    kf, kf_pose, qs, q_pose, phis = [], [], [], [], []
    for k in range(PLACE_LOOP):
        if k % 2 == 0:
            xyz, pose = synth.make_cloud3d(k, PLACE_LOOP, rings=32, n_az=512)
            kf.append(xyz), kf_pose.append(pose)
        else:
            xyz, pose = synth.make_cloud3d(k, PLACE_LOOP, rings=32, n_az=512, seed_base=20000)
            phi = rs.uniform(-np.pi, np.pi)
            qs.append(rotate_z(xyz, phi)), q_pose.append(pose), phis.append(phi)
    return kf, kf_pose, qs, q_pose, phis


def place_check(match_row, j, kf_pose, q_pose, phi, n_sectors):
    """query j (pose 2 j + 1) against keyframes 0 .. 23: (the best keyframe is one of the two true neighbours, its shift is
    within one sector of (phi + th_kf - th_q) / (2 pi / n_sectors), nearest wrong distance / best distance)"""
    d = np.array([int(v) for v in match_row["distance"][:PLACE_LOOP // 2]])
    s = np.array([int(v) for v in match_row["shift"][:PLACE_LOOP // 2]])
    order = sorted(range(len(d)), key=lambda i: (d[i], i))
    best = order[0]
    true = (j, (j + 1) % (PLACE_LOOP // 2))
    want = (phi + kf_pose[best][2] - q_pose[j][2]) / (2.0 * np.pi / n_sectors)
    off = (s[best] - want) % n_sectors
    wrong = min(d[i] for i in range(len(d)) if i not in true)
    return best in true, min(off, n_sectors - off) <= 1.0, wrong / max(d[best], 1)
