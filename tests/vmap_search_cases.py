"""The exhaustive lattice pose search (slam_vmap_search*, docs/VOXEL_MAP.md section 13) restated in numpy and Python ints,
written from the contract, and the cases tests/test_vmap_search_cases.py (the restatement alone, no device) and
tests/test_gpu_vmap_search.py (the device against it, bit for bit) share.  Nothing of the library is used but the ctypes mirror of
the parameter struct.
  cells      section 1's rule: q = (float)(((r0 x + r1 y) + r2 z) + t) in double, cell = floor((double) q / leaf), a cell iff
             |q| < 2^22 and |cell| < 2^20 on every axis (tests/vmap_oracle.py's OracleMap is the check of this numpy form)
  qualifying the cells of an OracleMap's voxels with count >= min_count, or of an OracleDistMap's voxels with flag 1
  volume     volume_by_sets: one set lookup per (rotation, offset, point), the definition; volume_dense: the same integers by
             adding slices of a dense 0 / 1 array, for the scene, where the former would take minutes
  selection  greedy on (score, lowest flat index) with the cyclic suppression box
  relocalize MapLocalizer.relocalize on tests/map_localizer_cases.py's OracleLocalizer"""
import math

import numpy as np

import map_localizer_cases as ML
import vmap_oracle as V
from slam_amd import api

MUT_NONE, MUT_TRUNCATE, MUT_SUBTRACT, MUT_TIE_HIGH, MUT_NO_WRAP, MUT_COUNT_NO_CELL = range(6)
CELL_LIMIT, COORD_LIMIT = 1 << 20, 4194304.0
DEFAULTS = dict(yaw0=0.0, n_yaw=64, cx=0.0, cy=0.0, cz=0.0, wx=24, wy=24, wz=0, planes_only=1, min_count=6, top_m=4, nms_yaw=2, nms_cells=2)
MAX_POSES, MAX_HITS = 1 << 26, 4096


def params(**kw):
    """the defaults of slam_vmap_default_search_params, as a dict, with `kw` over them"""
    assert set(kw) <= set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def refused(p, n=0):
    """what slam_vmap_search refuses of the parameters and n alone"""
    if n < 0 or p["n_yaw"] < 1 or min(p["wx"], p["wy"], p["wz"]) < 0 or not 0 <= p["top_m"] <= MAX_HITS or min(p["nms_yaw"], p["nms_cells"]) < 0:
        return True
    return p["n_yaw"] * (2 * p["wx"] + 1) * (2 * p["wy"] + 1) * (2 * p["wz"] + 1) > MAX_POSES


def yaw_of(p, k):
    return np.float32(float(np.float32(p["yaw0"])) + 2.0 * math.pi * k / p["n_yaw"])


def rotation(p, k, x=None, y=None, z=None):
    """rotation k: planar(cx, cy, yaw_k) with cz as its z translation, 4 x 4 f32; x, y, z replace the centre (a hit's init)"""
    M = ML.planar(p["cx"] if x is None else x, p["cy"] if y is None else y, yaw_of(p, k))
    M[2, 3] = np.float32(p["cz"] if z is None else z)
    return M


def moved_cells(xyz, M, leaf, mutation=MUT_NONE):
    """(cells [n, 3] int64, has [n] bool) of the points [n, >= 3] f32 under the 4 x 4 f32 M at `leaf`"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, np.asarray(xyz).shape[-1] if np.asarray(xyz).ndim > 1 else 3)
    P, D = xyz[:, :3].astype(np.float64), np.asarray(M, np.float32).astype(np.float64)
    cells, has = np.zeros((len(P), 3), np.int64), np.ones(len(P), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            q = (((D[a, 0] * P[:, 0] + D[a, 1] * P[:, 1]) + D[a, 2] * P[:, 2]) + D[a, 3]).astype(np.float32)
            c = q.astype(np.float64) / float(leaf)
            c = np.trunc(c) if mutation == MUT_TRUNCATE else np.floor(c)
            ok = (np.abs(q) < np.float32(COORD_LIMIT)) & (np.abs(c) < float(CELL_LIMIT))        # a NaN fails both
            cells[:, a] = np.where(ok, c, 0.0).astype(np.int64)
            has &= ok
    return cells, has


def qualifying(omap, planes_only, min_count=6):
    """the set of (x, y, z) cells of the qualifying voxels of an OracleMap (count >= min_count) or OracleDistMap (flag 1)"""
    if planes_only:
        d = omap.read()
        key = d["key"][d["flag"] == 1]
    else:
        _, count, key, _ = omap.extract()
        key = key[count >= max(int(min_count), 0)]
    x, y, z = V.cells_of(key)
    return set(zip(x.tolist(), y.tolist(), z.tolist()))


def all_cells(xyz, p, leaf, mutation=MUT_NONE):
    """per rotation the cells of the points that count: [(cells [m, 3], n_with_cell)]"""
    out = []
    for k in range(p["n_yaw"]):
        c, has = moved_cells(xyz, rotation(p, k), leaf, mutation)
        out.append((c if mutation == MUT_COUNT_NO_CELL else c[has], int(has.sum())))
    return out


def volume_by_sets(xyz, qual, leaf, p, mutation=MUT_NONE):
    """the volume int32 [n_yaw, 2 wz + 1, 2 wy + 1, 2 wx + 1] and n_with_cell [n_yaw], by set lookups"""
    sign = -1 if mutation == MUT_SUBTRACT else 1
    vol = np.zeros((p["n_yaw"], 2 * p["wz"] + 1, 2 * p["wy"] + 1, 2 * p["wx"] + 1), np.int32)
    rots = all_cells(xyz, p, leaf, mutation)
    for k, (cells, _) in enumerate(rots):
        cells = [tuple(int(v) for v in c) for c in cells]
        for dz in range(-p["wz"], p["wz"] + 1):
            for dy in range(-p["wy"], p["wy"] + 1):
                for dx in range(-p["wx"], p["wx"] + 1):
                    s = 0
                    for x, y, z in cells:
                        t = (x + sign * dx, y + sign * dy, z + sign * dz)
                        s += max(abs(v) for v in t) < CELL_LIMIT and t in qual
                    vol[k, dz + p["wz"], dy + p["wy"], dx + p["wx"]] = s
    return vol, np.array([n for _, n in rots], np.int32)


def volume_dense(xyz, qual, leaf, p):
    """volume_by_sets' integers through a dense 0 / 1 array of the qualifying cells: per distinct cell of a rotation's points one
    slice of the array, times the points in that cell, is added"""
    w = np.array([p["wx"], p["wy"], p["wz"]], np.int64)
    rots = all_cells(xyz, p, leaf)
    vol = np.zeros((p["n_yaw"], 2 * p["wz"] + 1, 2 * p["wy"] + 1, 2 * p["wx"] + 1), np.int32)
    nwc = np.array([n for _, n in rots], np.int32)
    allc = np.concatenate([c for c, _ in rots]) if rots else np.zeros((0, 3), np.int64)
    if len(allc) == 0 or not qual:
        return vol, nwc
    lo, hi = allc.min(0) - w, allc.max(0) + w
    occ = np.zeros(tuple((hi - lo + 1)[::-1]), np.int32)                                       # [z, y, x]
    q = np.array(sorted(qual), np.int64).reshape(-1, 3)
    q = q[((q >= lo) & (q <= hi)).all(1)] - lo
    occ[q[:, 2], q[:, 1], q[:, 0]] = 1
    for k, (cells, _) in enumerate(rots):
        u, mult = np.unique(cells - lo - w, axis=0, return_counts=True)
        for (x, y, z), m in zip(u.tolist(), mult.tolist()):
            vol[k] += m * occ[z:z + 2 * p["wz"] + 1, y:y + 2 * p["wy"] + 1, x:x + 2 * p["wx"] + 1]
    return vol, nwc


def select(vol, nwc, leaf, p, mutation=MUT_NONE):
    """the hits of a volume: dicts of score, k, dx, dy, dz, n_with_cell and init (4 x 4 f32), best first"""
    left = np.array(vol, np.int64)
    n_yaw, Dz, Dy, Dx = left.shape
    hits = []
    for _ in range(p["top_m"]):
        best = int(left.max()) if left.size else 0
        if best <= 0:
            break
        at = np.flatnonzero(left.reshape(-1) == best)
        flat = int(at[-1] if mutation == MUT_TIE_HIGH else at[0])
        k, z, y, x = np.unravel_index(flat, left.shape)
        dx, dy, dz = int(x) - p["wx"], int(y) - p["wy"], int(z) - p["wz"]
        init = rotation(p, int(k), np.float32(float(np.float32(p["cx"])) + dx * float(leaf)), np.float32(float(np.float32(p["cy"])) + dy * float(leaf)),
                        np.float32(float(np.float32(p["cz"])) + dz * float(leaf)))
        hits.append(dict(score=best, k=int(k), dx=dx, dy=dy, dz=dz, n_with_cell=int(nwc[k]), init=init))
        for j in range(n_yaw):
            dk = abs(j - int(k))
            if mutation != MUT_NO_WRAP:
                dk = min(dk, n_yaw - dk)
            if dk <= p["nms_yaw"]:
                c = p["nms_cells"]
                left[j, max(z - c, 0):z + c + 1, max(y - c, 0):y + c + 1, max(x - c, 0):x + c + 1] = 0
    return hits


def search(xyz, qual, leaf, p, mutation=MUT_NONE, dense=False):
    """(hits, volume, n_with_cell) of one call"""
    vol, nwc = volume_dense(xyz, qual, leaf, p) if dense else volume_by_sets(xyz, qual, leaf, p, mutation)
    return select(vol, nwc, leaf, p, mutation), vol, nwc


def same_hits(a, b):
    return len(a) == len(b) and all(all(x[f] == y[f] for f in ("score", "k", "dx", "dy", "dz", "n_with_cell")) and
                                    np.asarray(x["init"], np.float32).tobytes() == np.asarray(y["init"], np.float32).tobytes() for x, y in zip(a, b))


def ctypes_params(p):
    return api.VmapSearchParams(**p)


# ------------------------------------------------------------------ the hand-worked case (test_vmap_search_cases.py enumerates it)
HAND_POINTS = np.array([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 2.5, 0.5)], np.float32)         # cells (0 0 0), (1 0 0), (0 2 0) at leaf 1
HAND_VOXELS = {(0, 0, 0), (1, 0, 0), (0, 2, 0), (-1, -1, 0)}
HAND_PARAMS = params(n_yaw=4, wx=1, wy=1, wz=0, top_m=8, nms_yaw=0, nms_cells=0)


# one point with a cell and four without: a NaN, an infinity, |v| >= 2^22 on either side
NO_CELL = np.array([(0.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (5e6, 0.5, 0.5), (0.5, 0.5, -4194304.0)], np.float32)


def four_fold():
    """a voxel set that a quarter turn about the z axis through the corner of cells maps onto itself: cell (x, y) -> (-y - 1, x)"""
    base = [(2, 0, 0), (2, 1, 0), (1, 2, 0)]
    out = set()
    for x, y, z in base:
        for _ in range(4):
            out.add((x, y, z))
            x, y = -y - 1, x
    return out


def cell_centres(cells, leaf=1.0):
    return np.array([((x + 0.5) * leaf, (y + 0.5) * leaf, (z + 0.5) * leaf) for x, y, z in sorted(cells)], np.float32)


def map_of(cells, leaf=1.0, per_voxel=1):
    """an OracleMap with `per_voxel` points at the centre of each of `cells`"""
    m = V.OracleMap(leaf)
    m.integrate(np.repeat(cell_centres(cells, leaf), per_voxel, axis=0))
    return m


# ------------------------------------------------------------------ the scene (section 9.5 / 11.4) and relocalize
def map_window(omap, leaf):
    """(cx, cy, w): the centre of the box of the map's voxels in x and y and the half-width in cells that covers it whole"""
    x, y, _ = V.cells_of(omap.read()["key"])
    lo, hi = np.array([x.min(), y.min()]) * leaf, (np.array([x.max(), y.max()]) + 1) * leaf
    c = (lo + hi) / 2
    return float(np.float32(c[0])), float(np.float32(c[1])), int(math.ceil(float((hi - lo).max()) / 2 / leaf)) + 1


def hit_offset(hit, truth):
    """(metres in x and y, radians of yaw) between a hit's init and the truth"""
    T = np.asarray(hit["init"], np.float64)
    dth = math.atan2(T[1, 0], T[0, 0]) - math.atan2(truth[1, 0], truth[0, 0])
    return float(np.hypot(T[0, 3] - truth[0, 3], T[1, 3] - truth[1, 3])), abs(math.atan2(math.sin(dth), math.cos(dth)))


def relocalize(ora, cloud, cx, cy, cz, radius, max_score, level=1, n_yaw=64, n_starts=4, hits=None, inits=None):
    """MapLocalizer.relocalize on an OracleLocalizer.  `hits`: taken instead of the restated search (the device's, where the
    device is held against this).  `inits[k][i]`: the f32 transform start i enters level k with (the device's, likewise); None:
    the restatement's own chain.  localize's dict with hits added."""
    n_source = ora.set_scan(cloud)
    leaf = ora.levels[level].leaf
    w = int(math.ceil(float(radius) / leaf))
    p = params(n_yaw=n_yaw, top_m=n_starts, cx=cx, cy=cy, cz=cz, wx=w, wy=w, wz=0)
    if hits is None:
        hits = search(ora.src.xyz, qualifying(ora.levels[level], True), leaf, p, dense=True)[0]
    last = [[None] * len(hits) for _ in ora.levels]
    if not hits:
        return dict(found=False, index=-1, transform=None, transform64=None, n_source=n_source, last=last, hits=hits)
    T, alive = [np.array(h["init"], np.float32) for h in hits], [True] * len(hits)
    for k in range(level, -1, -1):
        for i in range(len(T)):
            if inits is not None:
                if inits[k][i] is None:
                    continue
                r = last[k][i] = ora.register(k, inits[k][i])
            elif alive[i]:
                r = last[k][i] = ora.register(k, T[i])
                if r["state"] in ML.OUT:
                    alive[i] = False
                else:
                    T[i] = r["transform"]
    found = [r if r is not None and alive[i] else None for i, r in enumerate(last[0])]
    wi = ML.pick(found, n_source, max_score)
    return dict(found=wi >= 0, index=wi, transform=last[0][wi]["transform"] if wi >= 0 else None,
                transform64=last[0][wi]["transform64"] if wi >= 0 else None, n_source=n_source, last=last, hits=hits)
