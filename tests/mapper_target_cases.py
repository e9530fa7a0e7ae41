"""The streaming mapper's sliding-window ICP target (slam_amd/csrc/mapper.hip), restated in numpy from the rules its text
states, and the cases tests/test_gpu_mapper_target.py runs.  Shares no code with the kernels: every function names the
lines it restates.  Contract and bounds: docs/MAPPER_TARGET.md."""
import functools
import math

import numpy as np

from slam_amd import synth


# ------------------------------------------------------------------ the rules

def per_chunk_of(target_points, window_chunks):
    """mapper.hip:327 (stride_for): about target_points / (2 W) points of a class per chunk, never fewer than 64"""
    return max(64, target_points // max(2 * window_chunks, 1))


def stride_for(n, thin_res, target_points, window_chunks):
    """mapper.hip:324-329: no decimation when the window is thinned at rebuild time; else ceil(n / per_chunk), at least 1"""
    if thin_res > 0:
        return 1
    pc = per_chunk_of(target_points, window_chunks)
    return max(1, (n + pc - 1) // pc)


def registered(chunk, R, t):
    """mapper.hip:74-75: ((R0*x + R1*y) + t0, (R2*x + R3*y) + t1) in f64, every operation rounded on its own; per class
    in scan order: (ga[n,2], nga[m,2])"""
    ga, nga = [], []
    for s in range(chunk.n_scans):
        p = chunk.pts[chunk.scan_off[s]:chunk.scan_off[s + 1]]
        x, y = p[:, 0], p[:, 1]
        qx = (R[s, 0] * x + R[s, 1] * y) + t[s, 0]
        qy = (R[s, 2] * x + R[s, 3] * y) + t[s, 1]
        q = np.stack([qx, qy], 1)
        g = int(chunk.scan_nga[s])
        ga.append(q[:g])
        nga.append(q[g:])
    return np.concatenate(ga).reshape(-1, 2), np.concatenate(nga).reshape(-1, 2)


def window_points(chunk, R, t, stride_ga, stride_nga):
    """mapper.hip:51-77 (window_points_kernel): a class's points are ranked in scan order (GA: the GA points of earlier
    scans, then j; NGA: the NGA points of earlier scans, then j - n_ga_s); rank % stride == 0 is kept at rank // stride --
    every stride-th of the class's sequence, from its first"""
    ga, nga = registered(chunk, R, t)
    return ga[::stride_ga].copy(), nga[::stride_nga].copy()


class Thinned:
    def __init__(self, points, index, kept, stride):
        self.points, self.index, self.kept, self.stride = points, index, kept, stride


def thin(points, thin_res, grid_size, res, cap):
    """mapper.hip:79-164, 346-354 (ThinGeom, thin_cell, thin_min_kernel, thin_pick_kernel): a lattice of pitch thin_res over
    the grid's extent; per cell the point of the lowest window rank; the winners in rank order, every stride-th of them
    when they are more than cap.  points: [n,2] f64 in window order (oldest chunk first, scan order inside)."""
    gx, gy = (grid_size, grid_size) if np.isscalar(grid_size) else grid_size
    inv = 1.0 / thin_res
    nx, ny = int(math.ceil(gx * res * inv)), int(math.ceil(gy * res * inv))
    x0, y0 = -0.5 * gx * res, -0.5 * gy * res
    winner = {}                                   # cell -> lowest rank
    for i in range(len(points)):
        vx, vy = (float(points[i, 0]) - x0) * inv, (float(points[i, 1]) - y0) * inv
        if not (math.isfinite(vx) and math.isfinite(vy)):      # NaN, infinity: takes no part
            continue
        fx, fy = math.floor(vx), math.floor(vy)
        if not (0 <= fx < nx and 0 <= fy < ny):                # outside the lattice
            continue
        cell = int(fy) * nx + int(fx)
        if cell not in winner:                    # ranks only rise along the window: the first seen is the lowest
            winner[cell] = i
    index = np.array(sorted(winner.values()), np.int64)
    kept = len(index)
    stride = max(1, (kept + cap - 1) // max(cap, 1))
    index = index[::stride]
    assert len(index) == (kept + stride - 1) // stride
    return Thinned(np.asarray(points, np.float64).reshape(-1, 2)[index], index, kept, stride)


def target(prior_ga, prior_nga, window_entries, params):
    """mapper.hip:381-464 (collect_window, begin_rebuild) and :466-481 (adopt_build): the target a rebuild makes of the
    window's entries (all so far, oldest first: (ga, nga) as window_points gave them), or None when it comes to fewer than
    five points and the previous target stays.  params: window_chunks, keep_prior, thin_res, target_points, grid_size,
    resolution.  Returns (ga f64, nga f64, info)."""
    use = window_entries[-params["window_chunks"]:]
    if not use:
        return None
    p_ga = np.asarray(prior_ga, np.float64).reshape(-1, 2) if params["keep_prior"] else np.zeros((0, 2))
    p_nga = np.asarray(prior_nga, np.float64).reshape(-1, 2) if params["keep_prior"] else np.zeros((0, 2))
    w_ga, w_nga = np.concatenate([w[0] for w in use]), np.concatenate([w[1] for w in use])
    info = dict(segments=(sum(1 for w in use if len(w[0])), sum(1 for w in use if len(w[1]))), window=(len(w_ga), len(w_nga)))
    if params["thin_res"] > 0:
        cap = max(64, params["target_points"] // 2)
        out = []
        for name, prior, w in (("ga", p_ga, w_ga), ("nga", p_nga, w_nga)):
            if len(w) == 0:                       # the class's count stays the prior's
                out.append(prior)
                info[name] = dict(kept=0, stride=1, cap=cap, blocks=0)
                continue
            th = thin(w, params["thin_res"], params["grid_size"], params["resolution"], cap)
            out.append(np.concatenate([prior, th.points]))
            info[name] = dict(kept=th.kept, stride=th.stride, cap=cap, blocks=(len(w) + 255) // 256)
        ga, nga = out
    else:
        ga, nga = np.concatenate([p_ga, w_ga]), np.concatenate([p_nga, w_nga])
    if len(ga) + len(nga) < 5:
        return None
    return ga, nga, info


class Schedule:
    """mapper.hip:762-770 with strict_window = 1: a rebuild is due at push k when k > 0 and k - max(last, 0) >= rebuild_every;
    it reads chunks k-W .. k-1 and chunk k meets its target.  `last` moves whether or not the rebuild came to five points."""

    def __init__(self, window_chunks, rebuild_every=1):
        self.W, self.every, self.last = window_chunks, rebuild_every, -1

    def push(self, k):
        """the chunks the rebuild at push k reads, or None when none is due"""
        if not (self.W and k > 0 and k - max(self.last, 0) >= self.every):
            return None
        self.last = k
        return list(range(max(0, k - self.W), k))


# ------------------------------------------------------------------ chunks

def chunk_of(first, lens, ngas, beams, n_loop=256):
    """Scans first, first+1, ... of the loop with `beams` beams each, in beam order; scan i cut to lens[i] points (None: all
    it has) of which the first ngas[i] are class GA (None: as many as the scan's own pillar returns, which then come first)."""
    pts, off, nga, R, t, poses = [], [0], [], [], [], []
    for i, (n, g) in enumerate(zip(lens, ngas)):
        a, b, pose = synth.make_scan(first + i, n_loop, n_beams=beams, all_nga=g is not None)
        p = np.concatenate([a, b])
        n = len(p) if n is None else n
        g = len(a) if g is None else g
        assert g <= n <= len(p), (first + i, g, n, len(p))
        pts.append(p[:n])
        off.append(off[-1] + n)
        nga.append(g)
        Rk, tk = synth.pose_to_Rt(*synth.init_pose(first + i, pose))
        R.append(Rk.reshape(4))
        t.append(tk)
        poses.append(pose)
    S = len(lens)
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)).reshape(-1, 2), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(R).reshape(S, 4), np.array(t).reshape(S, 2), np.array(poses).reshape(S, 3))


def chunk_with_totals(first, n_scans, beams, n_ga, n_nga):
    """a chunk of n_scans scans whose classes hold exactly n_ga and n_nga points, dealt over the scans as evenly as they go"""
    g = [n_ga // n_scans + (1 if i < n_ga % n_scans else 0) for i in range(n_scans)]
    m = [n_nga // n_scans + (1 if i < n_nga % n_scans else 0) for i in range(n_scans)]
    return chunk_of(first, [a + b for a, b in zip(g, m)], g, beams)


def class_totals(chunk):
    n_ga = int(chunk.scan_nga.sum())
    return n_ga, chunk.n_points - n_ga


class Case:
    def __init__(self, name, reaches, chunks, **params):
        self.name, self.reaches, self._chunks = name, reaches, chunks
        self.params = dict(window_chunks=2, rebuild_every=1, target_points=8000, keep_prior=1, thin_res=0.0,
                           grid_size=400, resolution=0.1)
        self.params.update(params)

    @functools.lru_cache(maxsize=None)
    def chunks(self):
        return self._chunks()

    def __repr__(self):
        return self.name


PRIOR_POINTS = 2000
STRIDE_TARGET = 256             # W = 2: per_chunk = max(64, 256 // 4) = 64
STRIDE_TOTALS = [(127, 63), (128, 64), (129, 65), (64, 129), (65, 127)]     # (GA, NGA) per chunk: per_chunk -1, 0, +1 and twice that
BLOCK_TOTALS = [(257, 255), (255, 256), (513, 257), (256, 513), (1, 300)]   # the pick's 256-point block, both classes
MANY_SCANS = 31                 # 2 chunks of 31 scans of 1081 beams: more than 65 536 points of one class in the window


def _stride_chunks():
    return [chunk_with_totals(3 * k, 2, 141, a, b) for k, (a, b) in enumerate(STRIDE_TOTALS)]


def _empty_scan_chunks():
    # per chunk: a scan of both classes, one without GA points, an EMPTY one in the middle, one without NGA points, an empty one last
    return [chunk_of(5 * k, [61, 61, 0, 61, 0], [20, 0, 0, 61, 0], 81) for k in range(4)]


def _block_chunks():
    return [chunk_with_totals(4 * k, 4, 241, a, b) for k, (a, b) in enumerate(BLOCK_TOTALS)]


def _many_chunks():
    full = synth.make_batch(2 * MANY_SCANS, n_loop=256, all_nga=True)
    out = []
    for s0 in (0, MANY_SCANS):
        o, e = full.scan_off[s0], full.scan_off[s0 + MANY_SCANS]
        out.append(synth.ScanBatch(full.pts[o:e], (full.scan_off[s0:s0 + MANY_SCANS + 1] - o).astype(np.int32),
                                   full.scan_nga[s0:s0 + MANY_SCANS], full.R[s0:s0 + MANY_SCANS], full.t[s0:s0 + MANY_SCANS],
                                   full.true_poses[s0:s0 + MANY_SCANS]))
    out.append(chunk_of(2 * MANY_SCANS, [None], [None], 181))
    return out


def _natural(n_chunks, scans, beams, ga=None):
    """consecutive scans of the loop; ga: the first `ga` points of every scan are class GA (None: its pillar returns)"""
    return lambda: [chunk_of(scans * k, [None] * scans, [ga] * scans, beams) for k in range(n_chunks)]


def _all_nga_chunks():
    return [chunk_of(2 * k, [None, None], [0, 0], 181) for k in range(3)]


def _too_few_chunks():
    return [chunk_of(0, [4], [3], 61), chunk_of(1, [30], [10], 61), chunk_of(2, [30], [10], 61)]


CASES = [
    Case("strides 1, 2, 3 around per_chunk", "a class's per-chunk count at per_chunk - 1, per_chunk, per_chunk + 1 (and 2 per_chunk + 1)",
         _stride_chunks, target_points=STRIDE_TARGET),
    Case("empty scans, prior kept", "ga_before and the scan search on equal offsets; the prior in front", _empty_scan_chunks,
         target_points=400),
    Case("empty scans, no prior", "ga_before and the scan search on equal offsets; the window alone", _empty_scan_chunks,
         target_points=400, keep_prior=0),
    Case("class totals 255, 256, 257, 513", "the pick's block boundary, ballot and wave prefix", _block_chunks, window_chunks=1, thin_res=0.1),
    Case("more than 65 536 points", "more than kThinGrid blocks; the scan's second round and its carry", _many_chunks, thin_res=0.1),
    Case("eight segments and the ring's wrap", "Segs full, seg_point over eight segments, ring wrap", _natural(13, 2, 121, ga=30),
         window_chunks=8, thin_res=0.1),
    Case("the extent cuts the room", "points outside the lattice take no part", _natural(4, 3, 721), thin_res=0.1, grid_size=320),
    Case("six rebuilds in a row", "the winners put their lattice cells back", _natural(7, 2, 181, ga=40), thin_res=0.1),
    Case("no GA point in the window", "the class's count stays the prior's", _all_nga_chunks, thin_res=0.1),
    Case("fewer than five points, not thinned", "the previous target stays (cap_ga + cap_nga < 5)", _too_few_chunks, window_chunks=1, keep_prior=0),
    Case("fewer than five points, thinned", "the previous target stays (the build's count from the device)", _too_few_chunks, window_chunks=1,
         keep_prior=0, thin_res=0.1),
    Case("a rebuild every third chunk", "which chunks a target holds between rebuilds", _natural(10, 1, 121), rebuild_every=3, target_points=600),
]
SAME_BITS_CASE = "six rebuilds in a row"


def case(name):
    return next(c for c in CASES if c.name == name)


def cap_edge_chunks():
    """the cap edge: chunk 0 decides K (the cells its NGA points occupy), chunk 1 meets the target made of it"""
    return [chunk_of(0, [None] * 3, [None] * 3, 541), chunk_of(3, [None], [None], 121)]
