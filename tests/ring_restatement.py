"""Host restatement (numpy) of the two ring searches of the batch ICP kernels on the cell index (icp_search.hpp:
nn_search_impl, nn_search_seeded_impl), for COUNTING: which model points a query's search evaluates, whether it took the
probe, the chords or the one-pass seeded form.  Not an oracle of the neighbour (the brute-force arbiter is); used by
test_gpu_icp_ring_prune.py to prove its inputs reach the pruning code and by tools/exp/ring_reads.py for the read counts."""
import numpy as np

F = np.float32
PROBE_FROM_LEVEL = 2   # kProbeFromLevelBatch
SEED_ROWS_MAX = 12     # kSeedRowsMax


class Lattice:
    """plan_core (icp_build.hip): origin at the f32 minimum of all model points, pitch as index_info() reports it."""

    def __init__(self, info, all_xy):
        xy = np.asarray(all_xy, F).reshape(-1, 2)
        self.nx, self.ny = int(info["nx"]), int(info["ny"])
        self.h = F(info["cell"])
        self.inv_h = F(1.0) / self.h
        self.x0, self.y0 = xy[:, 0].min(), xy[:, 1].min()
        maxabs = np.abs(xy).max()
        self.margin = max(self.h * F(0.0009765625), F(maxabs) * F(1.9073486328125e-06))

    def frac(self, q):
        q = np.asarray(q, F)
        return (q[..., 0] - self.x0) * self.inv_h, (q[..., 1] - self.y0) * self.inv_h


class CellIndex:
    """The points of one class sorted by cell (row-major), start[] per cell."""

    def __init__(self, L, xy):
        self.L = L
        xy = np.asarray(xy, F).reshape(-1, 2)
        fx, fy = L.frac(xy)
        cx = np.clip(np.floor(fx).astype(int), 0, L.nx - 1)
        cy = np.clip(np.floor(fy).astype(int), 0, L.ny - 1)
        self.order = np.lexsort((np.arange(len(xy)), cx, cy))
        self.pts = xy[self.order]
        self.start = np.searchsorted((cy * L.nx + cx)[self.order], np.arange(L.nx * L.ny + 1))

    def span(self, y, xl, xh, q):
        """(points read, least squared distance) of cells xl..xh of row y"""
        if xl > xh:
            return 0, np.inf
        a, e = self.start[y * self.L.nx + xl], self.start[y * self.L.nx + xh + 1]
        if e <= a:
            return 0, np.inf
        d = self.pts[a:e] - q
        return int(e - a), float((d * d).sum(1).min())

    def nearest(self, q):
        """positions (in the sorted array) of the nearest point of every query, by brute force"""
        q = np.asarray(q, F).reshape(-1, 2)
        out = np.empty(len(q), int)
        for o in range(0, len(q), 256):
            d = q[o:o + 256, None, :] - self.pts[None, :, :]
            out[o:o + 256] = (d * d).sum(2).argmin(1)
        return out


def chord(fx, fy, y, Rd, x_lo, x_hi):
    """row_chord (icp_search.hpp)"""
    dy = max(y - fy, fy - (y + 1), 0.0)
    half = np.sqrt(max(Rd * Rd - dy * dy, 0.0)) + 1e-3
    return max(x_lo, int(np.floor(fx - half))), min(x_hi, int(np.floor(fx + half)))


def _radius(L, d2):
    return (np.sqrt(d2) + float(L.margin)) / float(L.h)


def unseeded(ix, q, new=True, gate=np.inf, best=np.inf, rp=-1, count=None):
    """nn_search_impl for one query: returns (points read, least squared distance); `count` (a dict) gains
    'probed' (levels probed) and 'clipped' (rows whose chord drops a cell the square holds).  new=False: the form before
    the probe and the chords.  best / rp: start from a candidate and a visited square (the seeded ring loop)."""
    L = ix.L
    count = count if count is not None else {}
    q = np.asarray(q, F)
    fx, fy = (float(v) for v in L.frac(q))
    cx, cy = min(max(int(np.floor(fx)), 0), L.nx - 1), min(max(int(np.floor(fy)), 0), L.ny - 1)
    reads = 0
    if rp < 0:
        reads, d = ix.span(cy, cx, cx, q)
        best = min(best, d)
        rp = 0
    r = rp + 1 if rp > 0 else 1
    while True:
        yl, yh, xl, xh = max(cy - r, 0), min(cy + r, L.ny - 1), max(cx - r, 0), min(cx + r, L.nx - 1)
        covers = xl == 0 and yl == 0 and xh == L.nx - 1 and yh == L.ny - 1
        cand = best
        if new and cand == np.inf and r >= PROBE_FROM_LEVEL:
            count["probed"] = count.get("probed", 0) + 1
            for y in range(yl, yh + 1):
                row = y * L.nx
                if cy - rp <= y <= cy + rp:
                    l1, f2 = min(xh, cx - rp - 1), max(xl, cx + rp + 1)
                    js = []
                    if xl <= l1 and ix.start[row + l1 + 1] > ix.start[row + xl]:
                        js.append(ix.start[row + l1 + 1] - 1)
                    if f2 <= xh and ix.start[row + xh + 1] > ix.start[row + f2]:
                        js.append(ix.start[row + f2])
                else:
                    a, e = ix.start[row + xl], ix.start[row + xh + 1]
                    c = ix.start[row + min(max(cx, xl), xh)]
                    js = [min(c, e - 1), max(c - 1, a)] if e > a else []
                for j in js:
                    d = ix.pts[j] - q
                    cand = min(cand, float((d * d).sum()))
                    reads += 1
        Rd = None
        if cand < np.inf:
            Rd = _radius(L, cand)
            xl, xh = max(xl, int(np.floor(fx - Rd))), min(xh, int(np.floor(fx + Rd)))
            yl, yh = max(yl, int(np.floor(fy - Rd))), min(yh, int(np.floor(fy + Rd)))
        for y in range(yl, yh + 1):
            lo, hi = xl, xh
            if new and Rd is not None:
                lo, hi = chord(fx, fy, y, Rd, xl, xh)
                if (lo > xl or hi < xh) and xl <= xh:
                    count["clipped"] = count.get("clipped", 0) + 1
            if cy - rp <= y <= cy + rp:
                spans = ((lo, min(hi, cx - rp - 1)), (max(lo, cx + rp + 1), hi))
            else:
                spans = ((lo, hi),)
            for a_, b_ in spans:
                n, d = ix.span(y, a_, b_, q)
                reads += n
                best = min(best, d)
        bound = r * float(L.h) - float(L.margin)
        if covers or best < bound * bound or bound * bound >= gate:
            break
        rp = r
        r *= 2
    return reads, best


def seeded(ix, q, seed, new=True, gate=np.inf, count=None):
    """nn_search_seeded_impl for one query with last iteration's neighbour `seed` (position in the sorted array): returns
    (points read, least squared distance); `count` gains 'small' (the 3 x 3 path), 'big' (a larger disk), 'onepass' and
    'clipped'."""
    L = ix.L
    count = count if count is not None else {}
    q = np.asarray(q, F)
    fx, fy = (float(v) for v in L.frac(q))
    d = ix.pts[seed] - q
    best = float((d * d).sum())
    R = _radius(L, best)
    xl, xh = max(0, int(np.floor(fx - R))), min(L.nx - 1, int(np.floor(fx + R)))
    yl, yh = max(0, int(np.floor(fy - R))), min(L.ny - 1, int(np.floor(fy + R)))
    if xh - xl <= 2 and yh - yl <= 2 and xl <= xh and yl <= yh:
        count["small"] = count.get("small", 0) + 1
        reads = 0
        for y in range(yl, yh + 1):
            n, d2 = ix.span(y, xl, xh, q)
            reads += n
            best = min(best, d2)
        return reads, best
    count["big"] = count.get("big", 0) + 1
    if new and SEED_ROWS_MAX > 0 and yh - yl < SEED_ROWS_MAX and xl <= xh and yl <= yh:
        count["onepass"] = count.get("onepass", 0) + 1
        cy = min(max(int(np.floor(fy)), 0), L.ny - 1)
        ym = min(max(cy, yl), yh)
        Rd, reads, k = R, 0, 0
        while ym - k >= yl or ym + k <= yh:
            a, b = max(yl, int(np.floor(fy - Rd))), min(yh, int(np.floor(fy + Rd)))
            if ym - k < a and ym + k > b:
                break
            for y in ((ym,) if k == 0 else (ym - k, ym + k)):
                if y < a or y > b:
                    continue
                lo, hi = chord(fx, fy, y, Rd, xl, xh)
                if lo > xl or hi < xh:
                    count["clipped"] = count.get("clipped", 0) + 1
                n, d2 = ix.span(y, lo, hi, q)
                reads += n
                best = min(best, d2)
            Rd = _radius(L, best)
            k += 1
        return reads, best
    return unseeded(ix, q, new, gate, best=best, rp=-1, count=count)
