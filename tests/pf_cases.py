"""The particle filter (slam_pf_*, docs/PARTICLE_FILTER.md) restated in numpy, and the cases it is checked on.  No GPU, no
library.  The three tables (cos / sin pairs, Gaussian quantiles, weights) are inputs -- what the C-ABI's makers returned -- so libm
is not in question; every product and sum below is a numpy operation of its own, rounded on its own; everything behind them is
integer.  The score is tests/csm_plane_cases.score_poses.

  philox(c, key)                       Philox-4x32-10 from the published algorithm, vectorised over counters
  words(seed, p, t, purpose)           the four words of particles p at step t
  Filter                               predict, init_gaussian, update (weights, sums, decision, resampling), estimate
  resample_search / resample_direct    the resampling rule src(j) = min { i : C_i n > j W + r }, two independent forms
  RESAMPLE_CASES, loop_scenario(...)   the case lists
"""
import functools
import math

import numpy as np

import csm_plane_cases as P

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Q_LIMIT = (1 << 29) - 1
ONE = 65536
STEP_LIMIT = 1 << 20

# the three known answers: counter, key, output (they equal Random123's kat_vectors for philox4x32_10)
PHILOX_VECTORS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox(c, key):
    """c: [..., 4] counters, key: (k0, k1); [..., 4] uint32 words.  Ten rounds, the key bumped between them."""
    c = np.asarray(c, np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m32, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, p, t, purpose):
    """[len(p), 4] uint32: counter (p, t, purpose, 0), key (low, high half of seed)"""
    p = np.asarray(p, np.uint64).reshape(-1)
    c = np.zeros((len(p), 4), np.uint64)
    c[:, 0], c[:, 1], c[:, 2] = p, int(t) & MASK, int(purpose)
    return philox(c, (int(seed) & MASK, (int(seed) >> 32) & MASK))


# ------------------------------------------------------------------------------------------------------------- resampling
def clamp_weights(w):
    return np.minimum(np.asarray(w, np.int64), ONE)


def resample_search(w, r):
    """src [n] int64 by a search in the prefix sums; W = 0: the identity"""
    w = clamp_weights(w)
    n, C = len(w), np.cumsum(clamp_weights(w))
    W = int(C[-1])
    if W == 0:
        return np.arange(n, dtype=np.int64)
    target = np.arange(n, dtype=np.int64) * W + int(r) % W            # < 2^53
    return np.searchsorted(C * n, target, side="right").astype(np.int64)


def resample_direct(w, r, js=None):
    """the rule read off its definition, O(n) per output: for every j of js (all of them by default) the first i whose
    C_i n exceeds j W + r, the prefix sums built by a running Python integer"""
    w = [min(int(v), ONE) for v in np.asarray(w).tolist()]
    n, C, run = len(w), [], 0
    for v in w:
        run += v
        C.append(run)
    W = run
    js = range(n) if js is None else [int(j) for j in js]
    if W == 0:
        return np.array(list(js), np.int64)
    Cn = np.array([c * n for c in C], dtype=object) if n <= 4096 else np.array(C, np.int64) * n
    rr = int(r) % W
    out = []
    for j in js:
        t = j * W + rr
        out.append(int(np.argmax(Cn > t)))
    return np.array(out, np.int64)


def _ramp(n):
    return (np.arange(n, dtype=np.int64) * 37) % 1000


@functools.lru_cache(maxsize=None)
def resample_cases():
    """name -> uint32 weights"""
    out = {}
    rs = np.random.RandomState(11)
    for n in (1, 2, 255, 256, 257, 65537):
        out["random_%d" % n] = rs.randint(0, 65536, n)
        out["equal_%d" % n] = np.full(n, 300)
    out["full_262144"] = np.full(1 << 18, ONE)
    for n in (257, 65537):
        for name, at in (("first", 0), ("middle", n // 2), ("last", n - 1)):
            w = np.zeros(n, np.int64)
            w[at] = 12345
            out["one_%s_%d" % (name, n)] = w
        z = rs.randint(1, 65536, n)
        z[::2] = 0
        out["zeros_%d" % n] = z
        out["ramp_%d" % n] = _ramp(n)
    out["zero_sum_5"] = np.zeros(5, np.int64)
    return {k: np.ascontiguousarray(v, np.uint32) for k, v in out.items()}


def offsets_of(w):
    W = int(clamp_weights(w).sum())
    return (0, 1, max(W - 1, 0), W, W + 1)


# ------------------------------------------------------------------------------------------------------------- the filter
DEFAULTS = dict(n_particles=1024, n_angles=4096, gauss_bits=12, weight_len=1024, weight_shift=4, resample_num=1, resample_den=2,
                weight_scale=1024.0, seed=1)


def motion_ok(m):
    dx, dy, sx, sy, sk, dk = m
    return (all(math.isfinite(v) for v in (dx, dy, sx, sy, sk)) and sx >= 0.0 and sy >= 0.0 and 0.0 <= sk < STEP_LIMIT and
            -STEP_LIMIT < int(dk) < STEP_LIMIT)


class Filter:
    """cs [2 A] f64, G [2^b] f64, wtab [L] uint32: the tables in force.  State: x, y (f64), k (int64), acc (int64), t."""

    def __init__(self, cs, G, wtab, **params):
        self.p = dict(DEFAULTS, **params)
        n = self.p["n_particles"]
        self.cs, self.G, self.wtab = np.asarray(cs, np.float64), np.asarray(G, np.float64), np.asarray(wtab, np.int64)
        assert len(self.cs) == 2 * self.p["n_angles"] and len(self.G) == 1 << self.p["gauss_bits"] and len(self.wtab) == self.p["weight_len"]
        self.x, self.y, self.k, self.acc = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.w = np.zeros(n, np.int64)
        self.t, self.n_resamples, self.refused = 0, 0, 0
        self.last = None

    def set_particles(self, x, y, k):
        self.x, self.y, self.k = np.array(x, np.float64), np.array(y, np.float64), np.array(k, np.int64)
        self.acc = np.zeros(len(self.x), np.int64)

    def _draw(self, x, y, k, m, purpose):
        dx, dy, sx, sy, sk, dk = m
        w = words(self.p["seed"], np.arange(len(x)), self.t, purpose).astype(np.int64)
        sh = 32 - self.p["gauss_bits"]
        g0, g1, g2 = self.G[w[:, 0] >> sh], self.G[w[:, 1] >> sh], self.G[w[:, 2] >> sh]
        c, s = self.cs[2 * k], self.cs[2 * k + 1]
        with np.errstate(all="ignore"):
            ex = dx + sx * g0
            ey = dy + sy * g1
            nx = x + (c * ex - s * ey)
            ny = y + (s * ex + c * ey)
        nk = (k + int(dk) + np.rint(sk * g2).astype(np.int64)) & (self.p["n_angles"] - 1)
        return nx, ny, nk

    def predict(self, m):
        """m = (dx, dy, sx, sy, sk, dk); an invalid one is counted and skipped, as slam_pf_predict_dev does"""
        if not motion_ok(m):
            self.refused += 1
            return
        self.x, self.y, self.k = self._draw(self.x, self.y, self.k, m, 0)
        self.t = (self.t + 1) & MASK

    def init_gaussian(self, x, y, k, sx, sy, sk):
        n = self.p["n_particles"]
        self.x, self.y, self.k = self._draw(np.full(n, float(x)), np.full(n, float(y)), np.full(n, int(k), np.int64), (0.0, 0.0, sx, sy, sk, 0), 1)
        self.acc = np.zeros(n, np.int64)

    def scores(self, tabs, pts, n_ga, res, cx, cy):
        with np.errstate(all="ignore"):
            poses = np.stack([self.cs[2 * self.k], self.cs[2 * self.k + 1], self.x - cx, self.y - cy], axis=1)
        return P.score_poses(tabs, pts, n_ga, poses, res)[0].astype(np.int64)

    def update(self, tabs, pts, n_ga, res, cx=0.0, cy=0.0, score=None):
        """tabs, pts, n_ga, res as for csm_plane_cases.score_poses; score: given instead of computed.  Returns the state dict."""
        n = self.p["n_particles"]
        score = self.scores(tabs, pts, n_ga, res, cx, cy) if score is None else np.asarray(score, np.int64)
        self.acc = self.acc + score
        fin = np.isfinite(self.x) & np.isfinite(self.y)
        st = dict(t=self.t, n=n, resampled=0, degenerate=0, best=-1, A_max=0, W=0, S2=0, MX=0, MY=0, MC=0, MS=0)
        self.w = np.zeros(n, np.int64)
        if not fin.any():
            st["degenerate"] = 1
            return self._finish(st)
        A_max = int(self.acc[fin].max())
        d = np.minimum((A_max - self.acc) >> self.p["weight_shift"], self.p["weight_len"] - 1)
        self.w = np.where(fin, self.wtab[np.where(fin, d, 0)], 0).astype(np.int64)
        w = self.w

        def q(v):
            with np.errstate(all="ignore"):
                s = np.where(fin, v, 0.0) * 65536.0
            return np.where(s >= Q_LIMIT, Q_LIMIT, np.where(s <= -Q_LIMIT, -Q_LIMIT, np.rint(s))).astype(np.int64)

        qc, qs = np.rint(self.cs[2 * self.k] * 16777216.0).astype(np.int64), np.rint(self.cs[2 * self.k + 1] * 16777216.0).astype(np.int64)
        st.update(A_max=A_max, best=int(np.flatnonzero(fin & (self.acc == A_max))[0]), W=int(w.sum()), S2=int((w * w).sum()),
                  MX=int((w * q(self.x)).sum()), MY=int((w * q(self.y)).sum()), MC=int((w * qc).sum()), MS=int((w * qs).sum()))
        W, S2 = st["W"], st["S2"]
        if W * W * self.p["resample_den"] < self.p["resample_num"] * n * S2:
            w4 = words(self.p["seed"], [0], self.t, 2)[0]
            r = ((int(w4[0]) << 32) | int(w4[1])) % W
            src = resample_search(w, r)
            self.x, self.y, self.k = self.x[src], self.y[src], self.k[src]
            self.acc = np.zeros(n, np.int64)
            self.n_resamples += 1
            st["resampled"], st["src"] = 1, src
        return self._finish(st)

    def _finish(self, st):
        W = st["W"]
        if W:
            den = float(W) * 65536.0
            st["x"], st["y"], st["theta"] = float(st["MX"]) / den, float(st["MY"]) / den, math.atan2(float(st["MS"]), float(st["MC"]))
        else:
            st["x"] = st["y"] = st["theta"] = float("nan")
        st["n_resamples"], st["refused"] = self.n_resamples, self.refused
        self.last = st
        return st


# ---------------------------------------------------------------------------------------- the loop: filter against dead reckoning
LOOP = dict(size=500, res=0.1, sigma=0.2, R=6, n_loop=256, first=96, steps=20, A=4096,
            bias_dx=1.10, bias_dk=2,                      # the odometry: 10 % too long a step and two heading steps too many per scan
            init=(0.10, 0.10, 8.0), noise=(0.03, 0.03, 3.0), seeds=(1, 2, 3))


def loop_occupancy():
    """the occupancy plane of the synthetic room's map points by the grid's own cell rule: obstacle or unknown"""
    import csm_oracle as CO
    m_ga, m_nga = CO.synth_map()
    s = LOOP["size"]
    occ = np.full(s * s, -1, np.int8)
    x, y = P.grid_cells(np.concatenate([m_ga, m_nga]), s, s, LOOP["res"])
    occ[x + s * y] = 100
    return occ


@functools.lru_cache(maxsize=None)
def loop_plane():
    s = LOOP["size"]
    plane = P.likelihood_plane(loop_occupancy(), s, s, LOOP["res"], LOOP["sigma"], LOOP["R"])
    plane.setflags(write=False)
    return plane


@functools.lru_cache(maxsize=None)
def loop_scans():
    """per step i = 0 .. steps: (points, n_ga, true pose); heading steps of the loop are whole: 2 pi / 256 = 16 steps of 2 pi / 4096"""
    from slam_amd import synth
    out = []
    for i in range(LOOP["steps"] + 1):
        ga, nga, pose = synth.make_scan(LOOP["first"] + i, LOOP["n_loop"])
        out.append((np.concatenate([ga, nga]), len(ga), pose))
    return tuple(out)


def heading_index(theta, A):
    return int(round(theta / (2.0 * math.pi / A))) % A


def loop_odometry():
    """per step the biased motion (dx, dy, dk) in the old pose's frame, and the dead-reckoned poses (x, y, k) it gives from the
    true start, computed with the host's cos / sin (a yardstick, not a bit contract)"""
    scans, A = loop_scans(), LOOP["A"]
    x, y, th = scans[0][2]
    k = heading_index(th, A)
    dead, motions = [(x, y, k)], []
    for i in range(LOOP["steps"]):
        (x0, y0, t0), (x1, y1, t1) = scans[i][2], scans[i + 1][2]
        c, s = math.cos(t0), math.sin(t0)
        dx, dy = c * (x1 - x0) + s * (y1 - y0), -s * (x1 - x0) + c * (y1 - y0)
        dk = heading_index(t1, A) - heading_index(t0, A)
        m = (dx * LOOP["bias_dx"], dy, dk + LOOP["bias_dk"])
        motions.append(m)
        px, py, pk = dead[-1]
        a = 2.0 * math.pi * pk / A
        dead.append((px + math.cos(a) * m[0] - math.sin(a) * m[1], py + math.sin(a) * m[0] + math.cos(a) * m[1], (pk + m[2]) % A))
    return motions, dead


def run_loop(f, tabs, each=None):
    """f: a Filter (or anything with init_gaussian / predict / update of the same shape); returns per step (filter error,
    dead-reckoning error) in metres; each(i, f, state) is called after every update"""
    scans = loop_scans()
    motions, dead = loop_odometry()
    x, y, th = scans[0][2]
    f.init_gaussian(x, y, heading_index(th, LOOP["A"]), *LOOP["init"])
    errs = []
    for i in range(LOOP["steps"]):
        dx, dy, dk = motions[i]
        f.predict((dx, dy) + LOOP["noise"] + (dk,))
        pts, n_ga, (tx, ty, _) = scans[i + 1]
        st = f.update(tabs, pts, n_ga, LOOP["res"])
        if each:
            each(i, f, st)
        errs.append((math.hypot(st["x"] - tx, st["y"] - ty), math.hypot(dead[i + 1][0] - tx, dead[i + 1][1] - ty)))
    return errs
