"""A certificate for every executed ICP step (host only: numpy and the CPU oracle).

Every fit form writes, per scan and executed step, R, t, delta and n_corr into d_trace (slam_icp_fit_batch_dev).  certify()
takes the pose the DEVICE had before step k -- the initial pose, or row k - 1 exactly as written -- and runs ONE step of the
oracle from it with the brute-force arbiter (lowest original index on a tie) and the reference's gate.  Device and oracle then
form the same float queries, must choose the same correspondences and differ only in the order of their f64 sums: n_corr must be
equal and the pose within STEP_TOL, five orders of magnitude below what a chain-end comparison can ask (docs/ICP_STEP_CERTIFICATE.md).
No step is skipped and no other neighbour search is tried.

The module also restates both closed-form steps from a given correspondence list in long double (p2p_step, p2l_step), so that
tests can MUTATE the correspondences and ask what a wrong neighbour does to a row (tests/test_icp_step_certificate.py).
"""
import numpy as np

import oracle_lib as O

# |device - oracle| allowed on each of R, t and delta of one step taken from a shared pose.
#   point-to-point: the bound the project already holds whole chains to (test_gpu_icp.py, test_gpu_icp_spread.py): one step from a
#     shared pose cannot deviate more than a chain does.
#   point-to-line: ten times the largest deviation measured over every form and case on an MI355X, 3.22e-15 (the spread form with
#     staged tiles; docs/ICP_STEP_CERTIFICATE.md); the margin is for the order of the sums, which changes with CU count and launch
#     shape.  It is 1 / 1 800 000 of the smallest effect of a swapped neighbour on these inputs (6.0e-8).
STEP_TOL = {O.MODE_P2P: 1e-9, O.MODE_P2L: 10 * 3.22e-15}
MIN_SCAN_POINTS = 5       # icp.cpp:100-103


class CertificateError(AssertionError):
    """what: 'n_corr' | 'pose' | 'delta' | 'iters' | 'result' | 'unwritten' | 'too_few'"""

    def __init__(self, what, scan, step, detail):
        super().__init__("scan %d step %s: %s: %s" % (scan, step, what, detail))
        self.what, self.scan, self.step = what, scan, step


def _same(a, b):
    """equal values, NaN equal to NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def pose_before(batch, trace, s, k):
    if k == 0:
        return np.array(batch.R[s], np.float64).reshape(2, 2), np.array(batch.t[s], np.float64)
    return trace[s, k - 1, :4].reshape(2, 2).copy(), trace[s, k - 1, 4:6].copy()


def certify(model, batch, trace, result, max_iter, min_delta, indist, mode, R=None, t=None, fill=np.nan, tol=None, scans=None):
    """Holds every executed step of every scan to the oracle's step from the device's own previous pose, and the iteration rule
    to the device's own deltas.  trace[S, >= max_iter, 8] must have been filled with `fill` before the fit; R, t (optional) are
    the poses the fit left; `scans` restricts the check to some scans (the mutation tests).  Raises CertificateError; returns the
    largest |device - oracle| seen on R, t and delta."""
    tol = STEP_TOL[mode] if tol is None else tol
    trace = np.asarray(trace, np.float64)
    worst = 0.0
    for s in (range(batch.n_scans) if scans is None else scans):
        ga, nga = batch.scan(s)
        iters = int(result["iters"][s])
        R0, t0 = pose_before(batch, trace, s, 0)
        if len(ga) + len(nga) < MIN_SCAN_POINTS:
            if iters != 0:
                raise CertificateError("too_few", s, None, "iters %d for a scan of %d points" % (iters, len(ga) + len(nga)))
            if not all(_same(row, np.full(8, fill)) for row in trace[s]):
                raise CertificateError("unwritten", s, None, "a row was written for a scan of fewer than 5 points")
            if R is not None and not (_same(np.reshape(R[s], 4), R0.reshape(4)) and _same(t[s], t0)):
                raise CertificateError("too_few", s, None, "the pose of a scan of fewer than 5 points was touched")
            continue
        if not 1 <= iters <= max_iter:
            raise CertificateError("iters", s, None, "%d executed steps with max_iter %d" % (iters, max_iter))
        for k in range(iters):
            Rk, tk = pose_before(batch, trace, s, k)
            d, Ro, to, nc, _ = model.fit_step(ga, nga, Rk, tk, O.icp_params(1, -1.0, indist, O.NN_BRUTE, mode))
            row = trace[s, k]
            if not row[7] == nc:
                raise CertificateError("n_corr", s, k, "device %r oracle %d" % (row[7], nc))
            dev = np.abs(row[:6] - np.concatenate([Ro.reshape(4), to])).max()
            if not dev <= tol:                      # (NaN fails)
                raise CertificateError("pose", s, k, "|device - oracle| %.3g > %.3g" % (dev, tol))
            dd = abs(row[6] - d)
            if not dd <= tol:
                raise CertificateError("delta", s, k, "device %r oracle %r" % (row[6], d))
            worst = max(worst, dev, dd)
            # the iteration rule, from the device's own delta: the first k + 1 with delta_k < min_delta, else max_iter
            if row[6] < min_delta and k + 1 != iters:
                raise CertificateError("iters", s, k, "delta %r < min_delta %r but %d steps ran" % (row[6], min_delta, iters))
        last = trace[s, iters - 1]
        if iters < max_iter and not last[6] < min_delta:
            raise CertificateError("iters", s, iters - 1, "stopped after %d of %d steps at delta %r >= min_delta %r"
                                   % (iters, max_iter, last[6], min_delta))
        if not (result["delta"][s] == last[6] and result["n_corr"][s] == last[7]):
            raise CertificateError("result", s, iters - 1, "result (%r, %r) is not the last executed row (%r, %r)"
                                   % (result["delta"][s], result["n_corr"][s], last[6], last[7]))
        if R is not None and not (_same(np.reshape(R[s], 4), last[:4]) and _same(t[s], last[4:6])):
            raise CertificateError("result", s, iters - 1, "the pose left is not the last executed row")
        for k in range(iters, trace.shape[1]):
            if not _same(trace[s, k], np.full(8, fill)):
                raise CertificateError("unwritten", s, k, "a row beyond the %d executed steps was written" % iters)
    return worst


# ------------------------------------------------------------------------------------------------- the oracle's own trace
RESULT_DTYPE = np.dtype([("iters", np.int32), ("n_corr", np.int32), ("delta", np.float64)])


def oracle_trace(model, batch, max_iter, min_delta, indist, mode, fill=np.nan):
    """Icp::fit (icp.cpp:80-122) as a chain of the oracle's brute-force steps: trace[S, max_iter, 8] (rows not executed keep
    `fill`), result[S], the poses left, and per scan the list of correspondence arrays (model index per query, -1 = gated out)."""
    S = batch.n_scans
    trace = np.full((S, max_iter, 8), fill)
    result = np.zeros(S, RESULT_DTYPE)
    Rs, ts = np.array(batch.R, np.float64).reshape(S, 4).copy(), np.array(batch.t, np.float64).reshape(S, 2).copy()
    corrs = []
    prm = O.icp_params(1, -1.0, indist, O.NN_BRUTE, mode)
    for s in range(S):
        ga, nga = batch.scan(s)
        corrs.append([])
        if len(ga) + len(nga) < MIN_SCAN_POINTS:
            continue
        R, t = Rs[s].reshape(2, 2), ts[s]
        for k in range(max_iter):
            d, R, t, nc, corr = model.fit_step(ga, nga, R, t, prm)
            trace[s, k] = np.concatenate([R.reshape(4), t, [d, nc]])
            corrs[s].append(corr)
            result[s] = (k + 1, nc, d)
            if d < min_delta:
                break
        Rs[s], ts[s] = R.reshape(4), t
    return trace, result, Rs, ts, corrs


def continue_chain(model, batch, trace, result, s, k, max_iter, min_delta, indist, mode):
    """rows k + 1 ... of scan s redone by the oracle from row k as it stands: what a device does that went wrong in step k alone"""
    ga, nga = batch.scan(s)
    prm = O.icp_params(1, -1.0, indist, O.NN_BRUTE, mode)
    trace[s, k + 1:] = np.nan
    R, t, d, nc = trace[s, k, :4].reshape(2, 2), trace[s, k, 4:6], trace[s, k, 6], trace[s, k, 7]
    it = k + 1
    while it < max_iter and not d < min_delta:
        d, R, t, nc, _ = model.fit_step(ga, nga, R, t, prm)
        trace[s, it] = np.concatenate([R.reshape(4), t, [d, nc]])
        it += 1
    result[s] = (it, nc, d)


# ------------------------------------------------------------------------------------ the steps, restated for mutation
def queries(pts, R, t):
    """icpPointToPoint.cpp:69-70: the double expression r0 * x + r1 * y + t, summed left to right, stored as float"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    R = np.asarray(R, np.float64).reshape(2, 2)
    qx = R[0, 0] * pts[:, 0] + R[0, 1] * pts[:, 1] + t[0]
    qy = R[1, 0] * pts[:, 0] + R[1, 1] * pts[:, 1] + t[1]
    return np.stack([qx, qy], 1).astype(np.float32)


def two_nearest(xy_f32, q_f32):
    """per query: index and float distance (fl(fl(dx dx) + fl(dy dy)), kdtree.cpp:360-375) of the nearest model point -- the
    lowest index among equals -- and of the runner-up"""
    xy, q = np.asarray(xy_f32, np.float32), np.asarray(q_f32, np.float32)
    idx, dis = np.full((len(q), 2), -1, np.int64), np.full((len(q), 2), np.inf, np.float32)
    for lo in range(0, len(q), 256):
        rows = np.arange(len(q[lo:lo + 256]))
        dx, dy = xy[None, :, 0] - q[lo:lo + 256, None, 0], xy[None, :, 1] - q[lo:lo + 256, None, 1]
        d = dx * dx + dy * dy                                   # float32 throughout
        a = np.argmin(d, 1)                                     # the first of equals
        idx[lo:lo + 256, 0], dis[lo:lo + 256, 0] = a, d[rows, a]
        if xy.shape[0] > 1:
            d[rows, a] = np.inf
            b = np.argmin(d, 1)
            idx[lo:lo + 256, 1], dis[lo:lo + 256, 1] = b, d[rows, b]
    return idx, dis


class Correspondences:
    """What one step pairs up, in the oracle's order (class GA's queries, then class NGA's): q[n, 2] float queries, cls[n],
    idx[n] the model index within the searched set (-1: no search, the class is skipped), dis[n] the float distance, inlier[n];
    idx2 / dis2: the runner-up.  `xy` maps a class to the float model points its indices refer to."""

    def __init__(self, model, ga, nga, R, t, indist, mode):
        m_ga, m_nga = model.m_ga.astype(np.float32), model.m_nga.astype(np.float32)
        ga, nga = np.asarray(ga, np.float64).reshape(-1, 2), np.asarray(nga, np.float64).reshape(-1, 2)
        self.mode = mode
        self.q = queries(np.concatenate([ga, nga]), R, t)
        self.cls = np.concatenate([np.zeros(len(ga), int), np.ones(len(nga), int)])
        n = len(self.q)
        self.idx, self.idx2 = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        self.dis, self.dis2 = np.full(n, np.inf, np.float32), np.full(n, np.inf, np.float32)
        if mode == O.MODE_P2L:                     # one class, no gate (icpPointToPlane.cpp:55-77)
            self.xy = {0: np.concatenate([m_ga, m_nga])}
            self.xy[1] = self.xy[0]
            self.normals = model.normals()
            groups = [(np.arange(n), self.xy[0])]
        else:
            self.xy = {0: m_ga, 1: m_nga}
            groups = [(np.flatnonzero(self.cls == c), self.xy[c]) for c in (0, 1) if len(self.xy[c]) > 3]   # :59, :93
        for sel, xy in groups:
            i, d = two_nearest(xy, self.q[sel])
            self.idx[sel], self.idx2[sel], self.dis[sel], self.dis2[sel] = i[:, 0], i[:, 1], d[:, 0], d[:, 1]
        if mode == O.MODE_P2L:
            self.inlier = np.ones(n, bool)
        else:
            self.inlier = (self.idx >= 0) & (self.dis.astype(np.float64) < indist)      # :76 float promoted against double

    def model_points(self):
        out = np.zeros((len(self.q), 2), np.float32)
        for c in (0, 1):
            sel = (self.cls == c) & (self.idx >= 0)
            out[sel] = self.xy[c][self.idx[sel]]
        return out


def _compose(R_, t_, R, t):
    """icpPointToPoint.cpp:166-170: R = R_ R, t = R_ t + t_, delta = max(|R_ - I|_F, |t_|)"""
    R, t = np.asarray(R, np.float64).reshape(2, 2), np.asarray(t, np.float64)
    Rn = np.array([[R_[0, 0] * R[0, 0] + R_[0, 1] * R[1, 0], R_[0, 0] * R[0, 1] + R_[0, 1] * R[1, 1]],
                   [R_[1, 0] * R[0, 0] + R_[1, 1] * R[1, 0], R_[1, 0] * R[0, 1] + R_[1, 1] * R[1, 1]]])
    tn = np.array([(R_[0, 0] * t[0] + R_[0, 1] * t[1]) + t_[0], (R_[1, 0] * t[0] + R_[1, 1] * t[1]) + t_[1]])
    nr = np.sqrt((R_[0, 0] - 1.0) ** 2 + R_[0, 1] ** 2 + R_[1, 0] ** 2 + (R_[1, 1] - 1.0) ** 2)
    nt = np.sqrt(t_[0] ** 2 + t_[1] ** 2)
    return Rn, tn, max(nr, nt)


def p2p_step(c, R, t):
    """icpPointToPoint.cpp:33-172 from the correspondences c: sums and means in long double.  Returns the trace row."""
    sel = c.inlier
    n = int(sel.sum())
    if n == 0:
        return np.concatenate([np.reshape(R, 4), t, [-1.0, 0.0]])       # :128-131
    pt = c.q[sel].astype(np.longdouble)
    pm = c.model_points()[sel].astype(np.longdouble)
    mu_t, mu_m = pt.sum(0) / n, pm.sum(0) / n
    H = ((pt - mu_t)[:, :, None] * (pm - mu_m)[:, None, :]).sum(0)      # :155-159  H = ~q_t q_m
    R_ = O.p2p_rotation(H.astype(np.float64))
    mu_t, mu_m = mu_t.astype(np.float64), mu_m.astype(np.float64)
    t_ = np.array([mu_m[0] - (R_[0, 0] * mu_t[0] + R_[0, 1] * mu_t[1]), mu_m[1] - (R_[1, 0] * mu_t[0] + R_[1, 1] * mu_t[1])])
    Rn, tn, d = _compose(R_, t_, R, t)
    return np.concatenate([Rn.reshape(4), tn, [d, float(n)]])


def p2l_step(c, R, t):
    """icpPointToPlane.cpp:37-107 (2-D): the 3 x 3 normal equations in long double, the reference's Gauss-Jordan on them"""
    n = len(c.q)
    s = c.q.astype(np.longdouble)
    d = c.model_points().astype(np.longdouble)
    nm = c.normals[c.idx].astype(np.longdouble)
    A = np.stack([nm[:, 1] * s[:, 0] - nm[:, 0] * s[:, 1], nm[:, 0], nm[:, 1]], 1)
    b = nm[:, 0] * d[:, 0] + nm[:, 1] * d[:, 1] - nm[:, 0] * s[:, 0] - nm[:, 1] * s[:, 1]
    AtA, Atb = (A[:, :, None] * A[:, None, :]).sum(0), (A * b[:, None]).sum(0)
    ok, x = O.solve3(AtA.astype(np.float64), Atb.astype(np.float64))
    if not ok:
        return np.concatenate([np.reshape(R, 4), t, [0.0, float(n)]])   # :85
    Rn, tn, dl = _compose(O.orthonormal_from_omega(x[0]), x[1:], R, t)
    return np.concatenate([Rn.reshape(4), tn, [dl, float(n)]])


def restated_step(c, R, t):
    return p2l_step(c, R, t) if c.mode == O.MODE_P2L else p2p_step(c, R, t)
