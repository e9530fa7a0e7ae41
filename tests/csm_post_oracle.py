"""The posterior of a correlative match restated in numpy and Python integers (docs/CSM.md section 6): every candidate of
the exhaustive score volume within the margin, weighted by a table it is given, summed into integer moments about the
winner, and finished in IEEE doubles in the contract's order of operations.  It reads the volume of the scalar restatement
(csm_oracle.OracleMatcher.volume(..., counted=True)) and shares no code with the library."""
import math
import struct

import numpy as np

INT_FIELDS = ("valid", "n_within", "margin", "blocks_evaluated", "second_score", "second_k", "second_a", "second_b")
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx xy xt yy yt tt
DEFAULTS = dict(margin_per_point=16, beta=8.0, excl_xy=2, excl_theta=2)


def weight_table(beta):
    """the contract's formula with the host's libm, entry by entry"""
    return np.array([int(np.rint(65536.0 * math.exp(-(beta * float(j)) / 256.0))) for j in range(257)], np.uint32)


def guard_ok(n_x, n_y, n_theta):
    """65536 Dmax^2 N < 2^63 in Python integers"""
    dmax = max(n_x, n_y, n_theta) - 1
    return 65536 * dmax * dmax * (n_x * n_y * n_theta) < 2 ** 63


def invalid():
    out = {f: 0 for f in INT_FIELDS}
    out.update(second_score=-1, m0=0, m1=[0, 0, 0], m2=[0] * 6, mean=[0.0] * 3, cov=[0.0] * 6, mean_c=[0.0] * 3, cov_c=[0.0] * 6)
    return out


def within(vol, cnt, margin_per_point):
    """(winner (k, b, a), S*, M, deficits int64 [N_theta, N_y, N_x], mask d <= M)"""
    k, b, a = (int(v) for v in np.unravel_index(int(np.argmax(vol)), vol.shape))       # the first maximum: lowest flat index
    top = int(vol[k, b, a])
    M = int(margin_per_point) * int(cnt[k])
    d = top - vol.astype(np.int64)
    return (k, b, a), top, M, d, d <= M


def posterior(vol, cnt, n_scan_points, wtab, resolution, theta_step, margin_per_point=16, excl_xy=2, excl_theta=2, bounds=None,
              exhaustive=False, **_):
    """dict of slam_csm_posterior's fields (plus mean_c, cov_c in cells and steps).  bounds: U [N_theta, blocks_y, blocks_x]
    for blocks_evaluated (0 without it)."""
    if n_scan_points < 5:
        return invalid()
    assert guard_ok(vol.shape[2], vol.shape[1], vol.shape[0])
    (k, b, a), top, M, d, mask = within(vol, cnt, margin_per_point)
    kk, bb, aa = np.nonzero(mask)
    dd = d[mask]
    j = (dd * 256) // M if M > 0 else np.zeros_like(dd)
    assert j.min() >= 0 and j.max() <= 256
    w = [int(v) for v in np.asarray(wtab, np.uint32)[j]]
    o = [[int(v) - a for v in aa], [int(v) - b for v in bb], [int(v) - k for v in kk]]
    n = len(w)
    m0 = sum(w)
    m1 = [sum(w[c] * o[i][c] for c in range(n)) for i in range(3)]
    m2 = [sum(w[c] * o[i][c] * o[j_][c] for c in range(n)) for i, j_ in PAIRS]
    assert m0 >= 65536 and all(abs(v) < 2 ** 63 for v in [m0] + m1 + m2)
    out = dict(valid=1, n_within=n, margin=M, blocks_evaluated=0, m0=m0, m1=m1, m2=m2)
    if bounds is not None:
        out["blocks_evaluated"] = int(bounds.size) if exhaustive else int(np.count_nonzero(bounds.astype(np.int64) >= top - M))
    # the second mode: the best of the same candidates outside the exclusion box, the lowest flat index among equals
    K, B, A = np.indices(vol.shape)
    far = mask & ((np.abs(A - a) > excl_xy) | (np.abs(B - b) > excl_xy) | (np.abs(K - k) > excl_theta))
    out.update(second_score=-1, second_k=0, second_a=0, second_b=0)
    if far.any():
        sk, sb, sa = (int(v) for v in np.unravel_index(int(np.argmax(np.where(far, vol, -1))), vol.shape))
        out.update(second_score=int(vol[sk, sb, sa]), second_k=sk, second_a=sa, second_b=sb)
    # the finish: Python floats are IEEE doubles, every operation rounds on its own
    f0 = float(m0)
    u = (float(resolution), float(resolution), float(theta_step))
    mean_c = [float(m1[i]) / f0 for i in range(3)]
    cov_c = [float(m2[p]) / f0 - mean_c[i] * mean_c[j_] for p, (i, j_) in enumerate(PAIRS)]
    out["mean_c"], out["cov_c"] = mean_c, cov_c
    out["mean"] = [mean_c[i] * u[i] for i in range(3)]
    out["cov"] = [(cov_c[p] * u[i]) * u[j_] for p, (i, j_) in enumerate(PAIRS)]
    return out


def pack(post):
    """the bytes of a slam_csm_posterior holding these fields: 8 int32, 10 int64, 9 doubles"""
    return struct.pack("<8i10q9d", *[post[f] for f in INT_FIELDS], post["m0"], *post["m1"], *post["m2"], *post["mean"], *post["cov"])
