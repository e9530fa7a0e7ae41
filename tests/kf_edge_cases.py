"""Hand-worked keyframe edges, one per branch of the edge kernel's solver and stop rules, and the clouds that take the
gated search to where the lattice ends.  Not a test file: tests/test_kf_edge_cases.py walks the restatement
(tests/cpp/kf_edge_oracle.cpp) through them on the CPU, tests/test_gpu_kf_edge_branches.py the device, on the same inputs.

Rules for the inputs of the exact cases, which are what makes tight bounds legitimate:
  * coordinates are small multiples of 2^-8, transforms are 90-degree turns and dyadic shifts, pair counts are powers of
    two wherever a mean is taken.  Every f64 sum of the ICP (centroids, H) is then exact in any order, so the device's H is
    the restatement's bit for bit, and a vanishing singular value is an exact zero (axis-aligned planes and lines keep
    exact zero rows and columns through the Jacobi rotations): the rank decision cannot flip on reassociation;
  * points are far enough apart for the store's voxel filter to keep every one (each alone in its voxel; the two clouds
    with points closer than that carry a leaf_size of their own);
  * every intended pair is nearer than half the distance to any other point, so the pairing is the hand-worked one.

A case is a dict: name, src and tgt (raw [n, 3] f32 clouds; src = keyframe `to`, tgt = keyframe `from`), init (4 x 4),
store (parameters fixed at the store's creation: leaf_size), icp (parameters of the edge: max_iterations and the two
epsilons) and the expectations: n_src / n_tgt (filtered point counts), rank and sign (solver_sign below) of the first
iteration's H (None where no step is taken), state, iterations, pairs, first (pairs of the first iteration), num_corr, singular,
lum (why LUM falls back: "ss" for ss ~ 0, "nonfinite" for a non-finite D from a singular MM, "nopairs"; None when it does
not; singular = None leaves it to the restatement), mse (where it is an exact number), T (the hand-worked total transform,
or None), match (the hand-worked pairs as two coordinate arrays, or None), exact (False where the inputs are not dyadic)
and image (True where the pairs determine the image of the source but not the whole rotation: a line).  None in a count
means that the case does not pin it."""
import numpy as np

from slam_amd import api

SOLVE_TOL = 1e-12   # closed-form solves on exact pairs, as tests/test_gpu_icp.py
OFFSET = np.array([0.25, -0.125, 0.25])


def rot90(axis, quarter_turns):
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    R = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def lattice_cloud(seed=5, n=4, pitch=2.0):
    """n^3 points about `pitch` apart on dyadic coordinates (multiples of 2^-8): rotations by 90 degrees and dyadic
    translations of it are exact in f32, and every point is its copy's nearest neighbour for offsets below pitch / 2"""
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(n) * pitch] * 3, indexing="ij"), -1).reshape(-1, 3)
    return (g + rs.randint(-64, 65, g.shape) / 256.0 - pitch * (n - 1) / 2).astype(np.float32)


def T_of(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


AXES = np.array([[4, 0, 0], [-4, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def flat_cloud(thin_axis, thin=32, seed=7, n=8, pitch=2.0):
    """n x n points (64: a power of two) of pitch 2 with +-0.25 of dyadic jitter in two axes; the third coordinate a multiple
    of 2^-8 up to thin / 256 (0: a plane)"""
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(*[np.arange(n) * pitch] * 2, indexing="ij"), -1).reshape(-1, 2)
    g = g + rs.randint(-64, 65, g.shape) / 256.0 - pitch * (n - 1) / 2
    w = rs.randint(-thin, thin + 1, len(g)) / 256.0 if thin else np.zeros(len(g))
    out = np.insert(g, thin_axis, w, axis=1)
    return out.astype(np.float32)


def exact_copy(src, R, t):
    tgt = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    assert np.array_equal(tgt.astype(np.float64), src.astype(np.float64) @ R.T + t)
    return tgt


def case(name, src, tgt, init=None, store=None, icp=None, **expect):
    c = dict(name=name, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(tgt, np.float32),
             init=np.eye(4, dtype=np.float32) if init is None else np.asarray(init, np.float32), store=store or {}, icp=icp or {},
             rank=None, sign=None, T=None, lum=None, mse=None, exact=True, image=False)
    c.update(n_src=len(src), n_tgt=len(tgt))
    c.update(expect)
    c.setdefault("first", c["pairs"])
    c.setdefault("num_corr", c["pairs"])
    c.setdefault("singular", 0 if c["lum"] is None else 1)
    if "match" not in c:   # the hand-worked pairs: source point i belongs to target point i, for the first `first` of them
        n = c["first"]
        c["match"] = (c["src"][:n], c["tgt"][:n]) if n else None
    return c


def cloud3d_case():
    """keyframes 0 and 1 of synth.make_cloud3d: a noisy edge whose mse moves by a few per cent per iteration, against a
    fitness epsilon of 0.5.  The counts are those of the voxel filter at 0.5 m (tests/test_kf_edge_oracle.py)."""
    import kf_edge_oracle as K
    (x0, p0), (x1, p1) = K.cloud(0), K.cloud(1)
    return case("stop-rel-mse", x1, x0, K.relative_init(p0, p1), icp=dict(transformation_epsilon=-1.0, fitness_epsilon=0.5),
                rank=3, sign=1, state=api.KF_REL_MSE, iterations=2, pairs=None, first=None, num_corr=None, exact=False,
                n_src=None, n_tgt=None, match=None)


def cases():
    out = []
    # --- reflected pairs: det H < 0, the sign fix.  No closed form (the best proper rotation of a mirrored slab)
    for name, axis in (("mirror-z", 2), ("mirror-x", 0)):
        src = flat_cloud(axis)
        m = np.ones(3)
        m[axis] = -1
        out.append(case(name, src, exact_copy(src, np.diag(m), np.zeros(3)), rank=3, sign=-1, state=api.KF_TRANSFORM,
                        iterations=2, pairs=64))
    # --- planar pairs: rank 2; a rigid copy is recovered by the first step, the second is the identity
    for name, axis, turn in (("planar-z", 2, (2, 1)), ("planar-y", 0, (1, 1))):
        src = flat_cloud(axis, thin=0)
        R, t = rot90(*turn), np.array([0.5, -1.25, 2.0])
        out.append(case(name, src, exact_copy(src, R, t), T_of(R, t + OFFSET), rank=2, sign=1, state=api.KF_TRANSFORM,
                        iterations=2, pairs=64, lum="ss", T=T_of(R, t)))
    # --- a planar set mirrored in its own plane: 16 points 2 m apart along x, y a pattern that is even about the middle, so
    # that H = diag(Sxx, -Syy, 0) exactly; U = diag(1, -1, -1) after the completion, V = I: det U det V decides, and the
    # proper rotation that does it turns the plane over (180 degrees about x)
    y = np.array([3, -7, 12, 30, -18, 5, 26, -11], np.float64) / 256.0
    src = np.column_stack([np.arange(16) * 2.0 - 15, np.concatenate([y, y[::-1]]), np.zeros(16)])
    out.append(case("planar-mirror", src, src * [1, -1, 1], rank=2, sign=-1, state=api.KF_TRANSFORM, iterations=2, pairs=16,
                    lum="ss", T=T_of(np.diag([1.0, -1, -1]), np.zeros(3))))
    # --- collinear pairs: rank 1.  The line lands on its copy; the roll about it is whatever the completion gives (here a
    # quarter turn each step, so the transform test never passes and the mse, 0 twice, ends it).  16 pairs, a really
    # singular MM
    src = np.column_stack([np.arange(16) * 2.0 - 15, np.zeros(16), np.zeros(16)])
    out.append(case("line", src, src + [0.25, 0.125, -0.25], rank=1, sign=1, state=api.KF_ABS_MSE, iterations=3, pairs=16,
                    lum="nonfinite", image=True, T=T_of(np.eye(3), [0.25, 0.125, -0.25])))
    # --- coincident pairs: one target point, eight source points around it (a quarter of a metre apart: leaf 1/8): rank 0,
    # R = I, t = q - mean(p)
    q = np.array([[1.0, 2.0, -0.5]])
    off = np.stack(np.meshgrid(*[[-0.125, 0.25]] * 3, indexing="ij"), -1).reshape(-1, 3)
    out.append(case("coincident", q + off, q, store=dict(leaf_size=0.125), rank=0, sign=1, state=api.KF_TRANSFORM, iterations=2,
                    pairs=8, T=T_of(np.eye(3), [-0.0625] * 3), match=(q + off, np.repeat(q, 8, axis=0)), singular=None))
    # --- fewer than three pairs: no step, init returned
    tgt = np.array([[0, 0, 0], [5, 0, 0], [50, 50, 50]])
    out.append(case("two-pairs", [[0.125, 0, 0], [5.125, 0, 0], [20, 20, 20]], tgt, state=api.KF_NO_CORRESPONDENCES, iterations=0,
                    pairs=2, lum="nonfinite", T=np.eye(4)))
    out.append(case("one-pair", [[0.125, 0, 0], [30, 0, 0], [20, 20, 20]], tgt, state=api.KF_NO_CORRESPONDENCES, iterations=0,
                    pairs=1, lum="nonfinite", T=np.eye(4)))
    # --- exactly three pairs, the smallest set that takes a step: three points span a plane (the sums are exact; their
    # division by 3 rounds, the same way on both sides)
    tgt = np.array([[0, 0, 0], [6, 0, 0], [0, 3, 0], [50, 50, 50]])
    src = np.array([[0, 0, 0], [6, 0, 0], [0, 3, 0], [20, 20, 20]]) - OFFSET
    out.append(case("three-pairs", src, tgt, rank=2, sign=1, state=api.KF_TRANSFORM, iterations=2, pairs=3, lum="ss",
                    T=T_of(np.eye(3), OFFSET)))
    # --- at the gate.  0.75 and 0.5625 are exact in f32 and f64: ICP keeps d^2 = gate^2 (<=), LUM drops it (<).  LUM runs on
    # the final transform, so the edge that shows LUM's side takes no step: two of the four points at the gate, the others
    # out of reach.  One ulp inside the gate LUM takes the pair at the origin; 10 + 0.74999994 rounds to 10.75 in f32, at the
    # gate again
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10]], np.float32)
    out.append(case("gate-step", tgt + np.float32([0.75, 0, 0]), tgt, icp=dict(max_iterations=1), rank=3, sign=1,
                    state=api.KF_ITERATIONS, iterations=1, pairs=4, lum="ss", mse=0.5625, T=T_of(np.eye(3), [-0.75, 0, 0])))
    far = np.float32([[0, 30, 0], [0, 0, 30]])
    out.append(case("gate-hold", np.concatenate([tgt[:2] + np.float32([0.75, 0, 0]), far]), tgt, state=api.KF_NO_CORRESPONDENCES,
                    iterations=0, pairs=2, num_corr=0, lum="nopairs", mse=0.5625, T=np.eye(4)))
    inside = tgt[:2] + np.float32([np.nextafter(np.float32(0.75), np.float32(0)), 0, 0])
    assert inside[1, 0] == np.float32(10.75)
    out.append(case("gate-inside", np.concatenate([inside, far]), tgt, state=api.KF_NO_CORRESPONDENCES, iterations=0, pairs=2,
                    num_corr=1, lum="nonfinite", T=np.eye(4)))
    # --- the stop states, on a full-rank exact copy a quarter of a metre off
    src = lattice_cloud()
    tgt = src + np.float32([0.25, 0, 0])
    T = T_of(np.eye(3), [0.25, 0, 0])
    out.append(case("stop-cap", src, tgt, icp=dict(max_iterations=1), rank=3, sign=1, state=api.KF_ITERATIONS, iterations=1,
                    pairs=64, lum="ss", mse=0.0625, T=T))
    out.append(case("stop-transform", src, tgt, rank=3, sign=1, state=api.KF_TRANSFORM, iterations=2, pairs=64, lum="ss", T=T))
    out.append(case("stop-abs-mse", src, tgt, icp=dict(transformation_epsilon=-1.0), rank=3, sign=1, state=api.KF_ABS_MSE,
                    iterations=3, pairs=64, lum="ss", T=T))
    out.append(cloud3d_case())
    out.append(case("stop-disjoint", src + np.float32(100), tgt, state=api.KF_NO_CORRESPONDENCES, iterations=0, pairs=0,
                    lum="nopairs", T=np.eye(4)))
    # --- a NaN in init: every distance is NaN and dropped; the NaN init is returned
    init = np.eye(4, dtype=np.float32)
    init[1, 3] = np.nan
    out.append(case("nan-init", src, tgt, init, state=api.KF_NO_CORRESPONDENCES, iterations=0, pairs=0, lum="nopairs", T=init))
    # --- a plane in a generic orientation, coordinates rounded to f32: the third singular value is rounding noise, and which
    # side of 3 eps it falls on is not pinned.  Properties only, on device and restatement alike.
    p = flat_cloud(2, thin=0, seed=9).astype(np.float64)
    A, B = rodrigues([1, 2, 3], 0.7), rodrigues([2, -1, 0.5], 0.02)
    src = (p @ A.T).astype(np.float32)
    tgt = (src.astype(np.float64) @ B.T + [0.125, -0.0625, 0.1]).astype(np.float32)
    out.append(case("generic-plane", src, tgt, state=api.KF_TRANSFORM, iterations=None, pairs=64, exact=False,
                    T=T_of(B, [0.125, -0.0625, 0.1])))
    return out


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def icp_settings(c):
    """the edge parameters of a case, over setup_gicp's defaults"""
    s = dict(max_iterations=200, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
    s.update(c["icp"])
    return s


def residual(T, match):
    """the mean squared distance of the hand-worked pairs under the 4 x 4 transform T, in f64"""
    p, q = (np.asarray(a, np.float64) for a in match)
    d = p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3] - q
    return float((d * d).sum(axis=1).mean())


def solver_sign(H, rank):
    """Which way round the pairs are, in f64 from H alone: the sign of det H for a full-rank H; for a rank-2 H that of its
    second invariant (the product of the two non-zero eigenvalues: negative when the pairs are mirrored within their
    plane); for rank 1 that of the trace; +1 for H = 0."""
    H = np.asarray(H, np.float64)
    if rank == 3:
        return int(np.sign(np.linalg.det(H)))
    if rank == 2:
        return int(np.sign(sum(np.linalg.det(H[np.ix_(k, k)]) for k in ([0, 1], [0, 2], [1, 2]))))
    return int(np.sign(np.trace(H))) if rank == 1 else 1


def cross_covariance(p, q):
    """H = sum (q - qm)(p - pm)' / n in numpy f64"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    return (q - q.mean(axis=0)).T @ (p - p.mean(axis=0)) / len(p)


# ------------------------------------------------------------------ keyframes with an exact filtered point count
def counted_lattice(n, seed=3):
    """n points of pitch 1 with +-1/16 of dyadic jitter, filled plane by plane of a 16 x 16 base: each alone in its 0.5 m
    voxel (floor(2 (k + j)) is 2 k - 1 or 2 k), and a copy moved by less than 0.4375 m pairs point for point"""
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    g = np.column_stack([i % 16, (i // 16) % 16, i // 256]).astype(np.float64)
    return (g + rs.randint(-16, 17, g.shape) / 256.0 - [8, 8, 0]).astype(np.float32)


# ------------------------------------------------------------------ the search where the lattice ends
def lattice_bound(params):
    """B: the coordinate at which a cell coordinate clamps, lattice edge * 2^20"""
    return (params.cell_size if params.cell_size > 0 else params.gate) * api.KF_LATTICE_MARGIN * 2.0 ** 20


def box_cloud(centre, n=3000, side=12.0, seed=0):
    """about n distinct f32 points in a box (f32 spacing at 786 444 m is 1/16 m: rounded, then deduplicated)"""
    rs = np.random.RandomState(seed)
    p = (np.asarray(centre, np.float64) + rs.uniform(-side / 2, side / 2, (n, 3))).astype(np.float32)
    return np.unique(p, axis=0)


def box_queries(points, centre, n=6000, side=12.0, seed=1, sigma=0.5):
    """half near points of the cloud (inside and around the gate), half anywhere in the box grown by 2 m, some exact hits"""
    rs = np.random.RandomState(seed)
    near = points[rs.randint(0, len(points), n // 2), :3].astype(np.float64) + rs.normal(0, sigma, (n // 2, 3))
    anywhere = np.asarray(centre, np.float64) + rs.uniform(-side / 2 - 2, side / 2 + 2, (n - n // 2, 3))
    q = np.concatenate([near, anywhere]).astype(np.float32)
    q[:16] = points[:16, :3]
    return q


def placements(params):
    """name -> centre of the 12 m box.  The boxes at the clamp lie two thirds beyond it, so that the cell all clamped
    coordinates share holds (2/3)^3 of the corner cloud."""
    B = lattice_bound(params)
    return {"origin": (0.0, 0.0, 0.0), "+B in x": (B + 2, 40.0, -7.0), "-B in y": (13.0, -B - 2, 5.0),
            "corner": (B + 2, -B - 2, B + 2), "beyond": (3 * B, 3 * B, -3 * B)}


def one_cell_cloud(n=2000, seed=4):
    """n distinct points on a 2^-8 grid inside [1/8, 5/8) x [1/8, 5/8) x [1/8, 3/16): one lattice cell; leaf 2^-9 keeps
    them all (x * 512 is an even integer)"""
    rs = np.random.RandomState(seed)
    flat = rs.choice(128 * 128 * 16, n, replace=False)
    g = np.column_stack([flat % 128, (flat // 128) % 128, flat // (128 * 128)])
    return (g / 256.0 + 0.125).astype(np.float32)


ONE_CELL_LEAF = 2.0 ** -9


def corner_lattice(params, n=2048, seed=6):
    """a 16 x 16 x 8 lattice of pitch 1 (multiples of 1/16 there) about the corner (+B, -B, +B): every octant of the clamp
    holds an eighth of it; 2 048 points, so the centroids of a full pairing are exact"""
    B = np.floor(lattice_bound(params) * 16) / 16
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    g = np.column_stack([i % 16, (i // 16) % 16, i // 256]).astype(np.float64) - [7.5, 7.5, 3.5]
    p = g + rs.randint(-1, 2, g.shape) / 16.0 + [B, -B, B]
    out = p.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), p)
    return out
