"""Shared inputs of the Generalized ICP tests (tests/test_kf_gicp_oracle.py on the CPU, tests/test_gpu_kf_gicp.py and
tests/test_gpu_global_match.py on the device): the hand-worked requests, the clouds for the neighbour and covariance
checks, the scene GICP exists for, and global_match's scene.

The hand-worked requests have coordinates that are multiples of 2^-3, quarter turns, dyadic shifts, gicp_epsilon = 2^-10 and
surfaces whose normals are axes away from the corner's edges, so that C' is diagonal with entries 1 and 2^-10 there and the
copies are recovered in closed form.  Points next to an edge see both surfaces and get a tilted normal, and an end of the line
pairs I with diag(1, 1, 2^-10), so M is not dyadic everywhere and the sums are held to 1e-12, not to the bit; where a case says
`exact` (no pairs at all) every sum is an exact zero."""
import numpy as np

import kf_edge_oracle as K

EPS = 2.0 ** -10


def grid(us, vs):
    return np.array([(u, v) for u in us for v in vs], np.float64)


def corner(pitch, n, du=0.0, dv=0.0):
    """A floor (z = 0) and two walls (x = 0, y = 0), n x n samples each at `pitch`, from one pitch off the edges; the samples
    are shifted by (du, dv) within each surface."""
    a = pitch * np.arange(1, n + 1)
    g = grid(a + du, a + dv)
    z = np.zeros(len(g))
    floor = np.stack([g[:, 0], g[:, 1], z], 1)
    wall_x = np.stack([z, g[:, 0], g[:, 1]], 1)
    wall_y = np.stack([g[:, 1], z, g[:, 0]], 1)
    return np.concatenate([floor, wall_x, wall_y]).astype(np.float32)


def rigid(yaw_quarters=0, shift=(0, 0, 0), yaw=None):
    th = 0.5 * np.pi * yaw_quarters if yaw is None else yaw
    c, s = (np.round(np.cos(th)), np.round(np.sin(th))) if yaw is None else (np.cos(th), np.sin(th))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = shift
    return T


def apply(T, xyz):
    return (np.asarray(xyz, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


TRUTH = rigid(1, (0.5, -0.25, 0.125))            # source -> target: a quarter turn about z and a dyadic shift
CORNER = corner(0.25, 8)                         # 192 points, every one its own voxel at leaf 1/8
CORNER_SRC = apply(np.linalg.inv(TRUTH), CORNER)  # exact: the inverse is a quarter turn and a dyadic shift too
LINE = np.stack([0.25 * np.arange(16), np.zeros(16), np.zeros(16)], 1).astype(np.float32)
# eight points two metres apart: every moved source point has its twin exactly at the gate and nothing else within it
SPREAD = np.array([(2.0 * i, 2.0 * j, 2.0 * k) for i in range(2) for j in range(2) for k in range(2)], np.float32)

STORE = dict(leaf_size=0.125, gate=0.75)
TIGHT = dict(k_correspondences=8, cov_radius=0.5, gicp_epsilon=EPS, max_iterations=30, transformation_epsilon=1e-9, rotation_epsilon=1e-9)

# name: target, source, init (f64 4x4, rounded to f32 by the caller), store params, gicp params, what is expected:
#   state, iterations (None: not pinned), pairs of the last iteration, truth (None: not compared; to 1e-12 unless truth_tol), exact
CASES = {
    # the truth plus a dyadic shift: the linear model is exact, one step lands on the truth, the second moves nothing
    "copy-shift": dict(target=CORNER, source=CORNER_SRC, init=rigid(0, (1 / 16, 0, 1 / 32)) @ TRUTH, store=STORE, gicp=TIGHT,
                       state=2, iterations=2, pairs=192, truth=TRUTH),
    # the truth plus a turn of 0.04 rad about an axis through the corner: Gauss-Newton on zero residuals, a few steps.  The
    # start's rotation is rounded to f32 and no longer orthogonal by 2^-24 per entry; every step is a rotation applied on the
    # left, so that stays, and the truth is met to the f32 rounding of the start (times the 2.25 m of the cloud), not to 1e-12
    "copy-turn": dict(target=CORNER, source=CORNER_SRC, init=rigid(yaw=0.04) @ TRUTH, store=STORE, gicp=TIGHT,
                      state=2, iterations=None, pairs=192, truth=TRUTH, truth_tol=8 * 2.25 * 2.0 ** -24),
    # the same start as copy-shift, one iteration allowed
    "cap": dict(target=CORNER, source=CORNER_SRC, init=rigid(0, (1 / 16, 0, 1 / 32)) @ TRUTH, store=STORE,
                gicp=dict(TIGHT, max_iterations=1), state=1, iterations=1, pairs=192, truth=TRUTH),
    # started on the truth: r = 0 in every pair, g = 0, the step is the identity
    "copy-still": dict(target=CORNER, source=CORNER_SRC, init=TRUTH, store=STORE, gicp=TIGHT, state=2, iterations=1, pairs=192,
                       truth=TRUTH),
    # collinear pairs along x: no pair constrains the roll, H(0, 0) is an exact zero, the first pivot fails
    "line": dict(target=LINE, source=apply(rigid(0, (1 / 16, 0, 0)), LINE), init=np.eye(4), store=STORE, gicp=TIGHT,
                 state=6, iterations=0, pairs=16, truth=None),
    # every twin exactly at the gate: the strict test drops all of them (the ICP edge keeps them)
    "gate": dict(target=SPREAD, source=apply(rigid(0, (-0.75, 0, 0)), SPREAD), init=np.eye(4), store=STORE,
                 gicp=dict(TIGHT, k_correspondences=4), state=5, iterations=0, pairs=0, truth=None, exact=True),
    # one step inside: kept
    "gate-inside": dict(target=SPREAD, source=apply(rigid(0, (-0.625, 0, 0)), SPREAD), init=np.eye(4), store=STORE,
                        gicp=dict(TIGHT, k_correspondences=4, max_iterations=1), state=1, iterations=1, pairs=8, truth=None),
    # clouds that never meet
    "disjoint": dict(target=CORNER, source=apply(rigid(0, (64, 0, 0)), CORNER), init=np.eye(4), store=STORE, gicp=TIGHT,
                     state=5, iterations=0, pairs=0, truth=None, exact=True),
    # a NaN start is returned as it came
    "nan-init": dict(target=CORNER, source=CORNER_SRC, init=np.full((4, 4), np.nan), store=STORE, gicp=TIGHT,
                     state=5, iterations=0, pairs=0, truth=None, exact=True),
}


# ------------------------------------------------------------------ the case GICP exists for
def interleaved_scene(pitch=0.5, n=10):
    """Two clouds sample the same floor and two walls at interleaved positions: the source's samples lie half a pitch
    along each surface from the target's.  Returns (target, source in its own frame, truth source -> target)."""
    truth = rigid(yaw=0.3, shift=(1.0, -0.5, 0.25))
    tgt = corner(pitch, n)
    src_in_target_frame = corner(pitch, n, du=0.5 * pitch)
    return tgt, apply(np.linalg.inv(truth), src_in_target_frame), truth


INTERLEAVED_START = rigid(yaw=0.03, shift=(0.08, -0.06, 0.05))   # on top of the truth


# ------------------------------------------------------------------ clouds for the neighbour and covariance checks
def lattice_cloud(n, seed, span=8):
    """n distinct points with coordinates that are multiples of 2^-3 in a cube of `span` steps: equal distances abound."""
    rs = np.random.RandomState(seed)
    cells = rs.permutation(span ** 3)[:n]
    return (np.stack([cells % span, (cells // span) % span, cells // span ** 2], 1) * 0.125).astype(np.float32)


def random_cloud(n, seed, box):
    return np.random.RandomState(seed).uniform(-box, box, (n, 3)).astype(np.float32)


def jittered_cloud(n, seed, span, leaf=0.25):
    """n points at generic positions, each alone in its voxel of a span^3 block of voxels of edge `leaf` (the voxel filter
    keeps all n; its accumulator holds at most 2^26 voxels, so span is at most 400)."""
    rs = np.random.RandomState(seed)
    cells = rs.permutation(span ** 3)[:n]
    ijk = np.stack([cells % span, (cells // span) % span, cells // span ** 2], 1)
    return ((ijk + rs.uniform(0.1, 0.9, (n, 3))) * leaf).astype(np.float32)


# ------------------------------------------------------------------ global_match's scene
MAP_KS = (0, 1, 2, 4)     # the prior map: these make_cloud3d keyframes moved to the map frame (that of keyframe 0)
SCAN_K = 8                # the scan
POSE_OFFSET = (6.0, 0.0, 1.5)   # the current pose is this far from the truth (metres, metres, radians): start 0 fails


def global_match_scene():
    """(map [n, 3] f32 in keyframe 0's frame, scan [m, 3] f32 in its own, true pose (x, y, yaw) of the scan in the map)."""
    pose0 = K.cloud(MAP_KS[0])[1]
    parts = []
    for k in MAP_KS:
        xyz, pose = K.cloud(k)
        parts.append(apply(K.true_relative(pose0, pose), xyz[:, :3]))
    scan, pose = K.cloud(SCAN_K)
    M = K.true_relative(pose0, pose)
    return np.concatenate(parts), np.ascontiguousarray(scan[:, :3], np.float32), (M[0, 3], M[1, 3], float(np.arctan2(M[1, 0], M[0, 0])))
