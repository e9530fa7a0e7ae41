"""Inputs shared by tests/test_csm_oracle.py (the restatement alone) and tests/test_gpu_csm.py (the device against it):
small models and scans that reach every edge of the correlative matcher's contract (docs/CSM.md).  numpy only."""
import numpy as np

RES = 0.1


def centre(cx, cy, res=RES):
    """the centre of lattice cell (cx, cy): (c + 0.5) res / res floors to c whatever the rounding"""
    return np.stack([(np.asarray(cx, np.float64) + 0.5) * res, (np.asarray(cy, np.float64) + 0.5) * res], axis=-1)


def model_points(n, seed):
    """n points on both sides of 0 within about +-3 m; every fourth sits exactly on a lattice edge (a multiple of 0.5 m, which
    divides by 0.1 to a whole number, or k * 0.1, which may land an ulp below it: floor decides), one on (0, 0)"""
    rs = np.random.RandomState(seed)
    p = rs.uniform(-3.0, 3.0, size=(n, 2))
    if n:
        p[::4] = np.round(p[::4] * 2.0) / 2.0
        p[1::8] = np.round(p[1::8] * 10.0) * 0.1
        p[0] = 0.0
    if n > 2:
        p[2] = (-0.5, -1e-12)        # just below an edge on the negative side: cell -1, not 0
    return np.ascontiguousarray(p)


def box_model(n_ga=40, n_nga=300, seed=7):
    """an L-shaped wall (NGA) and a small pillar (GA): asymmetric, so a pose is identifiable"""
    rs = np.random.RandomState(seed)
    u = rs.uniform(0.0, 1.0, n_nga)
    wall = np.where((u < 0.6)[:, None], np.stack([-3.0 + 10.0 * u, np.full(n_nga, 2.5)], 1),
                    np.stack([np.full(n_nga, 3.0), 2.5 - 10.0 * (u - 0.6)], 1))
    v = rs.uniform(0.0, 1.0, n_ga)
    pillar = np.stack([-1.0 + 0.8 * v, -0.7 + 0.3 * np.sin(6.0 * v)], 1)
    return (np.ascontiguousarray(pillar + rs.normal(0, 0.01, pillar.shape)),
            np.ascontiguousarray(wall + rs.normal(0, 0.01, wall.shape)))


def scan_of(model, n, pose, seed, ga_share=None):
    """n points of the model seen from `pose` (x, y, theta) in the sensor frame: (t_ga, t_nga)"""
    m_ga, m_nga = model
    rs = np.random.RandomState(seed)
    n_ga = min(len(m_ga), n // 5) if ga_share is None else int(n * ga_share)
    n_ga = n_ga if len(m_ga) else 0
    out = []
    for m, k in ((m_ga, n_ga), (m_nga, n - n_ga)):
        if k == 0:
            out.append(np.zeros((0, 2)))
            continue
        w = m[rs.randint(0, len(m), k)] + rs.normal(0, 0.01, (k, 2))
        c, s = np.cos(pose[2]), np.sin(pose[2])
        d = w - np.array(pose[:2])
        out.append(np.ascontiguousarray(np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1)))
    return out[0], out[1]


def pose_Rt(x, y, th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, -s], [s, c]]), np.array([x, y], np.float64)


SCAN_SIZES = (5, 63, 64, 65, 1081)                 # wave and workgroup boundaries, and more than one staged piece (1024)
WINDOWS = ((8, 8), (2, 16), (0, 8))                # N = 17 x 17 (two full blocks and a ragged one), 5 x 33, N_x = 1
HALF_THETAS = (0, 4)                               # N_theta = 1 and 9
TRUE_POSE = (0.4, -0.3, 0.3)


def volume_cases():
    """(name, t_ga, t_nga, R0, t0, (half_x, half_y), half_theta) against box_model().  The start's x moves by one cell from scan
    to scan, so the first column a lookup reads, cell.x - half_x, takes all four residues mod 4."""
    model = box_model()
    out = []
    for i, n in enumerate(SCAN_SIZES):
        ga, nga = scan_of(model, n, TRUE_POSE, 100 + i)
        for j, win in enumerate(WINDOWS):
            for ht in HALF_THETAS:
                R0, t0 = pose_Rt(TRUE_POSE[0] + 0.2 + RES * ((i + j) % 4), TRUE_POSE[1] - 0.3, TRUE_POSE[2] + 0.02)
                out.append(("n%d_w%dx%d_t%d" % (n, win[0], win[1], ht), ga, nga, R0, t0, win, ht))
    ga, nga = scan_of(model, 200, TRUE_POSE, 200)
    # the wall's table ends at x = 3 m + K cells: a start 4 m to the right leaves about half the scan outside the window
    R0, t0 = pose_Rt(TRUE_POSE[0] + 4.0, TRUE_POSE[1], TRUE_POSE[2])
    out.append(("half_outside", ga, nga, R0, t0, (8, 8), 4))
    R0, t0 = pose_Rt(TRUE_POSE[0] + 100.0, TRUE_POSE[1] - 250.0, TRUE_POSE[2])
    out.append(("all_outside", ga, nga, R0, t0, (8, 8), 4))
    # the winner in the ragged last block of both axes: candidates a = b = 16 of 17, alone in block (2, 2)
    R0, t0 = pose_Rt(TRUE_POSE[0] - 0.8, TRUE_POSE[1] - 0.8, TRUE_POSE[2])
    out.append(("winner_in_ragged_block", ga, nga, R0, t0, (8, 8), 0))
    # three pieces of staged points, the classes changing inside the second
    ga, nga = scan_of(model, 2100, TRUE_POSE, 201, ga_share=0.6)
    R0, t0 = pose_Rt(TRUE_POSE[0] - 0.3, TRUE_POSE[1] + 0.2, TRUE_POSE[2] - 0.03)
    out.append(("n2100_three_pieces", ga, nga, R0, t0, (8, 8), 0))
    # a point that is not finite and one beyond the lattice are skipped, not fatal
    ga, nga = scan_of(model, 64, TRUE_POSE, 202)
    nga = nga.copy()
    nga[3] = (np.nan, 0.0)
    nga[4] = (np.inf, 1.0)
    nga[5] = (3e8, 0.0)
    out.append(("nonfinite", ga, nga, R0, t0, (8, 8), 0))
    return out


BLOCK_SIZES = (2, 11, 16)                          # candidates of a block per lane of 64: 4 lanes busy; 121 (two, the second
#                                                    ragged); 256 (all four).  The default 8 gives every lane exactly one.
BLOCK_VOLUME_CASES = ("n5_w8x8_t4", "n65_w8x8_t4", "n1081_w2x16_t0", "n65_w0x8_t4", "half_outside", "winner_in_ragged_block")


def block_cases():
    """(name, D, t_ga, t_nga, R0, t0, (half_x, half_y), half_theta) against box_model(), a matcher of its own per D: some of
    volume_cases() and one winner at candidate 218 of a 16 x 16 block, (a, b) = (10, 13), which only a lane's fourth holds."""
    cases = [c for c in volume_cases() if c[0] in BLOCK_VOLUME_CASES]
    assert len(cases) == len(BLOCK_VOLUME_CASES)
    ga, nga = scan_of(box_model(), 200, TRUE_POSE, 200)
    R0, t0 = pose_Rt(TRUE_POSE[0] - 0.2, TRUE_POSE[1] - 0.5, TRUE_POSE[2])
    cases.append(("winner_in_fourth_register", ga, nga, R0, t0, (8, 8), 0))
    return [(c[0], D) + c[1:] for D in BLOCK_SIZES for c in cases]


def tie_case():
    """An exact tie whose winner is NOT in the block the search evaluates first.  Five scan points on cell centres, one angle
    (R0 = identity: cos 1, sin 0 exactly), N = 17 x 17, D = 8, K = 1.  The model is the scan shifted to candidate (a, b) = (0, 1)
    and to (9, 0): both score 5 x 255, the most there is, so both blocks' bounds equal it.  Block (B, A) = (0, 0) is evaluated
    first (lowest index among equal bounds) and gives L = 1275 with candidate (0, 1), flat index 17; the winner is (9, 0), flat
    index 9, in block (0, 1) whose bound is exactly L.  Returns (params kw, m_ga, m_nga, t_ga, t_nga, R0, t0, winner (k, a, b),
    other (k, a, b), score)."""
    cells = np.array([(0, 0), (3, 1), (7, -2), (-4, 5), (11, 6)])
    half = 8
    m = np.concatenate([centre(cells[:, 0] + (0 - half), cells[:, 1] + (1 - half)),
                        centre(cells[:, 0] + (9 - half), cells[:, 1] + (0 - half))])
    kw = dict(resolution=RES, sigma=0.05, kernel_cells=1, block=8, half_x=half, half_y=half, half_theta=0, theta_step=0.01)
    return kw, np.zeros((0, 2)), m, np.zeros((0, 2)), centre(cells[:, 0], cells[:, 1]), np.eye(2), np.zeros(2), (0, 9, 0), (0, 0, 1), 1275


def batch_scans(n_scans):
    """(pts, scan_off, scan_nga, R0 [S, 4], t0 [S, 2]) of n_scans scans of box_model(): sizes vary, the middle one has 4 points"""
    model = box_model()
    sizes = [5, 63, 64, 65, 130, 257, 33]
    pts, off, nga, R, t = [], [0], [], [], []
    for s in range(n_scans):
        n = 4 if (n_scans > 2 and s == n_scans // 2) else sizes[s % len(sizes)]
        g, ng = scan_of(model, n, TRUE_POSE, 300 + s)
        R0, t0 = pose_Rt(TRUE_POSE[0] + 0.1 * (s % 7) - 0.3, TRUE_POSE[1] + 0.1 * (s % 5) - 0.2, TRUE_POSE[2] + 0.01 * (s % 4) - 0.02)
        pts += [g, ng]
        off.append(off[-1] + n)
        nga.append(len(g))
        R.append(R0.reshape(4))
        t.append(t0)
    return (np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
            np.ascontiguousarray(np.array(R)), np.ascontiguousarray(np.array(t)))
