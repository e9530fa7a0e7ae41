"""Hand-built clouds for the ground segmentation (slam_amd/csrc/gseg.hip, oracle/gseg_oracle.c), one per branch of the
sector kernel that benign clouds never take.  Not a test file: tests/test_gseg_cases.py shows on the oracle alone that every
case reaches the branch it is named for and stays clear of every threshold, tests/test_gpu_gseg_branches.py holds the
device to the oracle on them.

A cloud is built in polar form: K points per (sector, 0.5 m range bin), placed well inside the sector and the bin, the
height a function of the bin.  Point j of a bin lies 0.01 j above the bin's height, so point 0 is the prototype and every
other point of a ground bin is a few centimetres from it -- far from p_tg on either side.

A case is a dict:
  name      what it is for
  xyz       [n, 3] f32
  params    parameters that differ from the defaults, by the oracle's names (API_NAMES gives the C-ABI's)
  sector    the sector the case lives in (None: several)
  expect    what the oracle's trace must show, by the keys tests/test_gseg_cases.py:check_expectations knows
  value_tol bound on |device - oracle| of `value` over the bins with state > 0 (1e-9, tests/test_gseg.py's)
"""
import numpy as np

from slam_amd import synth

NA, NL = 72, 200
K = 6                      # points per bin: the least that makes a signal bin (count > 5)
VALUE_TOL = 1e-9
MARGIN_TOL = 1e-6          # every decision of every case is at least this far from its threshold, in its own units

# the oracle's parameter names -> the C-ABI's (slam_gseg_params)
API_NAMES = dict(rmax="rmax", num_seedpoints="num_seedpoints", p_l="gp_lengthparameter", p_sf="gp_covariancescale",
                 p_sn="gp_modelnoise", p_tmodel="gp_groundmodelconfidence", p_tdata="gp_grounddataconfidence",
                 p_tg="gp_groundthreshold", robot_height="robotheight", max_seed_range="seeding_maxrange",
                 max_seed_height="seeding_maxheight")


def api_params(params):
    return {API_NAMES[k]: v for k, v in params.items()}


def bin_points(sec, b, z, k=K, extra=()):
    """k points of bin b of sector sec, point j at height z + 0.01 j, then one point per entry of `extra` at z + entry;
    ranges within [b + 0.25, b + 0.75) half-metres, azimuths within the middle 60 % of the sector"""
    out = []
    for j in range(k + len(extra)):
        rho = 0.5 * (b + 0.25 + 0.5 * (j % k) / k)
        ang = np.deg2rad(5.0 * (sec + 0.2 + 0.6 * ((5 * j + b) % 7) / 7.0))
        dz = 0.01 * j if j < k else extra[j - k]
        out.append((rho * np.cos(ang), rho * np.sin(ang), z + dz))
    return out


def sector_cloud(sec, bins, z_of, k=K, extra_of=None):
    pts = []
    for b in bins:
        pts += bin_points(sec, b, z_of(b), k, extra_of(b) if extra_of else ())
    return np.asarray(pts, np.float64).astype(np.float32)


def flat(b):
    return -1.7


def case(name, xyz, params=None, sector=None, value_tol=VALUE_TOL, **expect):
    return dict(name=name, xyz=np.ascontiguousarray(xyz, np.float32), params=dict(params or {}), sector=sector, expect=expect,
                value_tol=value_tol)


RAMP = dict(p_tdata=1.0, p_sn=0.01, p_l=2.0, p_tmodel=0.2)


def ramp(b):
    r = 0.5 * (b + 0.25)
    return -1.7 + 0.004 * r * r


def octant_cloud():
    """6 points on each axis and diagonal direction at dyadic coordinates (one range bin per direction), and 6 just
    below the +x axis: atan2(-1e-30, r) * 180/pi + 360 rounds to 360.0, sector 72, clamped to 71"""
    pts, where = [], []
    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    for o, (dx, dy) in enumerate(dirs):
        diag = dx != 0 and dy != 0
        for j in range(K):
            r = 8.25 + j / 32.0 if diag else 10.0 + j / 16.0          # (8.25 .. 8.40625) sqrt 2 = 11.67 .. 11.89: one bin
            pts.append((dx * r, dy * r, -1.7 + 0.01 * j))
        where.append((9 * o, 23 if diag else 20))          # where libm puts them: 45 o degrees is the floor of sector 9 o
    for j in range(K):
        pts.append((20.0 + j / 16.0, -1e-30, -1.7 + 0.01 * j))
    where.append((71, 40))
    return np.asarray(pts, np.float32), where


def height_tie_cloud(sec=20):
    """Bins 15..20 with the bit-equal prototype height -0.5 and bins 9..14 with +-0.0f: ten seeds, so the cut falls inside
    the second tie and takes bins 9..12 by their index.  In bin 12 the first point is +0.0f at one range and a later one
    -0.0f at another: `pz < proto_z` keeps the first, and the bin's range is that point's.  The raised bins 30..33 stay
    candidates: their GP mean is taken at the model's ranges, bin 12's among them, 0.17 m apart between the two points."""
    pts = []
    for b in list(range(15, 21)) + list(range(9, 15)):
        p = np.asarray(bin_points(sec, b, -0.5 if b >= 15 else 0.0))
        if b == 12:
            p[4, 2] = -0.0
        pts.append(p)
    for b in range(30, 34):
        pts.append(np.asarray(bin_points(sec, b, 9.0)))
    xyz = np.concatenate(pts).astype(np.float32)
    i = 9 * K          # bin 12's first point
    assert not np.signbit(xyz[i, 2]) and xyz[i, 2] == 0 and np.signbit(xyz[i + 4, 2]) and xyz[i + 4, 2] == 0
    assert abs(np.hypot(*xyz[i, :2]) - np.hypot(*xyz[i + 4, :2])) > 0.1
    return xyz


def tie_one_seed_cloud(sec=21):
    """three bins, given as 30, 12, 25, with one prototype height: the one seed is bin 12, the lowest index, and with a
    model of one bin the others are dropped"""
    return np.concatenate([sector_cloud(sec, [b], lambda b: -1.0) for b in (30, 12, 25)])


def gate_order_cloud(sec=33):
    """Sorted by height: bins 120, 121 (beyond the seed range), 10, 122, 11, 12, 130 (|z| past the seed height) ... : the
    seeds are not a prefix of the sorted list, and the candidates keep their sorted order around them."""
    z = {120: -2.00, 121: -1.98, 10: -1.96, 122: -1.94, 11: -1.92, 12: -1.90, 123: -1.88, 13: -1.86}
    pts = []
    for b, zb in z.items():
        pts += bin_points(sec, b, zb)
    pts += bin_points(sec, 20, -16.0)          # the lowest of all, and too low to be a seed
    for b in range(14, 20):
        pts += bin_points(sec, b, -1.7)
    return np.asarray(pts, np.float64).astype(np.float32)


def synth_small():
    return synth.make_cloud3d(7, n_loop=50, rings=16, n_az=512)[0]


def long_run_cloud(sec=50, run=230):
    """`run` consecutive points of one bin (a run of equal bins that fills a wavefront and crosses three), its lowest point
    in the middle, between ordinary bins"""
    head = sector_cloud(sec, range(8, 20), flat)
    tail = sector_cloud(sec, range(21, 30), flat)
    j = np.arange(run)
    rho = 0.5 * (20 + 0.25 + 0.5 * (j % 16) / 16.0)
    ang = np.deg2rad(5.0 * (sec + 0.2 + 0.6 * (j % 11) / 11.0))
    z = -1.7 + 0.001 * np.abs(j - 137) + 0.0005
    mid = np.stack([rho * np.cos(ang), rho * np.sin(ang), z], 1).astype(np.float32)
    return np.concatenate([head, mid, tail])


def with_stride(xyz, stride=8):
    out = np.full((len(xyz), stride), 7.0, np.float32)
    out[:, :3] = xyz
    return out


def cases():
    out = []
    # (raised to +8 m: at +2.5 m the raised bins beyond the seeds' reach, where the GP says 0 +- 1, are inliers: 6 of 36 stay out)
    big = sector_cloud(5, range(4, 184), lambda b: 8.0 if b % 5 == 0 else -1.7,
                       extra_of=lambda b: (0.7, 2.0) if b % 5 == 1 else ())
    out.append(case("big_model", big, sector=5, seeds=10, rounds=2, model=144, left=36, over64=1, last_round_adds=0))
    out.append(case("ramp", sector_cloud(11, range(4, 120), ramp), RAMP, sector=11, min_rounds=3, max_entering=64, min_left=1))
    out.append(case("ramp_big", sector_cloud(12, range(4, 184), ramp_big), RAMP_BIG, sector=12, min_rounds=3, over64=3,
                    over64_distinct=3, min_left=1))
    out.append(case("all_seeds", sector_cloud(2, range(6, 14), flat), sector=2, seeds=8, rounds=0, model=8, left=0))
    one = sector_cloud(40, [20], flat)
    out.append(case("one_seed", one, sector=40, seeds=1, rounds=0, model=1, left=0, ground=K, dropped=0))
    far = sector_cloud(40, range(101, 121), flat)
    out.append(case("one_seed_plus", np.concatenate([one, far]), sector=40, seeds=1, rounds=0, model=1, left=0, ground=K,
                    dropped=len(far)))
    out.append(case("no_seed_high", sector_cloud(41, range(6, 26), lambda b: 16.0 if b % 2 else -16.0), sector=41, seeds=0,
                    rounds=0, model=0, left=0, ground=0, dropped=20 * K))
    out.append(case("no_seed_far", far, sector=40, seeds=0, rounds=0, model=0, left=0, ground=0, dropped=len(far)))
    flat36 = sector_cloud(60, range(10, 46), flat)
    out.append(case("seed0", flat36, dict(num_seedpoints=0), sector=60, seeds=1, rounds=0, model=1, left=0, ground=K,
                    dropped=35 * K))
    out.append(case("seed0_gate", np.concatenate([sector_cloud(60, [110], lambda b: -1.9), flat36]), dict(num_seedpoints=0),
                    sector=60, seeds=0, rounds=0, model=0, left=0, ground=0, dropped=37 * K))
    out.append(case("seed1", flat36, dict(num_seedpoints=1), sector=60, seeds=1, rounds=0, model=1, left=0, ground=K,
                    dropped=35 * K))
    out.append(case("seed200", sector_cloud(61, range(4, 190), flat), dict(num_seedpoints=200, max_seed_range=200.0), sector=61,
                    seeds=186, rounds=0, model=186, left=0, ground=186 * K, dropped=0))
    out.append(case("gate_order", gate_order_cloud(), sector=33, seeds=10, rounds=2, model=14, left=1, seeds_not_a_prefix=True))
    out.append(case("height_ties", height_tie_cloud(), sector=20, seeds=10, rounds=2, model=12, left=4))
    out.append(case("height_ties_one_seed", tie_one_seed_cloud(), dict(num_seedpoints=1), sector=21, seeds=1, rounds=0, model=1,
                    left=0, bins_state1=[21 * NL + 12], ground=K, dropped=2 * K))
    octs, where = octant_cloud()
    out.append(case("octants", octs, sector=None, bins_state1=[s * NL + b for s, b in where], ground=9 * K, dropped=0))
    three = np.concatenate([sector_cloud(s, range(6, 30), flat, extra_of=lambda b: (0.7, 2.0) if b % 4 == 0 else ())
                            for s in (0, 35, 71)])
    out.append(case("empty_sectors", three, sector=None, occupied_sectors=[0, 35, 71], dropped=0))
    # ---- order and shape variants
    rs = np.random.RandomState(5)
    out.append(case("big_model_shuffled", big[rs.permutation(len(big))], sector=5, seeds=10, rounds=2, model=144, left=36,
                    over64=1, same_as="big_model"))
    small = synth_small()
    # (more points than the 14 400 bins: the label kernel's launch is sized by the cloud here, by the bins after it)
    out.append(case("synth_big", synth.make_cloud3d(0, n_loop=50, rings=32, n_az=1024)[0], sector=None))
    out.append(case("synth", small, sector=None))
    out.append(case("synth_shuffled", small[rs.permutation(len(small))], sector=None, same_as="synth"))
    for n in (1, 63, 65, 257, 8191):
        assert n <= len(small)
        out.append(case("synth_n%d" % n, small[:n], sector=None))
    for n in (1, 63, 65, 257):
        out.append(case("big_model_n%d" % n, big[:n], sector=5))
    run = long_run_cloud()
    out.append(case("long_run", run, sector=50, seeds=10, model=22, left=0, ground=len(run), longest_run=230))
    out.append(case("long_run_stride8", with_stride(run), sector=50, seeds=10, model=22, left=0, same_as="long_run"))
    return out


def ramp_big(b):
    r = 0.5 * (b + 0.25)
    return -1.7 + 0.002 * r * r


RAMP_BIG = dict(RAMP, p_l=4.0)          # (with p_l = 2 no ramp of 180 bins takes the model past 59)
