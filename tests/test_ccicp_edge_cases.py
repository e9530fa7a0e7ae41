"""The plain references of tests/ccicp_edge_cases.py held to the oracle on every case, and the preconditions
tests/test_gpu_ccicp_edges.py relies on, checked on the references alone: no GPU here."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ccicp_edge_cases as E
import oracle_lib as O
from slam_amd import synth


@pytest.mark.parametrize("case", E.voxel_cases(), ids=lambda c: c["name"])
def test_exact_voxel_reference_is_the_oracle(case):
    """same voxels, same order, same flags; xyz within the 1e-5 the project allows between the oracle's double sums and
    the device's fixed point"""
    ref = E.voxel_exact(case["pts"], case["flags"], case["leaf"])
    out, n = O.voxel_downsample(E.for_oracle(case["pts"], case["flags"]), case["leaf"])
    assert n == len(ref["idx"]) > 0
    assert np.array_equal(out[:, 3], ref["flag"])
    assert np.abs(out[:, :3] - ref["fix"]).max() < 1e-5 and np.abs(out[:, :3] - ref["true"]).max() < 1e-5
    assert (np.diff(ref["idx"]) > 0).all() and ref["count"].sum() == np.isfinite(E.for_oracle(case["pts"], case["flags"])[:, :3]).all(1).sum()
    # what the case says about its coordinates: multiples of 2^-24 (bound A alone) within +-300 m, or not
    p = case["pts"][:, :3][np.isfinite(case["pts"][:, :3])].astype(np.float64)
    assert np.abs(p).max() <= 300.0
    assert case["dyadic"] == bool((p * E.FIX == np.rint(p * E.FIX)).all())
    if case["dyadic"]:
        assert np.array_equal(ref["fix"], ref["true"])
    else:
        assert np.abs(ref["fix"] - ref["true"]).max() <= E.QUANT
    # the Fractions are what the doubles round
    assert all(float(f) == ref["fix"][v, d] for v, row in enumerate(ref["frac"]) for d, f in enumerate(row))


def test_exact_voxel_reference_by_hand():
    pts = np.float32([[0.25, 0.25, 0.5], [0.375, 0.125, 1.5], [0.0, 0.0, 0.0], [-0.125, 0.25, 0.5], [np.nan, 0, 0], [7.0, 7.0, 7.0]])
    flags = np.uint8([1, 1, 0, 1, 1, 255])
    ref = E.voxel_exact(pts, flags)
    assert ref["idx"].tolist() == [0, 1] and ref["count"].tolist() == [1, 3] and ref["n_ga"].tolist() == [1, 2]
    assert ref["frac"][1] == [Fraction(5, 24), Fraction(1, 8), Fraction(2, 3)] and ref["frac"][0] == [Fraction(-1, 8), Fraction(1, 4), Fraction(1, 2)]
    assert ref["flag"].tolist() == [1.0, 0.0]                       # 2 / 3 truncates
    assert len(E.voxel_exact(pts[4:], flags[4:])["idx"]) == 0


def test_run_cloud_is_what_it_says():
    pts, flags, runs = E.run_cloud()
    ref = E.voxel_exact(pts, flags)
    assert sorted({r[1] for r in runs}) == sorted(E.RUN_LENGTHS) and {r[0] % 64 for r in runs} == set(E.RUN_OFFSETS)
    assert len(runs) == len(E.RUN_LENGTHS) * len(E.RUN_OFFSETS)
    inv = np.float32(1) / np.float32(E.LEAF)
    cell = np.floor(pts * inv)
    change = np.flatnonzero((cell[1:] != cell[:-1]).any(1)) + 1
    starts = np.r_[0, change].tolist()
    lengths = np.diff(np.r_[0, change, len(pts)]).tolist()
    for first, length in runs:                                       # each is a maximal run of one voxel that occurs nowhere else
        assert lengths[starts.index(first)] == length
    assert len(ref["idx"]) == len(starts) and sorted(ref["count"].tolist()) == sorted(lengths)
    assert any((first + length) % 256 == 0 for first, length in runs) or any(first % 256 == 0 for first, _ in runs)   # a block edge


def test_ulp_and_bounds():
    assert E.ulp32(1.0) == 2.0 ** -23 and E.ulp32(0.99) == 2.0 ** -24 and E.ulp32(-300.0) == 2.0 ** -15 and E.ulp32(0.0) == 2.0 ** -149
    x = np.float64([0.3, 1.7, -123.456, 2.0 ** -130])
    assert np.array_equal(E.ulp32(x), np.abs(np.spacing(x.astype(np.float32))).astype(np.float64))
    assert (np.abs(x.astype(np.float32).astype(np.float64) - x) <= E.centroid_bound(x)).all()        # a correctly rounded float meets A
    assert not (np.abs(np.nextafter(x.astype(np.float32), np.float32(np.inf)).astype(np.float64) - x) <= E.centroid_bound(x)).all()
    assert E.centroid_bound(1.0, dyadic=False) - E.centroid_bound(1.0) == E.QUANT == 2.0 ** -25


def test_ordered_float_decode():
    vals = np.float32([-np.inf, -300.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, 300.5, np.inf])
    words = [E.order_f32(v) for v in vals]
    assert words == sorted(words) and len(set(words)) == len(words)  # -0.0 orders below +0.0
    for v, w in zip(vals, words):
        assert E.unorder_f32(w).tobytes() == v.tobytes()
    assert 0 < words[0] and words[-1] < 0xffffffff                    # the initial words (0xffffffff / 0) are no value's


def test_quaternion_helper():
    """reproduces the hand-built pitch-then-yaw quaternions of test_gpu_height_matches_oracle; yaw from the matched rotation"""
    rs = np.random.RandomState(2)
    for trial in range(6):
        yaw, pitch = rs.uniform(-3, 3), rs.uniform(-0.05, 0.05)
        q = np.array([0, np.sin(pitch / 2), 0, np.cos(pitch / 2)])
        qz = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
        quat = [qz[3] * q[0] + qz[0] * q[3] + qz[1] * q[2] - qz[2] * q[1],
                qz[3] * q[1] - qz[0] * q[2] + qz[1] * q[3] + qz[2] * q[0],
                qz[3] * q[2] + qz[0] * q[1] - qz[1] * q[0] + qz[2] * q[3],
                qz[3] * q[3] - qz[0] * q[0] - qz[1] * q[1] - qz[2] * q[2]]
        assert np.abs(np.array(E.quat_rpy(0.0, pitch, yaw)) - quat).max() < 1e-15
        rs.uniform(size=3)
    assert E.quat_rpy(0, 0, 0) == [0, 0, 0, 1] and np.allclose(E.quat_rpy(0.2, 0, 0), [math.sin(0.1), 0, 0, math.cos(0.1)], atol=1e-16)
    # roll, then pitch, then yaw about the fixed axes: the rotation matrix of the quaternion is Rz(yaw) Ry(pitch) Rx(roll)
    r, p, y = 0.1, -0.03, 2.5
    x, yy, z, w = E.quat_rpy(r, p, y)
    M = np.array([[1 - 2 * (yy * yy + z * z), 2 * (x * yy - w * z), 2 * (x * z + w * yy)], [2 * (x * yy + w * z), 1 - 2 * (x * x + z * z), 2 * (yy * z - w * x)],
                  [2 * (x * z - w * yy), 2 * (yy * z + w * x), 1 - 2 * (x * x + yy * yy)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    assert np.abs(M - Rz @ Ry @ Rx).max() < 1e-15
    names = dict(E.YAW_R)
    assert E.yaw_of(names["pi exactly"]) == math.pi and E.yaw_of(names["pi/2 exactly"]) == math.pi / 2 and E.yaw_of(names["-pi/2"]) == -math.pi / 2
    assert all(-math.pi < E.yaw_of(R) <= math.pi for R in names.values())
    # the wheel points of the restatement here are the oracle's: a ground cloud made of them is found at distance zero
    pose = E.pose_of(E.rot2(0.4), (0.3, -0.2), 0.1, 0.1, -0.03)
    z, nc, idx = O.ccicp_height(E.wheel_points(pose), pose)
    assert nc == 4 and idx == [0, 1, 2, 3]
    assert np.array_equal(E.wheel_points(E.IDENTITY), np.concatenate([E.UNDER, np.full((4, 1), np.float32(-1.45))], 1))


# ---------------------------------------------------------------- preconditions of the GPU tests (conditions, not measurements)
def test_neighbour_margin_of_every_height_case():
    """for every wheel point the second-nearest ground point is more than 1e-3 m farther than the nearest: neither a last-bit
    difference of the device's sin / cos / atan2 nor the order of a float sum can change a neighbour"""
    ground = E.ground_patch()
    n = 0
    for name, R, t, z0, roll, pitch in E.rpy_cases():
        pose = E.pose_of(R, t, z0, roll, pitch)
        assert E.neighbour_margin(ground, pose).min() > 1e-3, name
        z, nc, idx = O.ccicp_height(ground, pose)
        assert nc == 4 and len(set(idx)) == 4, name                   # a plane through four different points
        n += 1
    assert n == 25 * len(E.YAW_R)
    for size, k in E.index_cases():
        g = E.indexed_ground(size, k)
        assert E.neighbour_margin(g, E.IDENTITY).min() > 1e-3 or size == 1, (size, k)
        z, nc, idx = O.ccicp_height(g, E.IDENTITY)
        assert idx[0] == k and nc == 4 and (size == 1 or len(set(idx)) == 4), (size, k)
    assert sorted({k for _, k in E.index_cases()}) == [0, 254, 255, 256, 1024] and {s for s, _ in E.index_cases()} == set(E.GROUND_SIZES)


def test_gate_and_degenerate_cases_on_the_oracle():
    q = E.wheel_points(E.IDENTITY)
    for inward in (False, True):
        g = E.gate_ground(inward)
        d = g[3] - q[3]
        dd = np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]) + np.float32(d[2] * d[2])
        assert (dd < np.float32(9.0)) == inward and (inward or (d[0] == 3.0 and dd == 9.0))   # exactly 3 m: outside the gate
        assert E.neighbour_margin(g, E.IDENTITY).min() > 0.1
        for z0 in (0.0, 0.25):
            z, nc, idx = O.ccicp_height(E.gate_ground(inward, z0), [0, 0, z0, 0, 0, 0, 1])
            assert idx == [0, 1, 2, 3] and nc == (4 if inward else 3) and (z == z0) == (not inward)
    for name, g in E.degenerate_grounds():
        z, nc, idx = O.ccicp_height(g, [0, 0, 0.25, 0, 0, 0, 1])
        assert nc == 4 and np.isfinite(z), name


def chain_reference(cloud, voxel, crop):
    return E.chain_reference(O, synth.make_cloud3d(**E.CHAIN_RINGS)[0], cloud, voxel, crop)


@pytest.mark.parametrize("voxel", (1, 0))
@pytest.mark.parametrize("crop", E.CHAIN_CROPS, ids=str)
@pytest.mark.parametrize("cloud", E.CHAIN_CLOUDS)
def test_chain_reference_margins_and_caps(cloud, voxel, crop):
    ref = chain_reference(cloud, voxel, crop)
    n_ga, n_nga = len(ref["ga"]), len(ref["nga"])
    assert 8 * 512 < len(ref["xyz"]) <= 16 * 512 + 3000 and len(ref["gnd"]) > 500 and ref["n_obs"] > 2000
    if crop is not None:
        # crop margin: no centroid within 1e-3 m of a face, so that the device's centroid (within bound A + B of the reference's)
        # lies on the same side
        box = np.float32([-E.CHAIN_CROP_DIST + crop[0], E.CHAIN_CROP_DIST + crop[0], -E.CHAIN_CROP_DIST + crop[1], E.CHAIN_CROP_DIST + crop[1]])
        d = np.abs(np.concatenate([ref["flt"][:, 0:1] - box[:2], ref["flt"][:, 1:2] - box[2:]], 1).astype(np.float64))
        assert d.min() > 1e-3 or not voxel                            # (without the voxel filter the rows are the cloud's own: exact)
        assert 0 < ref["keep"].sum() < len(ref["flt"])                # the crop bites
    if voxel:
        assert np.abs(ref["vox"]["fix"] - ref["vox"]["true"]).max() <= E.QUANT
    # cap cases really hit their caps: cap - 1 is the limit
    caps = E.chain_caps(n_ga)
    assert n_ga > 50 and (n_nga > 50 or cloud == "rings")
    for cap in caps:
        assert (min(n_ga, cap - 1) < n_ga) == (cap <= n_ga)
    assert sum(min(n_ga, cap - 1) < n_ga for cap in caps) == 4 and (sum(min(n_nga, cap - 1) < n_nga for cap in caps) >= 3 or cloud == "rings")
    # the oracle's split says the same
    for cap in (50, n_ga):
        ga, nga = O.ccicp_split(ref["flt"], ref["keep"], cap)
        assert np.array_equal(ga, ref["flt"][ref["ga"]][:cap - 1, :2].astype(np.float64))
        assert np.array_equal(nga, ref["flt"][ref["nga"]][:cap - 1, :2].astype(np.float64))


def test_far_cloud_has_obstacle_points_and_the_classification_drops_them_all():
    far = E.far_cloud()
    lab = O.gseg_segment(far, O.gseg_params(rmax=E.FAR_RMAX))[0]
    obs = far[lab >= O.GSEG_OBSTACLE]
    assert len(obs) > 5 and (O.classify_ga(obs) == 255).all()
    assert (O.gseg_segment(far)[0][4000:] == O.GSEG_DROPPED).all()


def test_split_references_and_cap_cloud():
    pts = E.cap_cloud()
    cx, cy, crop = E.CROP_WIDE
    box = (np.float32(-crop + cx), np.float32(crop + cx), np.float32(-crop + cy), np.float32(crop + cy))
    keep = O.ccicp_crop(pts, cx, cy, crop)
    assert np.array_equal(keep, E.box_keep(pts, box))
    ga, nga, totals = E.split_reference(pts, box)
    assert min(totals) > 1026                                         # every cap of cap_values bites on both classes
    for cap in E.cap_values(totals[0]):
        a, b, t = E.split_reference(pts, box, cap)
        oa, ob = O.ccicp_split(pts, keep, cap)
        assert np.array_equal(a, oa) and np.array_equal(b, ob) and t == totals
        assert len(a) == min(totals[0], cap - 1) and len(b) == min(totals[1], cap - 1)
    # the face cloud: CROP_BOX is the float box of ccicp_crop(CROP_CUR); a point on a face stays, one step outside goes
    f = E.face_cloud()
    keep = O.ccicp_crop(f, *E.CROP_CUR)
    assert np.array_equal(keep, E.box_keep(f, E.CROP_BOX))
    assert keep[:8].tolist() == [True, False] * 4 and keep[8:13].all() and not keep[13:18].any() and keep[18:].all()
    a, b, t = E.split_reference(f, E.CROP_BOX)
    oa, ob = O.ccicp_split(f, keep, len(f) + 2)
    assert np.array_equal(a, oa) and np.array_equal(b, ob)
    ga_rows = np.flatnonzero(E.box_keep(f, E.CROP_BOX) & (f[:, 3] > 0.5)).tolist()
    assert 19 in ga_rows and 18 not in ga_rows and 20 not in ga_rows and 21 not in ga_rows and 22 in ga_rows   # 0.5: NGA, next up: GA, NaN: NGA
    a, b, t = E.split_reference(f, None)                              # no crop: non-finite points pass through
    oa, ob = O.ccicp_split(f, None, len(f) + 2)
    assert np.array_equal(a, oa, equal_nan=True) and np.array_equal(b, ob, equal_nan=True) and sum(t) == len(f)


def test_compaction_cases():
    assert E.shrink_and_grow()[:4] == [68 * 1024 + 7, 1, 65 * 1024 + 1, 3] and sorted(E.shrink_and_grow()) == sorted(E.COMPACT_SIZES)
    assert sum(n > 64 * E.BLOCK for n in E.COMPACT_SIZES) == 3         # more than 64 blocks: the look-back's second round
    for n in (1, 5, 1025, 68 * 1024 + 7):
        names = [p[0] for p in E.patterns(n)]
        assert len(names) == 9 and all(len(sel) == n for _, sel in E.patterns(n))
        c = E.cloud_of(n)
        assert len(np.unique(c[:, 0])) == n and np.array_equal(E.strided(c, 7)[:, :3], c) and np.isnan(E.strided(c, 7)[:, 3:]).all()


def test_ga_and_pack_cases():
    for name, pts, cnt in E.ga_cases():
        flags = O.classify_ga(pts[:cnt])
        ext = E.extent_words(pts[:cnt], flags)
        if name in ("every point dropped", "count 0"):
            assert ext is None and (flags == 255).all(), name
        else:
            assert ext is not None and (ext[:3] <= ext[3:]).all() and set(flags.tolist()) >= {0, 1}, name
        if name == "finite xy, non-finite z":
            assert flags[5] != 255 and ext[3] < 100.0 and (flags[~np.isfinite(pts[:cnt, 2])] != 255).all()
        if name == "count below the capacity, outliers behind it":
            full = E.extent_words(pts, O.classify_ga(pts))
            assert cnt < len(pts) and full[3] > ext[3] + 100
        if name == "+-0.0":
            assert (ext[3:] == 0).all()
    a, r = E.ga_disjoint_pair()
    alone, both = O.classify_ga(r), O.classify_ga(np.concatenate([a, r]))[len(a):]
    assert (alone != both).sum() > 20 and (alone == 1).any()           # stale cells of the first cloud would show
    ba = np.floor((a[:, :2].astype(np.float64) + 300) / 0.5)
    br = np.floor((r[:, :2].astype(np.float64) + 300) / 0.5)
    assert not set(map(tuple, ba)) & set(map(tuple, br))
    seen = set()
    for name, scenes in E.pack_cases():
        assert 1 <= len(scenes) <= 32 and all(g in (0, s) for s, g in scenes)
        seen |= {s for s, _ in scenes}
    assert seen == set(E.PACK_SIZES) and {len(s) for _, s in E.pack_cases()} >= {1, 2, 32}
