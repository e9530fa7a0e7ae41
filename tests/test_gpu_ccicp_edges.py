"""The CCICP chain's device entry points at their edges, each against a plain reference (tests/ccicp_edge_cases.py: numpy, Python
integers and the oracle's pieces; tests/test_ccicp_edge_cases.py holds those references to the oracle on the CPU).  Every
output buffer is filled with a sentinel byte before a call; rows past the returned count must still hold it afterwards.
docs/CCICP_EDGES.md has the case table, the two arithmetic bounds of a voxel centroid and which entry point each test reaches."""
import ctypes as C

import numpy as np
import pytest

import ccicp_edge_cases as E
import oracle_lib as O
from slam_amd import api, synth

pytestmark = pytest.mark.gpu


def chain_reference(cloud, voxel, crop):
    return E.chain_reference(O, synth.make_cloud3d(**E.CHAIN_RINGS)[0], cloud, voxel, crop)


# ------------------------------------------------------------------ helpers
def dev(shape, dtype):
    """a device block holding the sentinel byte throughout"""
    d = api.DeviceArray(shape if isinstance(shape, tuple) else (shape,), dtype)
    refill(d)
    return d


def refill(d):
    api.check(api.lib().slam_memset(d.ptr, E.SENTINEL, d.nbytes, None))


def put(d, a):
    """the first a.nbytes of d"""
    a = np.ascontiguousarray(a)
    assert a.nbytes <= d.nbytes
    if a.nbytes:
        api.check(api.lib().slam_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes, None))


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == E.SENTINEL).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def i32(*v):
    return api.DeviceArray.from_host(np.array(v, np.int32))


def centroids_ok(got, ref, rows=slice(None), cols=3, dyadic=True):
    """bound A against the fixed-point mean, and A + B against the true mean where the coordinates are no multiples of 2^-24"""
    got = np.asarray(got, np.float64)
    fix, true = ref["fix"][rows][:, :cols], ref["true"][rows][:, :cols]
    ok = (np.abs(got - fix) <= E.centroid_bound(fix)).all()
    return bool(ok and (dyadic or (np.abs(got - true) <= E.centroid_bound(true, dyadic=False)).all()))


# ------------------------------------------------------------------ compaction against numpy
def test_select_against_numpy_on_one_handle():
    """slam_ccicp_select_dev: every size x every selection pattern on ONE handle, shrink and grow (stale look-back words of
    another epoch in the way), strides 3, 4 and 7 with NaN padding; rows and counts equal the boolean-mask result bit for bit"""
    L, cc = api.lib(), api.Ccicp()
    nmax = max(E.COMPACT_SIZES)
    d_in, d_lab, d_out = api.DeviceArray((nmax * 7,), np.float32), api.DeviceArray((nmax,), np.uint8), api.DeviceArray((nmax + 1, 4), np.float32)
    call = 0
    for n in E.shrink_and_grow():
        cloud = E.cloud_of(n)
        out = d_out.view(0, (n + 1, 4))
        for name, sel in E.patterns(n):
            stride = (3, 4, 7)[call % 3]
            call += 1
            lab = np.where(sel, 2 + np.arange(n) % 2, np.arange(n) % 2).astype(np.uint8)     # obstacle / overhead against dropped / ground
            put(d_in, E.strided(cloud, stride))
            put(d_lab, lab)
            refill(out)
            cnt = C.c_int(-1)
            api.check(L.slam_ccicp_select_dev(cc.h, d_in.ptr, n, stride, d_lab.ptr, (1 << 2) | (1 << 3), d_out.ptr, C.byref(cnt), None))
            got, want = out.download(), cloud[sel]
            assert cnt.value == len(want), (n, name, stride)
            assert same_bits(got[:len(want), :3], want) and (got[:len(want), 3] == 0).all(), (n, name, stride)
            assert untouched(got[len(want):]), (n, name, stride)
    cc.close()


def test_split_box_both_classes_against_numpy_on_one_handle():
    """slam_ccicp_split_box_dev without a box and without a cap that bites: the GA class is the selection, the NGA class its
    complement -- two compactions per call, against the mask and against the oracle's split"""
    L, cc = api.lib(), api.Ccicp()
    nmax = max(E.COMPACT_SIZES)
    d_in = api.DeviceArray((nmax * 7,), np.float32)
    d_ga, d_nga = api.DeviceArray((nmax + 1, 2), np.float64), api.DeviceArray((nmax + 1, 2), np.float64)
    call = 0
    for n in E.shrink_and_grow():
        cloud = E.cloud_of(n, seed=1)
        ga, nga = d_ga.view(0, (n + 1, 2)), d_nga.view(0, (n + 1, 2))
        for name, sel in E.patterns(n, seed=1):
            stride = (4, 7)[call % 2]
            call += 1
            pts = np.concatenate([cloud, sel[:, None].astype(np.float32)], 1)
            put(d_in, E.strided(pts, stride))
            refill(ga)
            refill(nga)
            counts, totals = (C.c_int * 2)(-1, -1), (C.c_int * 2)(-1, -1)
            api.check(L.slam_ccicp_split_box_dev(cc.h, d_in.ptr, n, stride, None, n + 2, d_ga.ptr, d_nga.ptr, counts, totals, None))
            want_ga, want_nga, tot = E.split_reference(pts, None)
            assert list(counts) == list(totals) == list(tot) == [int(sel.sum()), n - int(sel.sum())], (n, name)
            got_ga, got_nga = ga.download(), nga.download()
            assert same_bits(got_ga[:tot[0]], want_ga) and untouched(got_ga[tot[0]:]), (n, name, stride)
            assert same_bits(got_nga[:tot[1]], want_nga) and untouched(got_nga[tot[1]:]), (n, name, stride)
            if call % 9 == 0:                                          # (the oracle agrees with the mask: once per size)
                o_ga, o_nga = O.ccicp_split(pts, None, n + 2)
                assert same_bits(o_ga, want_ga) and same_bits(o_nga, want_nga)
    cc.close()


def test_split_box_caps_that_bite():
    """cap - 1 is the limit; 1025 / 1026 put it on the edge of a compaction block.  counts are capped, totals are not, and
    nothing is written behind the limit"""
    L, cc = api.lib(), api.Ccicp()
    pts = E.cap_cloud()
    cx, cy, crop = E.CROP_WIDE
    box = (C.c_float * 4)(-crop + cx, crop + cx, -crop + cy, crop + cy)
    keep = O.ccicp_crop(pts, cx, cy, crop)
    d_in = api.DeviceArray.from_host(pts)
    total = E.split_reference(pts, tuple(box))[2]
    d_ga, d_nga = dev((max(total) + 8, 2), np.float64), dev((max(total) + 8, 2), np.float64)
    for which in (0, 1):
        for cap in E.cap_values(total[which]):
            refill(d_ga)
            refill(d_nga)
            counts, totals = (C.c_int * 2)(-1, -1), (C.c_int * 2)(-1, -1)
            api.check(L.slam_ccicp_split_box_dev(cc.h, d_in.ptr, len(pts), 4, box, cap, d_ga.ptr, d_nga.ptr, counts, totals, None))
            want_ga, want_nga, tot = E.split_reference(pts, tuple(box), cap)
            o_ga, o_nga = O.ccicp_split(pts, keep, cap)
            assert same_bits(o_ga, want_ga) and same_bits(o_nga, want_nga)
            assert list(totals) == list(total) == list(tot) and list(counts) == [min(t, cap - 1) for t in total], cap
            got_ga, got_nga = d_ga.download(), d_nga.download()
            assert same_bits(got_ga[:counts[0]], want_ga) and untouched(got_ga[counts[0]:]), cap
            assert same_bits(got_nga[:counts[1]], want_nga) and untouched(got_nga[counts[1]:]), cap
    # slam_ccicp_split_dev forms the same box from the pose
    counts = (C.c_int * 2)(-1, -1)
    api.check(L.slam_ccicp_split_dev(cc.h, d_in.ptr, len(pts), 4, 1, cx, cy, crop, 1026, d_ga.ptr, d_nga.ptr, counts, None))
    assert list(counts) == [1025, 1025] and same_bits(d_ga.download()[:1025], E.split_reference(pts, tuple(box), 1026)[0])
    cc.close()


@pytest.mark.parametrize("stride", (4, 7))
def test_split_box_faces_non_finite_points_and_flag_values(stride):
    """points exactly on each face of the box are kept, one step outside dropped, -0.0 meets a 0.0 face; non-finite points are
    dropped when a box is given and pass through when it is null; 0.5 is NGA, the next float up GA, NaN NGA"""
    L, cc = api.lib(), api.Ccicp()
    pts = E.face_cloud()
    d_in = api.DeviceArray.from_host(E.strided(pts, stride))
    d_ga, d_nga = dev((len(pts) + 1, 2), np.float64), dev((len(pts) + 1, 2), np.float64)
    for box in (E.CROP_BOX, None):
        refill(d_ga)
        refill(d_nga)
        counts, totals = (C.c_int * 2)(-1, -1), (C.c_int * 2)(-1, -1)
        api.check(L.slam_ccicp_split_box_dev(cc.h, d_in.ptr, len(pts), stride, (C.c_float * 4)(*box) if box else None, len(pts) + 2,
                                             d_ga.ptr, d_nga.ptr, counts, totals, None))
        want_ga, want_nga, tot = E.split_reference(pts, box)
        o_ga, o_nga = O.ccicp_split(pts, O.ccicp_crop(pts, *E.CROP_CUR) if box else None, len(pts) + 2)
        assert same_bits(o_ga, want_ga) and same_bits(o_nga, want_nga)
        assert list(counts) == list(totals) == list(tot)
        got_ga, got_nga = d_ga.download(), d_nga.download()
        assert same_bits(got_ga[:tot[0]], want_ga) and untouched(got_ga[tot[0]:])
        assert same_bits(got_nga[:tot[1]], want_nga) and untouched(got_nga[tot[1]:])
    cc.close()


def test_scene_compactions_against_numpy_on_one_pair_of_handles():
    """slam_ccicp_scene_dev over every size, shrink and grow: the obstacle / ground compaction (two outputs from one pass)
    against the mask of the labels, the filtered cloud (slam_ccicp_scene_cloud_dev) against the bin order of the oracle's
    classification, the concatenated split against numpy -- none of them through a compaction of the device's"""
    L, seg, cc = api.lib(), api.GroundSegmentation(), api.Ccicp()
    base = synth.make_cloud3d(2, n_loop=50)[0]
    rs = np.random.RandomState(11)
    nmax = max(E.COMPACT_SIZES)
    assert len(base) >= nmax
    d_xyz, d_lab = api.DeviceArray((nmax, 3), np.float32), api.DeviceArray((nmax,), np.uint8)
    d_pts, d_gnd, d_flt = api.DeviceArray((2 * nmax + 2, 2), np.float64), api.DeviceArray((nmax + 1, 4), np.float32), api.DeviceArray((nmax + 1, 4), np.float32)
    d_scan, d_counts = dev(3, np.int32), dev(4, np.int32)
    for n in E.shrink_and_grow():
        xyz = np.ascontiguousarray(base[rs.permutation(len(base))[:n]])
        put(d_xyz, xyz)
        seg.segment_dev(d_xyz, n, 3, d_lab)
        api.synchronize()
        lab = d_lab.download()[:n]
        obs, gnd = xyz[lab >= api.GSEG_OBSTACLE], xyz[lab == api.GSEG_GROUND]
        pts, ground, flt = d_pts.view(0, (2 * n + 2, 2)), d_gnd.view(0, (n + 1, 4)), d_flt.view(0, (n + 1, 4))
        for b in (pts, ground, flt, d_scan, d_counts):
            refill(b)
        cap = n + 2
        api.check(L.slam_ccicp_scene_dev(cc.h, seg.h, d_xyz.ptr, n, 3, 0, 0, 0.0, 0.0, 75.0, cap, d_pts.ptr, d_scan.ptr, d_gnd.ptr, d_counts.ptr, None))
        api.synchronize()
        want = E.bin_order(obs, O.classify_ga(obs)) if len(obs) else np.zeros((0, 4), np.float32)
        counts, scan = d_counts.download(), d_scan.download()
        assert counts.tolist() == [len(obs), len(gnd), len(want), 0], n
        got = ground.download()
        assert same_bits(got[:len(gnd), :3], gnd) and (got[:len(gnd), 3] == 0).all() and untouched(got[len(gnd):]), n
        api.check(L.slam_ccicp_scene_cloud_dev(cc.h, d_flt.ptr, len(want), None))
        api.synchronize()
        got = flt.download()
        assert same_bits(got[:len(want)], want) and untouched(got[len(want):]), n
        w_ga, w_nga, tot = E.split_reference(want, None)
        assert scan.tolist() == [0, len(want), tot[0]], n
        got = pts.download()
        assert same_bits(got[:len(want)], np.concatenate([w_ga, w_nga])) and untouched(got[len(want):]), n
    seg.close()
    cc.close()


# ------------------------------------------------------------------ the chain with a cap that bites
def scene(L, cc, seg, d_xyz, n, voxel, crop, cap, d_pts, d_scan, d_gnd, d_counts):
    api.check(L.slam_ccicp_scene_dev(cc.h, seg.h, d_xyz.ptr if d_xyz else None, n, 3, voxel, 1 if crop else 0, crop[0] if crop else 0.0,
                                     crop[1] if crop else 0.0, E.CHAIN_CROP_DIST, cap, d_pts.ptr, d_scan.ptr, d_gnd.ptr if d_gnd else None,
                                     d_counts.ptr, None))
    api.synchronize()
    return d_scan.download(), d_counts.download()


@pytest.mark.parametrize("voxel", (1, 0))
@pytest.mark.parametrize("crop", E.CHAIN_CROPS, ids=str)
@pytest.mark.parametrize("cloud", E.CHAIN_CLOUDS)
def test_chain_with_a_cap_that_bites(cloud, voxel, crop):
    """slam_ccicp_scene_dev's concatenated two-output compaction (GA in front of NGA, each cut at cap - 1) against the chain
    built from oracle pieces: d_scan and the choice of points exact, the points within the voxel bounds (exact without the
    voxel filter), d_pts past scan[1] untouched; then slam_ccicp_scene_cloud_dev at capacity counts[2], one less and 0"""
    L, seg, cc = api.lib(), api.GroundSegmentation(), api.Ccicp()
    ref = chain_reference(cloud, voxel, crop)
    xyz, flt, vox = ref["xyz"], ref["flt"], ref["vox"]
    n, n_flt = len(xyz), len(flt)
    d_xyz = api.DeviceArray.from_host(xyz)
    d_scan, d_counts, d_gnd = dev(3, np.int32), dev(4, np.int32), dev((n + 1, 4), np.float32)
    for cap in E.chain_caps(len(ref["ga"])):
        d_pts = dev((2 * (cap - 1) + 8, 2), np.float64)
        for b in (d_scan, d_counts, d_gnd):
            refill(b)
        scan, counts = scene(L, cc, seg, d_xyz, n, voxel, crop, cap, d_pts, d_scan, d_gnd, d_counts)
        ga, nga = ref["ga"][:cap - 1], ref["nga"][:cap - 1]
        rows = np.r_[ga, nga]
        assert counts.tolist() == [ref["n_obs"], len(ref["gnd"]), n_flt, 0], cap
        assert scan.tolist() == [0, len(rows), len(ga)], cap
        got = d_pts.download()
        if voxel:
            assert same_bits(got[:len(rows)], got[:len(rows)].astype(np.float32).astype(np.float64))   # float coordinates widened
            assert centroids_ok(got[:len(rows)], vox, rows, 2, dyadic=False), cap
        else:
            assert same_bits(got[:len(rows)], flt[rows, :2].astype(np.float64)), cap
        assert untouched(got[len(rows):]), cap
        got = d_gnd.download()
        assert same_bits(got[:len(ref["gnd"]), :3], ref["gnd"]) and (got[:len(ref["gnd"]), 3] == 0).all() and untouched(got[len(ref["gnd"]):])
        # the filtered cloud the call left in the handle
        for capacity in (n_flt, n_flt - 1):
            d_c = dev((n_flt + 1, 4), np.float32)
            api.check(L.slam_ccicp_scene_cloud_dev(cc.h, d_c.ptr, capacity, None))
            api.synchronize()
            got = d_c.download()
            assert np.array_equal(got[:capacity, 3], flt[:capacity, 3]) and untouched(got[capacity:]), (cap, capacity)
            if voxel:
                assert centroids_ok(got[:capacity, :3], vox, slice(0, capacity), 3, dyadic=False), (cap, capacity)
            else:
                assert same_bits(got[:capacity], flt[:capacity]), (cap, capacity)
        api.check(L.slam_ccicp_scene_cloud_dev(cc.h, None, 0, None))
    seg.close()
    cc.close()


@pytest.mark.parametrize("voxel", (1, 0))
def test_chain_of_nothing(voxel):
    """n = 0 gives zero counts and d_scan = {0, 0, 0}; a cloud wholly outside the 600 m classification lattice n_flt = 0 and
    no error bit -- on handles that have just run a real cloud, and with a real cloud behind it"""
    L, seg, cc = api.lib(), api.GroundSegmentation(rmax=E.FAR_RMAX), api.Ccicp()
    ref = chain_reference("rings", voxel, None)
    d_real = api.DeviceArray.from_host(ref["xyz"])
    far = E.far_cloud()
    d_far, d_lab = api.DeviceArray.from_host(far), api.DeviceArray((len(far),), np.uint8)
    seg.segment_dev(d_far, len(far), 3, d_lab)
    api.synchronize()
    lab = d_lab.download()
    d_pts, d_scan, d_counts, d_gnd = dev((64, 2), np.float64), dev(3, np.int32), dev(4, np.int32), dev((len(far) + 1, 4), np.float32)
    big = api.DeviceArray((2 * len(ref["xyz"]), 2), np.float64)
    for what in ("real", "empty", "far", "real", "far", "empty"):
        for b in (d_pts, d_scan, d_counts, d_gnd):
            refill(b)
        if what == "real":
            scan, counts = scene(L, cc, seg, d_real, len(ref["xyz"]), voxel, None, len(ref["xyz"]), big, d_scan, None, d_counts)
            assert counts[2] > 0 and counts[3] == 0 and scan[1] == counts[2]
            continue
        if what == "empty":
            scan, counts = scene(L, cc, seg, None, 0, voxel, None, 20, d_pts, d_scan, d_gnd, d_counts)
            assert counts.tolist() == [0, 0, 0, 0]
            assert untouched(d_gnd.download())
        else:
            scan, counts = scene(L, cc, seg, d_far, len(far), voxel, None, 20, d_pts, d_scan, d_gnd, d_counts)
            assert counts.tolist() == [int((lab >= 2).sum()), int((lab == 1).sum()), 0, 0]
        assert scan.tolist() == [0, 0, 0] and untouched(d_pts.download())
    assert (lab >= 2).sum() > 0                                        # obstacle points went in, none came out
    seg.close()
    cc.close()


# ------------------------------------------------------------------ the voxel filter's runs
def voxel_call(L, cc, case, d_out, max_out=None):
    pts, flags = case["pts"], case["flags"]
    d_xyz = api.DeviceArray.from_host(pts)
    d_flag = api.DeviceArray.from_host(flags) if flags is not None else None
    refill(d_out)
    n_out = C.c_int(-1)
    rc = L.slam_ccicp_voxel_downsample_dev(cc.h, d_xyz.ptr, d_flag.ptr if d_flag else None, len(pts), pts.shape[1], case["leaf"][0],
                                           case["leaf"][1], case["leaf"][2], d_out.ptr, d_out.shape[0] - 1 if max_out is None else max_out,
                                           C.byref(n_out), None)
    return rc, n_out.value, d_out.download()


def check_voxels(case, n_out, got):
    ref = E.voxel_exact(case["pts"], case["flags"], case["leaf"])
    m = len(ref["idx"])
    assert n_out == m, case["name"]
    assert np.array_equal(got[:m, 3], ref["flag"]), case["name"]
    assert centroids_ok(got[:m, :3], ref, dyadic=case["dyadic"]), case["name"]
    assert untouched(got[m:]), case["name"]


def test_voxel_filter_cases_on_one_handle():
    """slam_ccicp_voxel_downsample_dev on every case of the table, one handle throughout (the 300 m cloud right in front of
    the 2 m cloud: nothing may leak from one lattice into the next): voxels, order and flags exact, centroids within bound A"""
    L, cc = api.lib(), api.Ccicp()
    cases = E.voxel_cases()
    assert [c["name"] for c in cases][-2:] == ["cloud over 300 m", "cloud over 2 m"]
    d_out = dev((max(len(c["pts"]) for c in cases) + 1, 4), np.float32)
    for case in cases + cases[::-1]:
        rc, n_out, got = voxel_call(L, cc, case, d_out)
        api.check(rc)
        check_voxels(case, n_out, got)
    # one output row too few: an error, the count, the rows there is room for, and nothing behind them
    case = cases[0]
    ref = E.voxel_exact(case["pts"], case["flags"], case["leaf"])
    m = len(ref["idx"])
    rc, n_out, got = voxel_call(L, cc, case, d_out, max_out=m - 1)
    with pytest.raises(api.SlamError):
        api.check(rc)
    assert n_out == m and untouched(got[m - 1:])
    assert np.array_equal(got[:m - 1, 3], ref["flag"][:m - 1]) and centroids_ok(got[:m - 1, :3], ref, slice(0, m - 1))
    rc, n_out, got = voxel_call(L, cc, case, d_out)                    # ... and the handle is as good as before
    api.check(rc)
    check_voxels(case, n_out, got)
    cc.close()


# ------------------------------------------------------------------ GA classification with the extent
def ga_call(L, seg, pts, count, d_flags, d_mm):
    d_xyz, d_n = api.DeviceArray.from_host(pts), i32(count)
    refill(d_flags)
    put(d_mm, np.array([0xffffffff] * 3 + [0] * 3, np.uint32))
    api.check(L.slam_gseg_classify_ga_extent_dev(seg.h, d_xyz.ptr, d_n.ptr, len(pts), pts.shape[1], d_flags.ptr, d_mm.ptr, None))
    api.synchronize()
    return d_flags.download(), d_mm.download()


def check_ga(pts, count, flags, mm, name):
    want = O.classify_ga(pts[:count]) if count else np.zeros(0, np.uint8)
    assert np.array_equal(flags[:count], want) and untouched(flags[count:]), name
    ext = E.extent_words(pts[:count], want) if count else None
    if ext is None:
        assert mm.tolist() == [0xffffffff] * 3 + [0] * 3, name
    else:
        got = np.array([E.unorder_f32(w) for w in mm], np.float32)
        assert np.array_equal(got, ext), name                          # numerically: -0.0 is 0.0


def test_classify_ga_with_extent():
    """slam_gseg_classify_ga_extent_dev: flags equal the oracle's, the extent numpy's minimum and maximum over the finite points
    whose flag is not 255 -- every case on ONE handle, so that each meets the cells the one before marked"""
    L, seg = api.lib(), api.GroundSegmentation()
    cases = list(E.ga_cases())
    d_flags, d_mm = dev(max(len(p) for _, p, _ in cases) + 1, np.uint8), dev(6, np.uint32)
    for name, pts, count in cases + cases[::-1]:
        flags, mm = ga_call(L, seg, pts, count, d_flags, d_mm)
        check_ga(pts, count, flags[:len(pts) + 1], mm, name)
    # two disjoint clouds in turn: the second must not see the first's cells
    a, r = E.ga_disjoint_pair()
    for pts in (a, r, a, r):
        flags, mm = ga_call(L, seg, pts, len(pts), d_flags, d_mm)
        check_ga(pts, len(pts), flags[:len(pts) + 1], mm, "disjoint pair")
    # a capacity of 0 leaves everything as it is
    put(d_mm, np.array([0xffffffff] * 3 + [0] * 3, np.uint32))
    d_n = i32(0)
    api.check(L.slam_gseg_classify_ga_extent_dev(seg.h, None, d_n.ptr, 0, 4, None, d_mm.ptr, None))
    api.synchronize()
    assert d_mm.download().tolist() == [0xffffffff] * 3 + [0] * 3
    seg.close()


# ------------------------------------------------------------------ height
def height_pose(L, cc, ground, count, capacity, R, t, z0, roll, pitch, stride=None):
    """slam_ccicp_height_rpy_pose_dev: (z, neighbours within 3 m)"""
    d_g = api.DeviceArray.from_host(ground) if ground is not None and len(ground) else None
    d_R, d_t, d_out = api.DeviceArray.from_host(np.array(R, np.float64)), api.DeviceArray.from_host(np.array(t, np.float64)), dev(3, np.float64)
    d_n = i32(count)
    api.check(L.slam_ccicp_height_rpy_pose_dev(cc.h, d_g.ptr if d_g else None, d_n.ptr, capacity, stride or (ground.shape[1] if d_g else 3),
                                               d_R.ptr, d_t.ptr, z0, roll, pitch, d_out.ptr, None))
    api.synchronize()
    out = d_out.download()
    assert untouched(out[2:])
    return float(out[0]), int(out[1])


EYE, ORIGIN = [1.0, 0.0, 0.0, 1.0], [0.0, 0.0]


def test_height_roll_pitch_and_yaw():
    """roll and pitch in {0, +-0.03, +-0.1} x yaws over (-pi, pi] (pi and pi/2 exactly among them): the device pose of
    slam_ccicp_height_rpy_pose_dev, and the same pose as a quaternion through slam_ccicp_height_dev, against the oracle"""
    L, cc = api.lib(), api.Ccicp()
    ground = E.ground_patch()
    d_g, d_n = api.DeviceArray.from_host(ground), i32(len(ground))
    d_R, d_t, d_out = api.DeviceArray((4,), np.float64), api.DeviceArray((2,), np.float64), dev(2, np.float64)
    for name, R, t, z0, roll, pitch in E.rpy_cases():
        pose = E.pose_of(R, t, z0, roll, pitch)
        zo, nco, idxo = O.ccicp_height(ground, pose)
        put(d_R, np.array(R, np.float64))
        put(d_t, np.array(t, np.float64))
        refill(d_out)
        api.check(L.slam_ccicp_height_rpy_pose_dev(cc.h, d_g.ptr, d_n.ptr, len(ground), 4, d_R.ptr, d_t.ptr, z0, roll, pitch, d_out.ptr, None))
        api.synchronize()
        z, nc = d_out.download()
        assert nc == nco == 4 and abs(z - zo) < 1e-6, name
        z2, nc2, idx2 = C.c_double(0), C.c_int(-1), (C.c_int * 4)()
        api.check(L.slam_ccicp_height_dev(cc.h, d_g.ptr, len(ground), 4, (C.c_double * 7)(*pose), C.byref(z2), C.byref(nc2), idx2, None))
        assert (nc2.value, list(idx2)) == (nco, idxo) and abs(z2.value - zo) < 1e-6, name
    cc.close()


def test_height_sizes_indices_ties_and_counts():
    L, cc = api.lib(), api.Ccicp()

    def host(g, pose=E.IDENTITY):
        d_g = api.DeviceArray.from_host(g)
        z, nc, idx = C.c_double(0), C.c_int(-1), (C.c_int * 4)()
        api.check(L.slam_ccicp_height_dev(cc.h, d_g.ptr, len(g), g.shape[1], (C.c_double * 7)(*pose), C.byref(z), C.byref(nc), idx, None))
        return z.value, nc.value, list(idx)

    # ground sizes around the neighbour search's block (256), the nearest point first, last and either side of the block's edge
    for n, k in E.index_cases():
        g = E.indexed_ground(n, k)
        zo, nco, idxo = O.ccicp_height(g, E.IDENTITY)
        z, nc, idx = host(g)
        assert (nc, idx) == (nco, idxo) and idx[0] == k and abs(z - zo) < 1e-6, (n, k)
        z, nc = height_pose(L, cc, g, n, n, EYE, ORIGIN, 0.0, 0.0, 0.0)
        assert nc == nco and abs(z - zo) < 1e-6, (n, k)
    # duplicated nearest points: the lowest index wins
    g = E.indexed_ground(1025, 256)
    for dup in (700, 255, 0):
        g[dup] = g[256]
        zo, nco, idxo = O.ccicp_height(g, E.IDENTITY)
        z, nc, idx = host(g)
        assert idx[0] == min(dup, 256) == idxo[0] and (nc, idx) == (nco, idxo) and abs(z - zo) < 1e-6, dup
        z, nc = height_pose(L, cc, g, 1025, 1025, EYE, ORIGIN, 0.0, 0.0, 0.0)
        assert nc == nco and abs(z - zo) < 1e-6, dup
    # NaN ground rows are skipped, wherever they are and whatever they would be near
    g = E.indexed_ground(257, 255)
    zo, nco, idxo = O.ccicp_height(g, E.IDENTITY)
    h = np.insert(g, [0, 0, 100, 256, 257], np.float32([[np.nan, -0.5, -1.6], [-0.5, np.nan, -1.6], [-0.5, -0.5, np.nan], [np.nan] * 3, [0.5, 0.5, np.nan]]), axis=0)
    moved = [i + int((np.array([0, 0, 100, 256, 257]) <= i).sum()) for i in idxo]
    z, nc, idx = host(h)
    assert O.ccicp_height(h, E.IDENTITY) == (zo, nco, moved)
    assert (nc, idx) == (nco, moved) and abs(z - zo) < 1e-6
    z, nc = height_pose(L, cc, h, len(h), len(h), EYE, ORIGIN, 0.0, 0.0, 0.0)
    assert nc == nco and abs(z - zo) < 1e-6
    z, nc, idx = host(np.full((5, 3), np.nan, np.float32), [0, 0, 0.3, 0, 0, 0, 1])
    assert (z, nc, idx) == (0.3, 0, [-1] * 4)
    # the count on the device: below the capacity with nearer decoys behind it, zero, and above the capacity (clamped)
    g = E.indexed_ground(600, 256)
    decoys = np.concatenate([E.UNDER, np.full((4, 1), np.float32(-1.45))], 1)      # the wheel points themselves: distance zero
    both = np.concatenate([g, decoys])
    zo, nco, _ = O.ccicp_height(g, E.IDENTITY)
    zd, ncd, _ = O.ccicp_height(both, E.IDENTITY)
    assert abs(zo - zd) > 1e-3
    z, nc = height_pose(L, cc, both, len(g), len(both), EYE, ORIGIN, 0.0, 0.0, 0.0)
    assert nc == nco == 4 and abs(z - zo) < 1e-6
    z, nc = height_pose(L, cc, both, len(both), len(both), EYE, ORIGIN, 0.0, 0.0, 0.0)
    assert nc == ncd == 4 and abs(z - zd) < 1e-6
    z, nc = height_pose(L, cc, both, 0, len(both), EYE, ORIGIN, 0.375, 0.0, 0.0)
    assert (z, nc) == (0.375, 0)
    z, nc = height_pose(L, cc, both, len(both) + 1000, len(g), EYE, ORIGIN, 0.0, 0.0, 0.0)   # clamps to the capacity: the decoys stay out
    assert nc == nco and abs(z - zo) < 1e-6
    z, nc = height_pose(L, cc, None, 0, 0, EYE, ORIGIN, -0.25, 0.0, 0.0)                     # no cloud at all
    assert (z, nc) == (-0.25, 0)
    z, nc = height_pose(L, cc, None, 7, 0, EYE, ORIGIN, -0.25, 0.0, 0.0)
    assert (z, nc) == (-0.25, 0)
    # calls in a row on one handle: four neighbours, then none -- no packed neighbour of the call before is left
    z, nc = height_pose(L, cc, g, len(g), len(g), EYE, ORIGIN, 0.0, 0.0, 0.0)
    assert nc == 4
    z, nc = height_pose(L, cc, g + np.float32([100, 0, 0]), len(g), len(g), EYE, ORIGIN, 0.125, 0.0, 0.0)
    assert (z, nc) == (0.125, 0)
    z, nc = height_pose(L, cc, g, len(g), len(g), EYE, ORIGIN, 0.0, 0.0, 0.0)
    assert nc == 4 and abs(z - zo) < 1e-6
    cc.close()


def test_height_three_metre_gate_and_degenerate_planes():
    """dd < 9.0f: a ground point exactly 3 m from its wheel point is no neighbour (three of four: z stays), one step nearer it
    is.  Host form with the identity pose, and the device form, whose gate is a line of its own."""
    L, cc = api.lib(), api.Ccicp()
    for z0 in (0.0, 0.25):
        for inward in (False, True):
            g = E.gate_ground(inward, z0)
            pose = [0, 0, z0, 0, 0, 0, 1]
            zo, nco, idxo = O.ccicp_height(g, pose)
            d_g = api.DeviceArray.from_host(g)
            z, nc, idx = C.c_double(7), C.c_int(-1), (C.c_int * 4)()
            api.check(L.slam_ccicp_height_dev(cc.h, d_g.ptr, 4, 3, (C.c_double * 7)(*pose), C.byref(z), C.byref(nc), idx, None))
            assert (nc.value, list(idx)) == (nco, idxo) == (4 if inward else 3, [0, 1, 2, 3]), (z0, inward)
            assert abs(z.value - zo) < 1e-6 and (z.value == z0) == (not inward), (z0, inward)
            zd, ncd = height_pose(L, cc, g, 4, 4, EYE, ORIGIN, z0, 0.0, 0.0)
            assert ncd == nco and abs(zd - zo) < 1e-6 and (zd == z0) == (not inward), (z0, inward)
    # degenerate planes: the device and the oracle run the same Jacobi sweeps and must agree (docs/CCICP_EDGES.md on PCL)
    for name, g in E.degenerate_grounds():
        pose = [0, 0, 0.25, 0, 0, 0, 1]
        zo, nco, idxo = O.ccicp_height(g, pose)
        d_g = api.DeviceArray.from_host(g)
        z, nc, idx = C.c_double(7), C.c_int(-1), (C.c_int * 4)()
        api.check(L.slam_ccicp_height_dev(cc.h, d_g.ptr, len(g), 3, (C.c_double * 7)(*pose), C.byref(z), C.byref(nc), idx, None))
        assert (nc.value, list(idx)) == (nco, idxo) and nco == 4 and abs(z.value - zo) < 1e-6, name
        zd, ncd = height_pose(L, cc, g, len(g), len(g), EYE, ORIGIN, 0.25, 0.0, 0.0)
        assert ncd == 4 and abs(zd - zo) < 1e-6, name
    cc.close()


def test_height_mirror():
    """mirror_bytes of a device block appear in pinned host memory when the stream has drained, bytes past them untouched;
    a source that contains d_out shows the new z; sizes that are no multiple of 8 or above 4096 are refused"""
    L, cc = api.lib(), api.Ccicp()
    g = E.indexed_ground(600, 256)
    zo, nco, _ = O.ccicp_height(g, E.IDENTITY)
    d_g, d_n = api.DeviceArray.from_host(g), i32(len(g))
    d_R, d_t = api.DeviceArray.from_host(np.array(EYE)), api.DeviceArray.from_host(np.array(ORIGIN))
    pattern = (np.arange(4096 + 64, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8)
    pattern[pattern == E.SENTINEL] = 1
    d_src = api.DeviceArray.from_host(pattern)
    d_out = d_src.view(0, (16,)).ptr                                   # d_out = the first two doubles of the mirrored block
    dst = api.PinnedArray((4096 + 64,), np.uint8)
    for nbytes in (0, 8, 4096):
        put(d_src, pattern)
        dst.array[:] = E.SENTINEL
        api.check(L.slam_ccicp_height_rpy_pose_mirror_dev(cc.h, d_g.ptr, d_n.ptr, len(g), 3, d_R.ptr, d_t.ptr, 0.0, 0.0, 0.0, d_out,
                                                          dst.ptr if nbytes else None, d_src.ptr if nbytes else None, nbytes, None))
        api.synchronize()
        src = d_src.download()
        z, nc = src[:16].view(np.float64)
        assert nc == nco == 4 and abs(z - zo) < 1e-6 and same_bits(src[16:], pattern[16:]), nbytes
        assert same_bits(dst.array[:nbytes], src[:nbytes]) and untouched(dst.array[nbytes:]), nbytes   # the new z included
    for nbytes in (12, 4104):
        with pytest.raises(api.SlamError):
            api.check(L.slam_ccicp_height_rpy_pose_mirror_dev(cc.h, d_g.ptr, d_n.ptr, len(g), 3, d_R.ptr, d_t.ptr, 0.0, 0.0, 0.0, d_out,
                                                              dst.ptr, d_src.ptr, nbytes, None))
    api.synchronize()
    assert untouched(dst.array[4096:])
    dst.free()
    cc.close()


# ------------------------------------------------------------------ every entry point on one handle
def test_every_entry_point_interleaved_on_one_handle():
    """the stepwise entry points and the chain, interleaved on ONE slam_ccicp handle, forwards and then backwards, a selection
    over 65 * 1024 + 1 items among them (look-back words of a larger launch in the way of the 8-block cloud's): every output
    buffer, the sentinel rows past the counts included, equals byte for byte what the same call leaves on a fresh handle --
    the handle's device words are every entry point's own, and no call finds what another left"""
    L = api.lib()
    xyz = np.ascontiguousarray(synth.make_cloud3d(**E.CHAIN_RINGS)[0], np.float32)
    n = len(xyz)
    assert n == 8 * E.BLOCK
    # the inputs of the later steps, made once by a pair of handles of their own
    seg0, cc0 = api.GroundSegmentation(), api.Ccicp()
    d_xyz, d_lab = api.DeviceArray.from_host(xyz), api.DeviceArray((n,), np.uint8)
    seg0.segment_dev(d_xyz, n, 3, d_lab)
    d_obs, d_gnd, d_flag, d_flt = dev((n, 4), np.float32), dev((n, 4), np.float32), dev(n, np.uint8), dev((n, 4), np.float32)
    n_obs, n_gnd, n_flt = C.c_int(0), C.c_int(0), C.c_int(0)
    api.check(L.slam_ccicp_select_dev(cc0.h, d_xyz.ptr, n, 3, d_lab.ptr, (1 << 2) | (1 << 3), d_obs.ptr, C.byref(n_obs), None))
    api.check(L.slam_ccicp_select_dev(cc0.h, d_xyz.ptr, n, 3, d_lab.ptr, 1 << 1, d_gnd.ptr, C.byref(n_gnd), None))
    api.check(L.slam_gseg_classify_ga_dev(seg0.h, d_obs.ptr, n_obs.value, 4, d_flag.ptr, None))
    api.check(L.slam_ccicp_voxel_downsample_dev(cc0.h, d_obs.ptr, d_flag.ptr, n_obs.value, 4, 0.5, 0.5, 2.0, d_flt.ptr, n, C.byref(n_flt), None))
    api.synchronize()
    n_obs, n_gnd, n_flt = n_obs.value, n_gnd.value, n_flt.value
    assert n_obs > E.BLOCK and n_gnd > E.BLOCK and n_flt > 60
    seg0.close()
    cc0.close()
    n_big = 65 * E.BLOCK + 1
    d_big = api.DeviceArray.from_host(E.cloud_of(n_big))
    d_big_lab = api.DeviceArray.from_host((2 * (np.arange(n_big) % 3 == 0)).astype(np.uint8))
    cx, cy = E.CHAIN_CROPS[1]
    box = (C.c_float * 4)(-E.CHAIN_CROP_DIST + cx, E.CHAIN_CROP_DIST + cx, -E.CHAIN_CROP_DIST + cy, E.CHAIN_CROP_DIST + cy)
    d_R, d_t, d_ngnd = api.DeviceArray.from_host(np.array(E.rot2(0.4))), api.DeviceArray.from_host(np.array([0.5, -0.25])), i32(n_gnd)
    pattern = (np.arange(64, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8)
    pinned = api.PinnedArray((72,), np.uint8)
    # the outputs, allocated once: a call refills its own with the sentinel
    o_rows, o_big, o_ga, o_nga = dev((n + 1, 4), np.float32), dev((n_big + 1, 4), np.float32), dev((n + 1, 2), np.float64), dev((n + 1, 2), np.float64)
    o_pts, o_scan, o_counts, o_gnd, o_src = dev((2 * n + 2, 2), np.float64), dev(3, np.int32), dev(4, np.int32), dev((n + 1, 4), np.float32), dev(64, np.uint8)

    def left(*bufs):
        api.synchronize()
        return [b.download().tobytes() for b in bufs]

    def voxel(cc, seg):
        refill(o_rows)
        cnt = C.c_int(-1)
        api.check(L.slam_ccicp_voxel_downsample_dev(cc.h, d_obs.ptr, d_flag.ptr, n_obs, 4, 0.5, 0.5, 2.0, o_rows.ptr, n, C.byref(cnt), None))
        return [cnt.value] + left(o_rows)

    def select(cc, seg):
        refill(o_rows)
        cnt = C.c_int(-1)
        api.check(L.slam_ccicp_select_dev(cc.h, d_xyz.ptr, n, 3, d_lab.ptr, (1 << 2) | (1 << 3), o_rows.ptr, C.byref(cnt), None))
        return [cnt.value] + left(o_rows)

    def select_big(cc, seg):
        refill(o_big)
        cnt = C.c_int(-1)
        api.check(L.slam_ccicp_select_dev(cc.h, d_big.ptr, n_big, 3, d_big_lab.ptr, 1 << 2, o_big.ptr, C.byref(cnt), None))
        return [cnt.value] + left(o_big)

    def bin_order(cc, seg):
        refill(o_rows)
        cnt = C.c_int(-1)
        api.check(L.slam_ccicp_bin_order_dev(cc.h, d_obs.ptr, d_flag.ptr, n_obs, 4, o_rows.ptr, C.byref(cnt), None))
        return [cnt.value] + left(o_rows)

    def split(with_box, cap):
        def call(cc, seg):
            refill(o_ga)
            refill(o_nga)
            counts, totals = (C.c_int * 2)(-1, -1), (C.c_int * 2)(-1, -1)
            api.check(L.slam_ccicp_split_box_dev(cc.h, d_flt.ptr, n_flt, 4, box if with_box else None, cap, o_ga.ptr, o_nga.ptr, counts, totals, None))
            return [list(counts), list(totals)] + left(o_ga, o_nga)
        return call

    def height(cc, seg):
        z, nc, idx = C.c_double(7), C.c_int(-1), (C.c_int * 4)()
        pose = E.pose_of(E.rot2(0.4), [0.5, -0.25], 0.125, 0.03, -0.03)
        api.check(L.slam_ccicp_height_dev(cc.h, d_gnd.ptr, n_gnd, 4, (C.c_double * 7)(*pose), C.byref(z), C.byref(nc), idx, None))
        return [z.value, nc.value, list(idx)]

    def scene_call(voxel, crop, cap):
        def call(cc, seg):
            for b in (o_pts, o_scan, o_counts, o_gnd, o_rows):
                refill(b)
            scan, counts = scene(L, cc, seg, d_xyz, n, voxel, crop, cap, o_pts, o_scan, o_gnd, o_counts)
            api.check(L.slam_ccicp_scene_cloud_dev(cc.h, o_rows.ptr, int(counts[2]), None))
            return left(o_pts, o_scan, o_counts, o_gnd, o_rows)
        return call

    def mirror(cc, seg):
        put(o_src, pattern)
        pinned.array[:] = E.SENTINEL
        api.check(L.slam_ccicp_height_rpy_pose_mirror_dev(cc.h, d_gnd.ptr, d_ngnd.ptr, n_gnd, 4, d_R.ptr, d_t.ptr, 0.125, 0.03, -0.03,
                                                          o_src.view(0, (16,)).ptr, pinned.ptr, o_src.ptr, 64, None))
        return left(o_src) + [pinned.array.tobytes()]

    calls = [("voxel_downsample", voxel), ("select over %d" % n_big, select_big), ("select", select), ("bin_order", bin_order),
             ("split_box with a box", split(True, 50)), ("height", height), ("scene, voxel filter", scene_call(1, E.CHAIN_CROPS[1], 50)),
             ("split_box without a box", split(False, n + 2)), ("height_rpy_pose_mirror", mirror), ("scene, bin order", scene_call(0, None, n))]
    fresh = {}
    for name, call in calls:
        seg, cc = api.GroundSegmentation(), api.Ccicp()
        fresh[name] = call(cc, seg)
        seg.close()
        cc.close()
    assert fresh["select"][0] == n_obs and fresh["voxel_downsample"][0] == n_flt and fresh["height"][1] == 4
    assert fresh["split_box with a box"][0] != fresh["split_box with a box"][1]              # the cap bites
    assert np.frombuffer(fresh["height_rpy_pose_mirror"][0][:16], np.float64)[1] == 4
    seg, cc = api.GroundSegmentation(), api.Ccicp()
    for order in (calls, calls[::-1]):
        for name, call in order:
            assert call(cc, seg) == fresh[name], name
    pinned.free()
    seg.close()
    cc.close()


# ------------------------------------------------------------------ packing
@pytest.mark.parametrize("case", list(E.pack_cases()), ids=lambda c: c[0])
def test_pack_scans(case):
    """slam_ccicp_pack_scans_dev against np.concatenate, the cumulative scan_off[n + 1] and scan_nga"""
    L = api.lib()
    name, scenes = case
    rs = np.random.RandomState(len(scenes))
    n = len(scenes)
    pts = [rs.randn(s + 3, 2) for s, _ in scenes]                      # (rows behind a scene's size are not the scene's)
    d_pts = [api.DeviceArray.from_host(p) for p in pts]
    d_scan = [i32(0, s, g) for s, g in scenes]
    total = sum(s for s, _ in scenes)
    d_out, d_off, d_nga = dev((total + 2, 2), np.float64), dev(n + 2, np.int32), dev(n + 1, np.int32)
    api.check(L.slam_ccicp_pack_scans_dev(n, (C.c_void_p * n)(*[d.ptr for d in d_pts]), (C.c_void_p * n)(*[d.ptr for d in d_scan]), d_out.ptr,
                                          d_off.ptr, d_nga.ptr, None))
    api.synchronize()
    out, off, nga = d_out.download(), d_off.download(), d_nga.download()
    assert off[:n + 1].tolist() == np.r_[0, np.cumsum([s for s, _ in scenes])].tolist() and untouched(off[n + 1:])
    assert nga[:n].tolist() == [g for _, g in scenes] and untouched(nga[n:])
    assert same_bits(out[:total], np.concatenate([p[:s] for p, (s, _) in zip(pts, scenes)])) and untouched(out[total:])


def test_pack_scans_refuses_bad_arguments():
    L = api.lib()
    d_p, d_s = api.DeviceArray.from_host(np.zeros((4, 2))), i32(0, 4, 0)
    d_out, d_off, d_nga = dev((200, 2), np.float64), dev(40, np.int32), dev(40, np.int32)
    for n, ptrs, scans in ((0, [d_p.ptr], [d_s.ptr]), (33, [d_p.ptr] * 33, [d_s.ptr] * 33), (2, [d_p.ptr, None], [d_s.ptr] * 2),
                           (2, [d_p.ptr] * 2, [None, d_s.ptr])):
        with pytest.raises(api.SlamError):
            api.check(L.slam_ccicp_pack_scans_dev(n, (C.c_void_p * len(ptrs))(*ptrs), (C.c_void_p * len(scans))(*scans), d_out.ptr, d_off.ptr,
                                                  d_nga.ptr, None))
    api.synchronize()
    assert untouched(d_out.download()) and untouched(d_off.download()) and untouched(d_nga.download())


# ------------------------------------------------------------------ the grid's in-order update from device clouds
@pytest.mark.parametrize("stride", (3, 4))
def test_grid_add_scan_inorder_dev(stride):
    """slam_grid_add_scan_inorder_dev equals the host form and the oracle's in-order update, scan after scan, an empty
    obstacle cloud and an empty ground cloud among them"""
    L = api.lib()
    rs = np.random.RandomState(90 + stride)
    g_dev, g_host = (api.Grid(64, 64, 0.25, min_cluster_points=3, rolling=1) for _ in range(2))
    p = g_dev.params
    gp = O.grid_params(64, 64, 0.25, p.max_range, p.occupancy_increment, p.occupancy_decrement, p.min_cluster_points, p.rolling, *g_dev.get_pose())
    num, drv, occ = np.zeros(64 * 64), np.full(64 * 64, -1, np.int8), np.full(64 * 64, -1, np.int8)
    for n_obs, n_gnd in ((300, 500), (0, 400), (257, 0), (1, 1), (600, 900), (0, 0)):
        obs = (rs.randn(n_obs, stride) * 2.5).astype(np.float32)
        gnd = (rs.randn(n_gnd, stride) * 5.0).astype(np.float32)
        d_obs = api.DeviceArray.from_host(obs) if n_obs else None
        d_gnd = api.DeviceArray.from_host(gnd) if n_gnd else None
        api.check(L.slam_grid_add_scan_inorder_dev(g_dev.h, d_obs.ptr if d_obs else None, n_obs, d_gnd.ptr if d_gnd else None, n_gnd, stride, None))
        api.synchronize()
        api.check(L.slam_grid_add_scan_inorder(g_host.h, api._ptr(obs), n_obs, api._ptr(gnd), n_gnd, stride))
        if n_obs + n_gnd:
            O.grid_add_scan_inorder(gp, obs.reshape(-1, stride), gnd.reshape(-1, stride), num, drv, occ)
        assert np.array_equal(g_dev.read_occupancy(), occ) and np.array_equal(g_host.read_occupancy(), occ), (n_obs, n_gnd)
        assert np.array_equal(g_dev.read_num_pts(), num) and np.array_equal(g_host.read_num_pts(), num), (n_obs, n_gnd)   # bit-exact doubles
    assert (occ == 100).sum() > 0 and (occ == 0).sum() > 0
    g_dev.close()
    g_host.close()
