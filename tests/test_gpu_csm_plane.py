"""The correlative matcher over a byte plane and the pose-set scorer on the device (slam_csm_create_from_plane*,
slam_csm_set_plane_dev, slam_csm_score_poses*; docs/GRID_MATCH.md) against the numpy restatement of tests/csm_plane_cases.py:
tables, answers, posterior and scores equal it, no tolerance.  The angle pairs the restatement is fed are the ones
slam_csm_angles returned, so libm is not in question."""
import ctypes as C
import types

import numpy as np
import pytest

import csm_cases as K
import csm_oracle as CO
import csm_plane_cases as P
import csm_post_oracle as PO
from slam_amd import api

gpu = pytest.mark.gpu


def R_of(theta):
    return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])


def matcher_for(c, **kw):
    args = dict(resolution=c["res"], block=c["D"], half_x=c["half_x"], half_y=c["half_y"], half_theta=c["half_theta"], theta_step=c["theta_step"])
    args.update(kw)
    return api.CorrelativeMatcher.from_plane(c["plane"], c["ox"], c["oy"], **args)


def restated(c, cm, plane=None, ox=None, oy=None):
    """(R0, the device's angle pairs, vol, counted) of a case, optionally over another plane / origin"""
    R0 = R_of(c["theta0"])
    cs = cm.angles(R0)
    tab = (c["ox"] if ox is None else ox, c["oy"] if oy is None else oy, c["plane"] if plane is None else plane)
    vol, cnt = P.volume_slices(tab, c["pts"], cs, c["t0"], c["res"], c["half_x"], c["half_y"])
    return R0, cs, vol, cnt


def held(c, cm, vol, cnt, cs, R0, n_ga=None):
    """both search forms give the restatement's answer: indices, score, counts, R and t to the bit"""
    n_ga = c["n_ga"] if n_ga is None else n_ga
    wR, wt, want = P.match(vol, cnt, len(c["pts"]), cs, c["t0"], c["res"], c["half_x"], c["half_y"], R0)
    out = []
    for ex in (0, 1):
        cm.set_exhaustive(ex)
        R, t, r = cm.match(c["pts"][:n_ga], c["pts"][n_ga:], R0, c["t0"])
        got = dict(zip(("k", "a", "b", "score", "n_points", "max_score"), CO.result_tuple(r)))
        assert got == want, (c["name"], ex, got, want)
        assert R.tobytes() == wR.tobytes() and t.tobytes() == wt.tobytes(), (c["name"], ex, t, wt)
        out.append(got)
    return out[0]


# ------------------------------------------------------------------------------------------------------------------ tables
@gpu
@pytest.mark.parametrize("D", (1, 8, 16))
@pytest.mark.parametrize("i", range(len(P.PLANE_SIZES)))
def test_tables_equal_the_restatement(i, D):
    (w, h), (ox, oy) = P.PLANE_SIZES[i], P.ORIGINS[i]
    plane = P.random_plane(w, h, 40 + i)
    T, W = P.tables(plane, D)
    d_plane = api.DeviceArray.from_host(plane)
    for cm in (api.CorrelativeMatcher.from_plane(plane, ox, oy, resolution=P.RES, block=D),
               api.CorrelativeMatcher.from_plane(d_plane, ox, oy, resolution=P.RES, block=D)):
        for cls in (0, 1):                                                      # one table, read by both classes
            gx, gy, got = cm.table(cls, 0)
            assert (gx, gy) == (ox, oy) and got.shape == T.shape and np.array_equal(got, T)
            gx, gy, got = cm.table(cls, 1)
            assert (gx, gy) == (ox - (D - 1), oy - (D - 1)) and got.shape == W.shape and np.array_equal(got, W)
        info = cm.info()
        assert info["table_bytes"] == T.size + W.size                           # counted once
        assert info["params"].sigma == 0.0 and info["params"].kernel_cells == 0  # the plane carries the kernel
        cm.close()


# ------------------------------------------------------------------------------------------------------------------- match
@gpu
@pytest.mark.parametrize("name", [c["name"] for c in P.cases() if c["name"] != "four_points"])
def test_match_equals_the_restatement(name):
    c = P.case(name)
    cm = matcher_for(c)
    R0, cs, vol, cnt = restated(c, cm)
    got = held(c, cm, vol, cnt, cs, R0)
    if name.endswith("_outside"):
        assert (got["score"], got["k"], got["b"], got["a"]) == (0, 0, 0, 0) and got["n_points"] == len(c["pts"])
    if name == "tie":
        assert (got["k"], got["b"], got["a"]) == (0, 0, 0) and got["score"] == 9 * 50
    # the device's score volume, every entry
    assert np.array_equal(cm.score_volume(c["pts"][:c["n_ga"]], c["pts"][c["n_ga"]:], R0, c["t0"]), vol)
    cm.close()


@gpu
def test_four_points_keep_the_pose():
    c = P.case("four_points")
    cm = matcher_for(c)
    R0 = R_of(c["theta0"])
    with pytest.raises(api.SlamError) as e:
        cm.match(c["pts"][:2], c["pts"][2:], R0, c["t0"])
    assert e.value.code == api.E_TOO_FEW_SCENE
    batch = types.SimpleNamespace(n_scans=1, pts=c["pts"], scan_off=np.array([0, 4], np.int32), scan_nga=np.array([2], np.int32),
                                  R=R0.reshape(1, 4), t=c["t0"].reshape(1, 2))
    for ex in (0, 1):
        cm.set_exhaustive(ex)
        R, t, res = cm.match_batch(batch)
        assert int(res[0]["score"]) == -1 and R.tobytes() == R0.tobytes() and t.tobytes() == c["t0"].tobytes()
    cm.close()


@gpu
def test_the_class_split_makes_no_difference():
    c = P.case("97x83_half")
    cm = matcher_for(c)
    R0, cs, vol, cnt = restated(c, cm)
    seen = [held(c, cm, vol, cnt, cs, R0, n_ga=n_ga) for n_ga in P.N_GA_SPLITS]
    assert seen[0] == seen[1] == seen[2]
    cm.close()


# --------------------------------------------------------------------------------------------------------------- posterior
@gpu
@pytest.mark.parametrize("name", ("97x83_inside", "wide_D16"))
def test_posterior_equals_the_restatement(name):
    c = P.case(name)
    cm = matcher_for(c)
    cm.set_post_params()
    pp = cm.post_params
    R0, cs, vol, cnt = restated(c, cm)
    U = P.bounds((c["ox"], c["oy"], c["plane"]), c["D"], c["pts"], cs, c["t0"], c["res"], c["half_x"], c["half_y"])
    for ex in (0, 1):
        cm.set_exhaustive(ex)
        want = PO.posterior(vol, cnt, len(c["pts"]), cm.post_table(), c["res"], c["theta_step"], margin_per_point=pp.margin_per_point,
                            excl_xy=pp.excl_xy, excl_theta=pp.excl_theta, bounds=U, exhaustive=bool(ex))
        R, t, res, post = cm.match_post(c["pts"][:c["n_ga"]], c["pts"][c["n_ga"]:], R0, c["t0"])
        assert bytes(post) == PO.pack(want), (name, ex, [(f, getattr(post, f), want[f]) for f in PO.INT_FIELDS], post.m0, want["m0"])
        assert want["n_within"] >= 1
    cm.close()


# ----------------------------------------------------------------------------------------------------------- set_plane_dev
@gpu
def test_set_plane_dev_refreshes_tables_and_answers():
    c = P.case("97x83_inside")
    h, w = c["plane"].shape
    cm = matcher_for(c)
    st = api.Stream()
    sparse = np.zeros_like(c["plane"])
    sparse[::9, ::7] = c["plane"][::9, ::7]
    sparse[40, 50] = 255
    steps = [(P.random_plane(w, h, 77, density=0.9), c["ox"], c["oy"]), (sparse, c["ox"], c["oy"]), (np.zeros_like(sparse), c["ox"], c["oy"]),
             (c["plane"], c["ox"] + 3, c["oy"] - 2), (c["plane"], c["ox"], c["oy"])]
    for plane, ox, oy in steps:
        d_plane = api.DeviceArray.from_host(plane)
        cm.set_plane_dev(d_plane, ox, oy, stream=st)
        st.synchronize()
        T, W = P.tables(plane, c["D"])
        for cls in (0, 1):
            assert cm.table(cls, 0)[:2] == (ox, oy) and np.array_equal(cm.table(cls, 0)[2], T)
            assert cm.table(cls, 1)[:2] == (ox - c["D"] + 1, oy - c["D"] + 1) and np.array_equal(cm.table(cls, 1)[2], W)
        R0, cs, vol, cnt = restated(c, cm, plane, ox, oy)
        got = held(c, cm, vol, cnt, cs, R0)
        if not plane.any():
            assert (got["score"], got["k"], got["b"], got["a"]) == (0, 0, 0, 0)
    # refused: another size (the adapter holds a DeviceArray to the handle's), a handle made from a model, an origin off the lattice
    with pytest.raises(api.SlamError) as e:
        cm.set_plane_dev(api.DeviceArray((h, w + 1), np.uint8), 0, 0)
    assert e.value.code == api.E_INVALID
    with pytest.raises(api.SlamError) as e:
        cm.set_plane_dev(api.DeviceArray.from_host(c["plane"]), (1 << 30) - 8, 0)
    assert e.value.code == api.E_INVALID and "slam_csm_set_plane_dev" in str(e.value)
    assert cm.table(0, 0)[:2] == (c["ox"], c["oy"])                             # a refused call changes nothing
    box = K.box_model()
    model = api.CorrelativeMatcher(box[0], box[1])
    with pytest.raises(api.SlamError) as e:
        model.set_plane_dev(api.DeviceArray.from_host(c["plane"]), 0, 0)
    assert e.value.code == api.E_INVALID and "slam_csm_set_plane_dev" in str(e.value) and "model" in str(e.value)
    model.close()
    cm.close()


# --------------------------------------------------------------------------------------------------------------- refusals
@gpu
@pytest.mark.parametrize("dev", (False, True))
def test_every_refusal_of_the_create_calls(dev):
    fn = "slam_csm_create_from_plane_dev" if dev else "slam_csm_create_from_plane"
    d_plane = api.DeviceArray((128,), np.uint8)
    host = np.zeros(128, np.uint8)
    L = api.lib()
    for w, h, ox, oy, kw, word in P.BAD_PLANES:
        p = CO.default_params(**kw)
        out = C.c_void_p(0x5A5A)
        rc = getattr(L, fn)(d_plane.ptr if dev else host.ctypes.data_as(C.c_void_p), w, h, ox, oy, C.byref(p), C.byref(out))
        msg = L.slam_last_error().decode()
        assert rc == api.E_INVALID and (fn + ":") in msg and word in msg and not out.value, (w, h, ox, oy, kw, msg)
    with pytest.raises(api.SlamError) as e:
        api.CorrelativeMatcher.from_plane(np.zeros((0, 5), np.uint8), 0, 0)
    assert e.value.code == api.E_INVALID and "slam_csm_create_from_plane" in str(e.value)


# ------------------------------------------------------------------------------------------------------------ score_poses
@pytest.fixture(scope="module")
def big():
    c = P.case("chunk_1025")
    cm = matcher_for(c)
    yield c, cm, (c["ox"], c["oy"], c["plane"])
    cm.close()


@gpu
@pytest.mark.parametrize("n", P.POINT_COUNTS)
@pytest.mark.parametrize("n_poses", P.POSE_COUNTS)
def test_score_poses_equals_the_restatement(big, n_poses, n):
    c, cm, tab = big
    pts, n_ga = c["pts"][:n], min(c["n_ga"], n)
    poses = P.pose_set(n_poses, 1000 + n_poses)
    want_s, want_n = P.score_poses((tab, tab), pts, n_ga, poses, c["res"])
    s, k = cm.score_poses(pts[:n_ga], pts[n_ga:], poses)
    assert np.array_equal(s, want_s) and np.array_equal(k, want_n), (n_poses, n)
    if n_poses > 2:
        assert s[1] == 0 and k[1] == 0 and s[2] == 0 and k[2] == 0             # a NaN and an infinite pose: 0, 0
        finite = np.isfinite(poses).all(axis=1)
        assert (k[finite] == n).all()                                           # a point outside the table is counted ...
        if n >= 1023 and n_poses >= 63:
            assert (s[finite] == 0).any() and (s[finite] > 0).any()             # ... and scores 0: some poses put the whole scan outside
    # the device form on a stream, outputs poisoned first
    st = api.Stream()
    d_pts, d_poses = api.DeviceArray.from_host(pts.reshape(-1, 2)), api.DeviceArray.from_host(poses)
    d_s, d_k = api.DeviceArray.from_host(np.full(n_poses, -7, np.int32)), api.DeviceArray.from_host(np.full(n_poses, -7, np.int32))
    cm.score_poses_dev(d_pts, n, n_ga, d_poses, n_poses, d_s, d_k, stream=st)
    st.synchronize()
    assert np.array_equal(d_s.download(), want_s) and np.array_equal(d_k.download(), want_n)


@gpu
def test_score_poses_edges(big):
    c, cm, tab = big
    # no pose: a successful no-op, whatever else it is handed
    assert api.lib().slam_csm_score_poses_dev(cm.h, None, 5, 0, None, 0, None, None, None) == api.SLAM_OK
    s, k = cm.score_poses(c["pts"][:3], c["pts"][3:5], np.zeros((0, 4)))
    assert len(s) == 0 and len(k) == 0
    # the class split makes no difference on a plane-built handle
    poses = P.pose_set(65, 5)
    a = cm.score_poses(c["pts"][:0], c["pts"], poses)
    b = cm.score_poses(c["pts"], c["pts"][:0], poses)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
    # too many points: refused
    one = api.DeviceArray((4,), np.float64)
    out = api.DeviceArray((1,), np.int32)
    rc = api.lib().slam_csm_score_poses_dev(cm.h, one.ptr, (1 << 23) + 1, 0, one.ptr, 1, out.ptr, out.ptr, None)
    assert rc == api.E_INVALID and "slam_csm_score_poses_dev" in api.lib().slam_last_error().decode()


@gpu
@pytest.mark.parametrize("n_ga_model", (400, 3))
def test_score_poses_on_a_model_built_handle(n_ga_model):
    """scored against read_table's tables; a class of 3 model points has no table and its scan points are not counted"""
    m_ga, m_nga = K.model_points(n_ga_model, 11), K.model_points(500, 12)
    cm = api.CorrelativeMatcher(m_ga, m_nga)
    tabs = []
    for cls in (0, 1):
        ox, oy, T = cm.table(cls, 0)
        tabs.append((ox, oy, T) if T.size else None)
    assert (tabs[0] is None) == (n_ga_model == 3) and tabs[1] is not None
    rs = np.random.RandomState(3)
    ox, oy, T = tabs[1]
    pts = np.stack([(ox + rs.rand(1100) * T.shape[1]) * 0.1, (oy + rs.rand(1100) * T.shape[0]) * 0.1], axis=1)
    th = rs.uniform(-0.2, 0.2, 130)
    poses = np.stack([np.cos(th), np.sin(th), rs.uniform(-1, 1, 130), rs.uniform(-1, 1, 130)], axis=1)
    poses[7, 0] = np.nan
    want_s, want_n = P.score_poses(tabs, pts, 300, poses, cm.params.resolution)
    s, k = cm.score_poses(pts[:300], pts[300:], poses)
    assert np.array_equal(s, want_s) and np.array_equal(k, want_n) and s.any()
    assert k[0] == (800 if n_ga_model == 3 else 1100) and k[7] == 0
    cm.close()


@gpu
def test_a_pose_on_the_lattice_equals_the_score_volume(big):
    """two kernels against each other: resolution 0.125, dyadic coordinates, the four exact rotations -- the pose of candidate
    (k, b, a) is (c_k, s_k, t0 + ((a - half_x) res, (b - half_y) res)), every sum exact"""
    c, cm, tab = big
    cm.set_window(7, 6, 1, 0.01)
    pts = np.round(c["pts"][:600] * 64) / 64
    t0 = np.array([0.25, -0.5])
    for cs in (np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]), np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0]])):
        d_pts, d_t0, d_cs = api.DeviceArray.from_host(pts), api.DeviceArray.from_host(t0), api.DeviceArray.from_host(cs)
        d_vol = api.DeviceArray((3, 13, 15), np.int32)
        api.check(api.lib().slam_csm_score_volume_dev(cm.h, d_pts.ptr, len(pts), 200, d_t0.ptr, d_cs.ptr, d_vol.ptr, None))
        api.synchronize()
        vol = d_vol.download()
        k, b, a = np.indices(vol.shape)
        poses = np.stack([cs[k.ravel(), 0], cs[k.ravel(), 1], t0[0] + (a.ravel() - 7) * P.RES, t0[1] + (b.ravel() - 6) * P.RES], axis=1)
        s, n = cm.score_poses(pts[:200], pts[200:], poses)
        assert np.array_equal(s, vol.ravel()) and (n == len(pts)).all() and vol.any()
        want = P.volume_slices(tab, pts, cs, t0, P.RES, 7, 6)[0]
        assert np.array_equal(vol, want)
    cm.set_window(c["half_x"], c["half_y"], c["half_theta"], c["theta_step"])
