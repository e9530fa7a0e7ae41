"""slam_kf_* (slam_amd/csrc/kf_edge.hip) against the scalar restatement tests/cpp/kf_edge_oracle.cpp: the keyframe store
(filter, gated search), the ICP of graph_slam's calcEdgeIcp with and without its stop rules, computeEdgeInformationLUM,
batch independence and determinism, the degenerate edges and the argument errors.  Bounds: docs/KF_EDGE.md section 6."""
import ctypes as C
import signal

import numpy as np
import pytest

import kf_edge_oracle as K
from slam_amd import api

POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_icp.py
CHAIN_TOL = 1e-9                # reassociated f64 sums and nothing else (tests/test_gpu_icp.py:86)
MARGIN_TOL = 1e-9
TEST_SECONDS = 300


@pytest.fixture(autouse=True)
def time_limit():
    """Every test here ends after TEST_SECONDS, and the session with it: nothing more is started on the GPU."""
    def expired(signum, frame):
        pytest.exit("GPU test exceeded %d s" % TEST_SECONDS, returncode=3)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


class Scene:
    """The six make_cloud3d keyframes in a store, and their restatement twins built from the store's filtered clouds."""

    def __init__(self, **kw):
        self.store = api.KeyframeStore(**kw)
        self.poses, self.ora, self.filtered = [], [], []
        for k in K.EDGE_KS:
            xyz, pose = K.cloud(k)
            kid = self.store.add_keyframe(xyz)
            assert kid == len(self.poses)
            f = self.store.read_keyframe(kid)
            self.poses.append(pose)
            self.filtered.append(f)
            self.ora.append(K.OracleKeyframe(f[:, :3], self.store.params))

    def init(self, to, perturb=K.PERTURB):
        return K.relative_init(self.poses[0], self.poses[to], perturb)

    def oracle_edge(self, frm, to, init, params=None, **kw):
        tgt = self.ora[frm]
        return K.register_edge(tgt, self.filtered[to][:, :3], init, params=params or self.store.params, **kw)


@pytest.fixture(scope="module")
def scene():
    return Scene()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_result(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("transform", "transform64", "information")) and \
        all(a[k] == b[k] for k in ("iterations", "state", "converged", "pairs", "num_corr", "singular")) and \
        np.array_equal(bits(np.float64(a["mse"])), bits(np.float64(b["mse"]))) and \
        np.array_equal(bits(np.float32(a["ss"])), bits(np.float32(b["ss"])))


@pytest.mark.gpu
def test_store_filter_equals_the_voxel_filter_called_directly(scene):
    cc = api.Ccicp()
    for i, k in enumerate(K.EDGE_KS):
        xyz, _ = K.cloud(k)
        direct = cc.voxel_downsample(xyz, leaf=(0.5, 0.5, 0.5))
        got = scene.filtered[i]
        assert got.shape == direct.shape and np.array_equal(got.view(np.uint32), direct.view(np.uint32)), k
        info = scene.store.info(i)
        cells, max_cell = scene.ora[i].stats()
        print("keyframe %d: %d points, %d cells, largest %d, %d slots, %d bytes" %
              (k, info["n_points"], info["n_cells"], info["max_cell_points"], info["table_slots"], info["device_bytes"]))
        assert (info["n_points"], info["n_cells"], info["max_cell_points"]) == (len(direct), cells, max_cell)
        # O(filtered points): two float4 copies and a table of at most 4 n slots of 16 bytes
        assert info["device_bytes"] <= 96 * info["n_points"] + 1024


brute_force = K.brute_force


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_gated_search_equals_brute_force(scene, strict):
    rs = np.random.RandomState(11)
    f = scene.filtered[0]
    # half the queries near points of the cloud (inside and around the gate), half anywhere in its box
    near = f[rs.randint(0, len(f), 50000), :3] + rs.normal(0, 0.5, (50000, 3)).astype(np.float32)
    lo, hi = f[:, :3].min(axis=0) - 2, f[:, :3].max(axis=0) + 2
    q = np.concatenate([near, rs.uniform(lo, hi, (50000, 3))]).astype(np.float32)
    q[:16] = f[:16, :3]                    # exact hits
    gi, gd = scene.store.nearest(0, q, strict=strict)
    bi, bd = brute_force(f, q, scene.store.params.gate, strict)
    print("kept %d of %d queries" % ((bi >= 0).sum(), len(q)))
    assert (bi >= 0).sum() > 20000
    assert np.array_equal(gi, bi)
    assert np.array_equal(gd.view(np.uint32), bd.view(np.uint32))
    oi, od = scene.ora[0].nearest(q, strict=strict)
    assert np.array_equal(oi, bi) and np.array_equal(od.view(np.uint32), bd.view(np.uint32))


FIXED = (1, 2, 5, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("to", [1, 2, 3, 4, 5])
def test_fixed_iterations_follow_the_restatement(scene, to):
    """Stop rules off (negative epsilons): pairs of every iteration equal, total transform within 1e-9; where the f32
    transforms are bit-equal, the information matrix to its reassociation bounds."""
    init = scene.init(to)
    lum_checked = 0
    for iters in FIXED:
        scene.store.set_params(max_iterations=iters, transformation_epsilon=-1.0, fitness_epsilon=-1.0)
        dev = scene.store.register_edges([(0, to, init)], trace=32)[0]
        ora = scene.oracle_edge(0, to, init, trace=32, lum_detail=True)
        print("edge 0-%d, %d iterations: pairs %s  |dT| %.3g" % (K.EDGE_KS[to], iters, dev["pairs_trace"][:iters].tolist(),
                                                              np.abs(dev["transform64"] - ora["transform64"]).max()))
        assert (dev["iterations"], dev["state"], dev["converged"]) == (ora["iterations"], ora["state"], ora["converged"]) == \
            (iters, api.KF_ITERATIONS, 1)
        assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"])
        assert dev["pairs"] == ora["pairs"]
        assert np.abs(dev["transform64"] - ora["transform64"]).max() < CHAIN_TOL
        assert abs(dev["mse"] - ora["mse"]) <= 1e-12 * max(1.0, ora["mse"])
        if np.array_equal(bits(dev["transform"]), bits(ora["transform"])):
            check_information(dev, ora)
            lum_checked += 1
    scene.store.set_params(max_iterations=200, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
    assert lum_checked >= 1, "no fixed-iteration case gave bit-equal f32 transforms"


def mm_terms(aver, diff):
    """|term| sums of graphSlamTools.cpp:153-176 per MM entry (f64), for the reassociation bound n 2^-53 sum|term|"""
    a = aver.astype(np.float64)
    s = np.zeros((6, 6))
    s[0, 4] = np.abs(a[:, 1]).sum()
    s[0, 5] = s[1, 3] = np.abs(a[:, 2]).sum()
    s[1, 4] = s[2, 5] = np.abs(a[:, 0]).sum()
    s[2, 3] = s[0, 4]
    s[3, 4] = np.abs((aver[:, 0] * aver[:, 2]).astype(np.float64)).sum()
    s[3, 5] = np.abs((aver[:, 0] * aver[:, 1]).astype(np.float64)).sum()
    s[4, 5] = np.abs((aver[:, 1] * aver[:, 2]).astype(np.float64)).sum()
    s[3, 3] = (aver[:, 1] * aver[:, 1] + aver[:, 2] * aver[:, 2]).astype(np.float64).sum()
    s[4, 4] = (aver[:, 0] * aver[:, 0] + aver[:, 1] * aver[:, 1]).astype(np.float64).sum()
    s[5, 5] = (aver[:, 0] * aver[:, 0] + aver[:, 2] * aver[:, 2]).astype(np.float64).sum()
    return np.maximum(s, s.T)


def check_information(dev, ora):
    """numCorr equal; MM (info * ss) to n 2^-53 sum|term|; ss to n 2^-24 relative; info to the two together."""
    n = ora["num_corr"]
    assert dev["num_corr"] == n and dev["singular"] == ora["singular"] == 0
    ss_d, ss_o = float(dev["ss"]), float(ora["ss"])
    ss_bound = n * 2.0 ** -24
    print("    LUM: n %d  ss %.9g vs %.9g (rel %.3g, bound %.3g)" % (n, ss_d, ss_o, abs(ss_d - ss_o) / ss_o, ss_bound))
    assert abs(ss_d - ss_o) <= ss_bound * ss_o
    # MM as the device summed it: info = MM * (double)(1.0f / ss), an exact-to-rounding product that is divided out again
    w_d = float(np.float32(1.0) / np.float32(dev["ss"]))
    mm_dev = dev["information"] / w_d
    terms = mm_terms(ora["aver"], ora["diff"])
    mm_bound = n * 2.0 ** -53 * terms + 4 * 2.0 ** -53 * np.abs(ora["MM"])   # + the rounding of * w and / w
    err = np.abs(mm_dev - ora["MM"])
    print("    LUM: max |dMM| / bound %.3g" % (err / np.maximum(mm_bound, 1e-300)).max())
    assert (err <= mm_bound).all()
    # the weight (double)(1.0f / ss): ss's bound, and the f32 roundings of ss and of the division
    info_bound = (ss_bound / (1 - ss_bound) + 2.0 ** -22) * np.abs(ora["information"]) + mm_bound / ss_o
    assert (np.abs(dev["information"] - ora["information"]) <= info_bound).all()


@pytest.mark.gpu
def test_setup_gicp_settings_follow_the_restatement(scene):
    """The five edges with setup_gicp's values: pose within 1e-4 m / 1e-5 rad, iterations and stop state equal; an edge may
    differ in iterations only where the restatement decided a stop test by less than 1e-9, and at most one may."""
    excused = 0
    inits = [scene.init(to) for to in range(1, 6)]
    devs = scene.store.register_edges([(0, to, inits[to - 1]) for to in range(1, 6)], trace=256)
    for to in range(1, 6):
        dev, init = devs[to - 1], inits[to - 1]
        ora = scene.oracle_edge(0, to, init, trace=256, lum_detail=True)
        dpos, dang = K.pose_error(dev["transform64"], ora["transform64"])
        tpos, tang = K.pose_error(ora["transform64"], K.true_relative(scene.poses[0], scene.poses[to]))
        print("edge 0-%d: %d / %d iterations, state %d / %d, pairs %d / %d, margin %.3g, device - restatement %.3g m %.3g rad, "
              "restatement - truth %.3g m %.3g rad" % (K.EDGE_KS[to], dev["iterations"], ora["iterations"], dev["state"], ora["state"],
                                                      dev["pairs"], ora["pairs"], ora["margin"], dpos, dang, tpos, tang))
        assert tpos < 0.05 and tang < 0.01
        assert dpos < POS_TOL and dang < ANG_TOL
        if (dev["iterations"], dev["state"]) != (ora["iterations"], ora["state"]):
            assert ora["margin"] < MARGIN_TOL
            excused += 1
            continue
        assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"])
        assert dev["converged"] == 1 and dev["num_corr"] == ora["num_corr"]
        if np.array_equal(bits(dev["transform"]), bits(ora["transform"])):
            check_information(dev, ora)
    assert excused <= 1


@pytest.mark.gpu
def test_batch_independence_and_determinism(scene):
    """Four edges that share a source (graph_slam's shape), alone and together, twice: the same bits."""
    src = 5
    edges = [(frm, src, K.relative_init(scene.poses[frm], scene.poses[src])) for frm in (0, 1, 2, 4)]
    together = [scene.store.register_edges(edges) for _ in range(2)]
    alone = [[scene.store.register_edges([e])[0] for e in edges] for _ in range(2)]
    for e in range(4):
        print("edge %d-%d: %d iterations, state %d, pairs %d" % (edges[e][0], src, together[0][e]["iterations"],
                                                                 together[0][e]["state"], together[0][e]["pairs"]))
        assert together[0][e]["iterations"] > 0
        for other in (together[1][e], alone[0][e], alone[1][e]):
            assert same_result(together[0][e], other)


@pytest.mark.gpu
def test_target_in_lds_or_through_l2_is_the_same_result(scene):
    """Staging the target's points in LDS is a question of time only.  Every target here fits (4 298-5 931 points, room for
    6 144); a batch that mixes targets that fit with one that does not, and both sides of the boundary, is in
    tests/test_gpu_kf_edge_branches.py."""
    edges = [(frm, 5, K.relative_init(scene.poses[frm], scene.poses[5])) for frm in (0, 1, 2, 4)]
    staged = scene.store.register_edges(edges)
    scene.store.set_params(target_in_lds=0)
    direct = scene.store.register_edges(edges)
    scene.store.set_params(target_in_lds=1)
    for a, b in zip(staged, direct):
        assert a["iterations"] > 0 and same_result(a, b)


@pytest.mark.gpu
def test_edge_to_itself_is_the_identity(scene):
    r = scene.store.register_edges([(0, 0, np.eye(4))])[0]
    assert np.abs(r["transform64"] - np.eye(4)).max() < 1e-12
    assert r["pairs"] == r["num_corr"] == len(scene.filtered[0]) and r["mse"] == 0.0
    assert float(r["ss"]) < 1e-13 and r["singular"] == 1 and np.array_equal(r["information"], np.eye(6))
    o = scene.oracle_edge(0, 0, np.eye(4))
    assert (o["iterations"], o["state"], o["singular"]) == (r["iterations"], r["state"], 1)


@pytest.mark.gpu
def test_disjoint_clouds_have_no_correspondences(scene):
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = (1000.0, -500.0, 250.0)
    r = scene.store.register_edges([(0, 1, init)])[0]
    assert (r["state"], r["converged"], r["iterations"], r["pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 0)
    assert np.array_equal(r["transform"], init) and np.array_equal(r["transform64"], init.astype(np.float64))
    assert r["num_corr"] == 0 and r["singular"] == 1 and np.array_equal(r["information"], np.eye(6))
    o = scene.oracle_edge(0, 1, init)
    assert (o["state"], o["converged"], o["iterations"], o["singular"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 1)


@pytest.mark.gpu
def test_bad_arguments_are_error_codes(scene):
    L, h = api.lib(), scene.store.h
    req = (api.KfEdgeReq * 1)()
    res = (api.KfEdgeResult * 1)()
    req[0].from_, req[0].to = 0, len(K.EDGE_KS)
    assert L.slam_kf_register_edges(h, req, 1, res, None) == api.E_INVALID
    assert b"names keyframes" in L.slam_last_error()
    req[0].from_, req[0].to = -1, 0
    assert L.slam_kf_register_edges(h, req, 1, res, None) == api.E_INVALID
    req[0].from_ = 0
    assert L.slam_kf_register_edges(h, None, 1, res, None) == api.E_INVALID
    assert L.slam_kf_register_edges(h, req, 1, None, None) == api.E_INVALID
    assert L.slam_kf_register_edges(None, req, 1, res, None) == api.E_INVALID
    assert L.slam_kf_register_edges(h, req, 0, res, None) == api.SLAM_OK
    kid = C.c_int()
    assert L.slam_kf_add_keyframe(h, None, 10, 3, C.byref(kid)) == api.E_INVALID
    assert L.slam_kf_add_keyframe(h, C.addressof(req), 10, 2, C.byref(kid)) == api.E_INVALID
    assert L.slam_kf_keyframe_info(h, 99, None, None, None, None, None) == api.E_INVALID
    assert L.slam_kf_nearest_dev(h, 99, None, 0, 3, 0, None, None, None) == api.E_INVALID
    with pytest.raises(api.SlamError):   # the lattice is fixed once a keyframe is in
        scene.store.set_params(gate=1.0)
    scene.store.params.gate = 0.75
    assert len(scene.store) == len(K.EDGE_KS)


@pytest.mark.gpu
def test_ten_times_the_points(scene):
    """A keyframe ten times as dense (leaf 0.1 m): nothing in the store or the launch is sized for 5 000 points."""
    st = api.KeyframeStore(leaf_size=0.1, max_iterations=3, transformation_epsilon=-1.0, fitness_epsilon=-1.0)
    ora = []
    for k in (0, 1):
        kid = st.add_keyframe(K.cloud(k)[0])
        ora.append(K.OracleKeyframe(st.read_keyframe(kid)[:, :3], st.params))
        print("keyframe %d: %s" % (k, st.info(kid)))
    assert st.info(0)["n_points"] > 45000
    init = K.relative_init(K.cloud(0)[1], K.cloud(1)[1])
    dev = st.register_edges([(0, 1, init)], trace=8)[0]
    o = K.register_edge(ora[0], ora[1].xyz, init, params=st.params, trace=8)
    assert np.array_equal(dev["pairs_trace"], o["pairs_trace"]) and dev["num_corr"] == o["num_corr"]
    assert np.abs(dev["transform64"] - o["transform64"]).max() < CHAIN_TOL
