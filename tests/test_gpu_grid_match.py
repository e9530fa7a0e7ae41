"""Grid -> distance field -> matcher, end to end on the device (slam_amd.api.GridMatcher, docs/GRID_MATCH.md): the matcher's table
is the restatement made from the grid's read-back occupancy (tests/grid_dist_cases.two_pass and cost_of with a likelihood
table), every answer equals the numpy restatement of tests/csm_plane_cases.py worked on that plane, no tolerance, and lies within
one cell per axis and one angular step of the truth."""
import numpy as np
import pytest

import csm_oracle as CO
import csm_plane_cases as P
from slam_amd import api, synth

gpu = pytest.mark.gpu
WARM_OFFSET = (0.73, -0.58, 0.153)
KS = (CO.BASIN_KS[0], CO.BASIN_KS[3])


def mapped_grid(size, res, centre=None):
    """a rolling grid fed make_map()'s points as obstacles (no ground cloud), finalized; centre: set_pose first"""
    m_ga, m_nga = CO.synth_map()
    g = api.Grid(size, size, res, min_cluster_points=0)
    if centre is not None:
        g.set_pose(*centre)
    c = np.asarray(g.get_pose(), np.float64)
    obs = (np.concatenate([m_ga, m_nga]) - c).astype(np.float32)                # the window's frame is centred on the grid's pose
    g.add_endpoints(obs, np.zeros((0, 2), np.float32))
    g.finalize()
    return g


def plane_of(g, sigma, R):
    """the restatement of the matcher's table from the occupancy the grid reads back"""
    occ = g.read_occupancy()
    assert (occ == 100).sum() > 100 and set(np.unique(occ)) <= {-1, 0, 100}
    return P.likelihood_plane(occ, g.size_x, g.size_y, g.resolution, sigma, R)


def restated_match(gm, plane, t_ga, t_nga, R0, t0_map):
    """the restatement's answer, worked in the window's frame with the centre added back"""
    m = gm.matcher
    p = m.params
    centre = np.asarray(gm.centre, np.float64)
    pts = np.concatenate([t_ga, t_nga])
    cs = m.angles(R0)
    t0 = np.asarray(t0_map, np.float64) - centre
    tab = (-(gm.grid.size_x // 2), -(gm.grid.size_y // 2), plane)
    vol, cnt = P.volume_slices(tab, pts, cs, t0, p.resolution, p.half_x, p.half_y)
    R, t, want = P.match(vol, cnt, len(pts), cs, t0, p.resolution, p.half_x, p.half_y, R0)
    return R, t + centre, want


def same_answer(got, want):
    R, t, res = got
    wR, wt, w = want
    r = dict(zip(("k", "a", "b", "score", "n_points", "max_score"), CO.result_tuple(res)))
    assert r == w, (r, w)
    assert np.asarray(R).tobytes() == wR.tobytes() and np.asarray(t).tobytes() == wt.tobytes(), (t, wt)


def table_is(gm, plane):
    for cls in (0, 1):
        ox, oy, T = gm.matcher.table(cls, 0)
        assert (ox, oy) == (-(gm.grid.size_x // 2), -(gm.grid.size_y // 2)) and np.array_equal(T, plane)


@pytest.fixture(scope="module")
def warm():
    g = mapped_grid(500, 0.1)
    gm = api.GridMatcher(g, 0.2, half_x=10, half_y=10, half_theta=20, theta_step=0.01)
    st = api.Stream()
    gm.update(stream=st)
    st.synchronize()
    yield g, gm, plane_of(g, 0.2, 6)
    gm.close()


@pytest.fixture(scope="module")
def cold():
    g = mapped_grid(128, 0.5)
    gm = api.GridMatcher(g, 0.5)
    st = api.Stream()
    gm.update(stream=st)
    st.synchronize()
    yield g, gm, plane_of(g, 0.5, 3)
    gm.close()


# -------------------------------------------------------------------------------------------------------------- warm start
@gpu
def test_warm_table_is_the_restatement(warm):
    g, gm, plane = warm
    assert gm.max_cells == 6 and np.array_equal(gm.table, P.likelihood_table_np(0.1, 0.2, 6)[0])
    assert gm.matcher.params.resolution == 0.1 and gm.centre == (0.0, 0.0)
    table_is(gm, plane)
    assert plane.max() == 255 and (plane == 0).any()


@gpu
@pytest.mark.parametrize("k", KS)
def test_warm_start_equals_the_restatement_and_finds_the_truth(warm, k):
    g, gm, plane = warm
    t_ga, t_nga, pose = synth.make_scan(k, 256)
    R0, t0 = synth.pose_to_Rt(pose[0] + WARM_OFFSET[0], pose[1] + WARM_OFFSET[1], pose[2] + WARM_OFFSET[2])
    want = restated_match(gm, plane, t_ga, t_nga, R0, t0)
    for ex in (0, 1):
        gm.matcher.set_exhaustive(ex)
        got = gm.match(t_ga, t_nga, R0, t0)
        same_answer(got, want)
    R, t, res = got
    theta = pose[2] + WARM_OFFSET[2] + (res.k - 20) * 0.01
    print("warm k=%d: %.3f m %.3f m %.4f rad, score %d of %d" % (k, abs(t[0] - pose[0]), abs(t[1] - pose[1]), abs(theta - pose[2]), res.score,
                                                                  res.max_score))
    assert abs(t[0] - pose[0]) <= 0.1 and abs(t[1] - pose[1]) <= 0.1 and abs(theta - pose[2]) <= 0.01


@gpu
def test_warm_posterior_batch_and_scores(warm):
    """match_post and match_batch give match's answer; score_poses at the answer gives its score"""
    g, gm, plane = warm
    gm.matcher.set_exhaustive(0)
    gm.matcher.set_post_params()
    t_ga, t_nga, pose = synth.make_scan(KS[0], 256)
    R0, t0 = synth.pose_to_Rt(pose[0] + WARM_OFFSET[0], pose[1] + WARM_OFFSET[1], pose[2] + WARM_OFFSET[2])
    R, t, res = gm.match(t_ga, t_nga, R0, t0)
    Rp, tp, resp, post = gm.match_post(t_ga, t_nga, R0, t0)
    assert Rp.tobytes() == R.tobytes() and tp.tobytes() == t.tobytes() and resp.score == res.score and post.valid == 1
    batch = synth.make_batch(2, 256, first=KS[0])
    t_start = batch.true_poses[:, :2] + np.array(WARM_OFFSET[:2])
    R_start = np.stack([synth.pose_to_Rt(p[0], p[1], p[2] + WARM_OFFSET[2])[0].reshape(4) for p in batch.true_poses])
    Rb, tb, resb = gm.match_batch(batch, R_start, t_start)
    assert Rb[0].tobytes() == R.tobytes() and tb[0].tobytes() == t.tobytes() and int(resb[0]["score"]) == res.score
    poses = np.array([[R[0, 0], R[1, 0], t[0], t[1]], [R[0, 0], R[1, 0], np.nan, t[1]]])
    s, n = gm.score_poses(t_ga, t_nga, poses)
    tab = (-250, -250, plane)
    ws, wn = P.score_poses((tab, tab), np.concatenate([t_ga, t_nga]), len(t_ga), poses, 0.1)     # (the centre is 0, 0)
    assert np.array_equal(s, ws) and np.array_equal(n, wn) and n.tolist() == [res.n_points, 0] and s[1] == 0
    # (not held to res.score: the scorer forms the cell of R p + t, the search the cell of R p + t0 shifted by whole cells, and at
    # 0.1 m the two may round a point on a cell's edge to either side; tests/test_gpu_csm_plane.py holds them equal at 0.125 m)


# -------------------------------------------------------------------------------------------------------------- cold start
@gpu
@pytest.mark.parametrize("k", KS)
def test_cold_start_relocalizes_from_no_prior(cold, k):
    g, gm, plane = cold
    assert gm.max_cells == 3
    table_is(gm, plane)
    t_ga, t_nga, pose = synth.make_scan(k, 256)
    R, t, res = gm.relocalize(t_ga, t_nga, 0.05)
    p = gm.matcher.params
    assert (p.half_x, p.half_y, p.half_theta, p.theta_step) == (64, 64, 63, 0.05)   # the whole grid, all angles
    same_answer((R, t, res), restated_match(gm, plane, t_ga, t_nga, np.eye(2), (0.0, 0.0)))
    theta = (res.k - 63) * 0.05
    dth = abs((theta - pose[2] + np.pi) % (2 * np.pi) - np.pi)
    print("cold k=%d: %.3f m %.3f m %.4f rad, score %d of %d" % (k, abs(t[0] - pose[0]), abs(t[1] - pose[1]), dth, res.score, res.max_score))
    assert abs(t[0] - pose[0]) <= 0.5 and abs(t[1] - pose[1]) <= 0.5 and dth <= 0.05


# ------------------------------------------------------------------------------------------------------------ rolling grid
@gpu
def test_rolling_grid_works_in_the_windows_frame():
    res = 0.5
    g = mapped_grid(128, res, centre=(7 * res + 0.2, -5 * res - 0.1))           # (+7, -5) cells and a sub-cell remainder, which is dropped
    assert g.window_cell() == (7, -5) and g.get_pose() == (7 * res, -5 * res)
    gm = api.GridMatcher(g, 0.5, half_x=6, half_y=6, half_theta=4, theta_step=0.05)
    st = api.Stream()
    gm.update(stream=st)
    st.synchronize()
    assert gm.centre == (3.5, -2.5)
    plane = plane_of(g, 0.5, 3)
    table_is(gm, plane)
    # the same room seven cells further left in the window: the plane is the fixed grid's, shifted
    fixed = plane_of(mapped_grid(128, res), 0.5, 3)
    assert np.array_equal(plane[10:100, 10:100], fixed[5:95, 17:107])
    t_ga, t_nga, pose = synth.make_scan(KS[1], 256)
    R0, t0 = synth.pose_to_Rt(pose[0] + 1.3, pose[1] - 0.9, pose[2] + 0.08)
    want = restated_match(gm, plane, t_ga, t_nga, R0, t0)
    got = gm.match(t_ga, t_nga, R0, t0)
    same_answer(got, want)
    R, t, r = got
    assert abs(t[0] - pose[0]) <= res and abs(t[1] - pose[1]) <= res            # in the map frame: the centre was added back
    # the C-ABI stays in the window's frame
    Rw, tw, rw = gm.matcher.match(t_ga, t_nga, R0, t0 - np.array(gm.centre))
    assert (rw.k, rw.a, rw.b, rw.score) == (r.k, r.a, r.b, r.score) and (tw + np.array(gm.centre)).tobytes() == t.tobytes()
    gm.close()


# ------------------------------------------------------------------------------------------- cross-check against the old path
@gpu
@pytest.mark.parametrize("Kc,sigma", ((6, 0.2), (3, 0.12)))
def test_model_built_table_is_the_likelihood_plane_of_one_obstacle(Kc, sigma):
    """four model points in one cell: T of a model-built matcher with kernel K is, inside its (2K + 1)^2 square, the likelihood
    plane of a single obstacle at R = ceil(K sqrt 2)"""
    res = 0.1
    model = np.array([[0.31, -0.27], [0.32, -0.21], [0.39, -0.29], [0.35, -0.25]])   # cell (3, -3)
    cm = api.CorrelativeMatcher(model, np.zeros((0, 2)), resolution=res, sigma=sigma, kernel_cells=Kc)
    ox, oy, T = cm.table(0, 0)
    S = 2 * Kc + 1
    assert (ox, oy) == (3 - Kc, -3 - Kc) and T.shape == (S, S)
    R = int(np.ceil(Kc * np.sqrt(2.0)))
    table = api.likelihood_table(res, sigma, R)
    df = api.DistanceField(S, S, max_cells=R, unknown_keep_from=0)
    df.set_table(table)
    occ = np.full(S * S, -1, np.int8)
    occ[Kc + S * Kc] = 100
    df.compute(occ)
    cost = df.read()[1].reshape(S, S)
    assert np.array_equal(T, cost) and T[Kc, Kc] == 255
    j, i = np.indices((S, S)) - Kc
    assert np.array_equal(T, table[i * i + j * j])
    # ... and a plane-built handle over that plane answers as the model-built one does
    cp = api.CorrelativeMatcher.from_plane(cost, ox, oy, resolution=res, half_x=5, half_y=5, half_theta=3, theta_step=0.02)
    cm.set_window(5, 5, 3, 0.02)
    rs = np.random.RandomState(1)
    scan = model[rs.randint(0, 4, 40)] + rs.uniform(-0.3, 0.3, (40, 2))
    a = cm.match(scan, np.zeros((0, 2)), np.eye(2), np.array([0.2, -0.1]))
    b = cp.match(scan[:11], scan[11:], np.eye(2), np.array([0.2, -0.1]))
    assert CO.result_tuple(a[2]) == CO.result_tuple(b[2]) and a[1].tobytes() == b[1].tobytes() and a[2].score > 0
    cm.close(), cp.close(), df.close()


# ------------------------------------------------------------------------- nothing is allocated, nothing waits: a captured graph
@gpu
def test_update_match_and_scores_replay_in_a_graph(cold):
    g, gm, plane = cold
    m = gm.matcher
    m.set_window(8, 8, 6, 0.05)
    m.set_exhaustive(0)
    batch = synth.make_batch(2, 256, first=KS[1])
    S = batch.n_scans
    m.reserve(S)
    R0 = np.stack([synth.pose_to_Rt(p[0], p[1], p[2] + 0.11)[0].reshape(4) for p in batch.true_poses])
    t0 = batch.true_poses[:, :2] + np.array([1.2, -0.8])
    ga, nga = batch.scan(0)
    pts0 = np.concatenate([ga, nga])
    poses = api.CorrelativeMatcher.poses(batch.true_poses[0, 2] + np.linspace(-0.2, 0.2, 70), np.full(70, batch.true_poses[0, 0]),
                                         np.full(70, batch.true_poses[0, 1]))
    d_pts, d_off, d_nga = api.DeviceArray.from_host(batch.pts), api.DeviceArray.from_host(batch.scan_off), api.DeviceArray.from_host(batch.scan_nga)
    d_R0, d_t0 = api.DeviceArray.from_host(R0), api.DeviceArray.from_host(t0)
    d_cs = api.DeviceArray.from_host(np.stack([m.angles(R0[s]) for s in range(S)]))
    d_R, d_t, d_res = api.DeviceArray((S, 4), np.float64), api.DeviceArray((S, 2), np.float64), api.DeviceArray((S,), api.CSM_RESULT_DTYPE)
    d_pts0, d_poses = api.DeviceArray.from_host(pts0), api.DeviceArray.from_host(poses)
    d_s, d_n = api.DeviceArray((70,), np.int32), api.DeviceArray((70,), np.int32)
    st = api.Stream()
    before = m.info()
    with api.Graph(st) as graph:
        gm.update(stream=st)
        m.match_batch_dev(d_pts, d_off, d_nga, S, d_R0, d_t0, d_cs, d_R, d_t, d_res, stream=st)
        m.score_poses_dev(d_pts0, len(pts0), len(ga), d_poses, 70, d_s, d_n, stream=st)
    after = m.info()
    assert (before["table_bytes"], before["scratch_bytes"]) == (after["table_bytes"], after["scratch_bytes"])
    runs = []
    for _ in range(2):
        for d in (d_R, d_t, d_res, d_s, d_n):
            d.zero(st)
        graph.launch()
        st.synchronize()
        runs.append([d.download().tobytes() for d in (d_R, d_t, d_res, d_s, d_n)])
    assert runs[0] == runs[1]
    table_is(gm, plane)
    tab = (-64, -64, plane)
    for s in range(S):
        a, b = batch.scan(s)
        want = restated_match(gm, plane, a, b, R0[s].reshape(2, 2), t0[s])
        got = d_res.download()[s]
        assert {f: int(got[f]) for f in ("k", "a", "b", "score", "n_points", "max_score")} == want[2]
        assert d_t.download()[s].tobytes() == want[1].tobytes()
    ws, wn = P.score_poses((tab, tab), pts0, len(ga), poses, 0.5)
    assert np.array_equal(d_s.download(), ws) and np.array_equal(d_n.download(), wn) and ws.max() > 0
