"""The correlative scan matcher on the device (slam_csm_*, slam_amd/csrc/csm.hip) against its scalar restatement
(tests/cpp/csm_oracle.cpp): tables, score volumes and answers bit for bit; batches; the basin scans end to end into
slam_icp_fit_batch_from_dev; handle lifetime.  Shapes are the smallest that reach every edge (tests/csm_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import csm_cases as K
import csm_oracle as CO
import oracle_lib as O
from slam_amd import api, synth

gpu = pytest.mark.gpu


def same_table(dev, ora):
    return dev[0] == ora[0] and dev[1] == ora[1] and dev[2].shape == ora[2].shape and np.array_equal(dev[2], ora[2])


# ------------------------------------------------------------------ what the cases reach (no GPU)
def test_cases_reach_the_edges():
    box = K.box_model()
    om = CO.OracleMatcher(box[0], box[1])
    ox = om.table(1)[0]
    residues, seen = set(), {}
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
        seen[name] = (vol, cnt, len(ga) + len(nga))
        # the first column of T a lookup reads for the scan's first NGA point at the middle angle
        cs = om.angles(R0)[ht]
        qx = (cs[0] * nga[0, 0] - cs[1] * nga[0, 1]) + t0[0]
        residues.add((int(np.floor(qx / K.RES)) - ox - win[0]) % 4)
    assert residues == {0, 1, 2, 3}
    assert seen["all_outside"][0].max() == 0 and seen["all_outside"][1].min() == 200
    vol, cnt, n = seen["half_outside"]
    assert 0.2 * 255 * n < vol.max() < 0.7 * 255 * n      # about half the scan still finds the tables
    assert seen["nonfinite"][1].max() == 64 - 3
    vol = seen["winner_in_ragged_block"][0]
    assert np.unravel_index(int(np.argmax(vol)), vol.shape) == (0, 16, 16)
    # other block sizes: a lane of the block kernels holds candidate r * 64 + lane of its block in register r
    regs = {D: set() for D in K.BLOCK_SIZES}
    for name, D, ga, nga, R0, t0, win, ht in K.block_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        vol = om.volume(ga, nga, R0, t0)
        k, b, a = np.unravel_index(int(np.argmax(vol)), vol.shape)
        regs[D].add(((b % D) * D + a % D) // 64)
        if name == "winner_in_fourth_register":
            assert (a, b) == (10, 13) and (D != 16 or (b % D) * D + a % D == 218)
    assert regs[2] == {0} and 1 in regs[11] and {2, 3} <= regs[16], regs


# ------------------------------------------------------------------ tables
TABLE_CASES = [(5, 300, 1, 2), (2000, 3, 6, 8), (300, 0, 6, 2), (0, 2000, 1, 8), (5, 5, 6, 8), (300, 2000, 6, 8)]


@gpu
@pytest.mark.parametrize("n_ga,n_nga,Kc,D", TABLE_CASES)
def test_tables_equal_the_restatement(n_ga, n_nga, Kc, D):
    m_ga, m_nga = K.model_points(n_ga, 11), K.model_points(n_nga, 12) + (0.0 if n_nga != 5 else 1.3)
    kw = dict(kernel_cells=Kc, block=D, sigma=0.2 if Kc == 6 else 0.05)
    om = CO.OracleMatcher(m_ga, m_nga, **kw)
    cm = api.CorrelativeMatcher(m_ga, m_nga, **kw)
    d_ga, d_nga = api.DeviceArray.from_host(m_ga), api.DeviceArray.from_host(m_nga)
    cd = api.CorrelativeMatcher.from_device(d_ga, n_ga, d_nga, n_nga, **kw)
    for cls, n in ((0, n_ga), (1, n_nga)):
        for level in (0, 1):
            want = om.table(cls, level)
            assert (want[2].size == 0) == (n <= 3)
            assert same_table(cm.table(cls, level), want), (cls, level)
            assert same_table(cd.table(cls, level), want), (cls, level)
    cm.close()
    cd.close()


# ------------------------------------------------------------------ score volumes and answers
@pytest.fixture(scope="module")
def box():
    m = K.box_model()
    return m, CO.OracleMatcher(m[0], m[1]), api.CorrelativeMatcher(m[0], m[1])


def answers(cm, om, ga, nga, R0, t0):
    """the device's pruned and exhaustive answers and the restatement's two: all four must be one"""
    out = []
    for ex in (0, 1):
        cm.set_exhaustive(ex)
        R, t, r = cm.match(ga, nga, R0, t0)
        out.append((CO.result_tuple(r), R.tobytes(), t.tobytes(), r.blocks_evaluated))
        Ro, to, ro = om.match(ga, nga, R0, t0, exhaustive=bool(ex))
        out.append((CO.result_tuple(ro), Ro.tobytes(), to.tobytes(), ro.blocks_evaluated))
    cm.set_exhaustive(0)
    return out


@gpu
def test_volumes_and_answers_equal_the_restatement(box):
    _, om, cm = box
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        cm.set_window(win[0], win[1], ht, 0.01)
        assert np.array_equal(cm.angles(R0), om.angles(R0)), name
        want = om.volume(ga, nga, R0, t0)
        got = cm.score_volume(ga, nga, R0, t0)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int(np.abs(got - want).max()))
        a = answers(cm, om, ga, nga, R0, t0)
        assert all(x[:3] == a[0][:3] for x in a), (name, [x[0] for x in a])
        assert a[0][3] == a[1][3] and a[2][3] == a[3][3], name     # the same blocks survive on both sides (a diagnostic)
        if name == "all_outside":
            assert a[0][0][:4] == (0, 0, 0, 0)


@gpu
def test_blocks_of_other_sizes():
    m = K.box_model()
    made = {}
    for name, D, ga, nga, R0, t0, win, ht in K.block_cases():
        if D not in made:
            made[D] = (CO.OracleMatcher(m[0], m[1], block=D), api.CorrelativeMatcher(m[0], m[1], block=D))
        om, cm = made[D]
        om.set_window(win[0], win[1], ht, 0.01)
        cm.set_window(win[0], win[1], ht, 0.01)
        assert np.array_equal(cm.score_volume(ga, nga, R0, t0), om.volume(ga, nga, R0, t0)), (name, D)
        a = answers(cm, om, ga, nga, R0, t0)
        assert all(x[:3] == a[0][:3] for x in a), (name, D, [x[0] for x in a])
        assert a[0][3] == a[1][3] and a[2][3] == a[3][3], (name, D)
    for _, cm in made.values():
        cm.close()


@gpu
def test_second_class_without_a_table():
    m_ga, m_nga = K.centre([0, 1, 2], [0, 0, 0]), K.box_model()[1]
    om, cm = CO.OracleMatcher(m_ga, m_nga), api.CorrelativeMatcher(m_ga, m_nga)
    assert cm.table(0)[2].size == 0
    for n in (5, 65):
        ga, nga = K.scan_of((K.box_model()[0], m_nga), n, K.TRUE_POSE, 500 + n, ga_share=0.4)
        R0, t0 = K.pose_Rt(K.TRUE_POSE[0] + 0.3, K.TRUE_POSE[1], K.TRUE_POSE[2] - 0.02)
        for c, o in ((cm, om), ):
            c.set_window(8, 8, 4, 0.01)
            o.set_window(8, 8, 4, 0.01)
        assert np.array_equal(cm.score_volume(ga, nga, R0, t0), om.volume(ga, nga, R0, t0))
        a = answers(cm, om, ga, nga, R0, t0)
        assert all(x[:3] == a[0][:3] for x in a) and a[0][0][4] == len(nga)
    cm.close()


@gpu
def test_exact_tie_on_the_device():
    kw, m_ga, m_nga, ga, nga, R0, t0, winner, other, score = K.tie_case()
    om, cm = CO.OracleMatcher(m_ga, m_nga, **kw), api.CorrelativeMatcher(m_ga, m_nga, **kw)
    vol = cm.score_volume(ga, nga, R0, t0)
    assert np.array_equal(vol, om.volume(ga, nga, R0, t0))
    assert vol[winner[0], winner[2], winner[1]] == score == vol[other[0], other[2], other[1]] == vol.max()
    a = answers(cm, om, ga, nga, R0, t0)
    assert all(x[:3] == a[0][:3] for x in a), [x[0] for x in a]
    assert a[0][0][:4] == (*winner, score)
    cm.close()


# ------------------------------------------------------------------ batches
@gpu
@pytest.mark.parametrize("n_scans", [1, 2, 37])
def test_batches(box, n_scans):
    _, om, cm = box
    om.set_window(8, 8, 4, 0.01)
    cm.set_window(8, 8, 4, 0.01)
    pts, off, nga, R0, t0 = K.batch_scans(n_scans)
    batch = synth.ScanBatch(pts, off, nga, R0, t0, None)
    first = None
    for ex in (0, 1, 0):
        cm.set_exhaustive(ex)
        R, t, res = cm.match_batch(batch)
        bits = (R.tobytes(), t.tobytes(), tuple(CO.result_tuple(r) for r in res))
        first = first or bits
        assert bits == first                                  # twice the same bits, and the exhaustive form's
    cm.set_exhaustive(0)
    for s in range(n_scans):
        ga, ng = batch.scan(s)
        Ro, to, ro = om.match(ga, ng, R0[s], t0[s])
        assert CO.result_tuple(res[s]) == CO.result_tuple(ro), s
        assert np.array_equal(R[s], Ro.reshape(4)) and np.array_equal(t[s], to), s
        if len(ga) + len(ng) < 5:
            assert res[s]["score"] == -1 and np.array_equal(R[s], R0[s]) and np.array_equal(t[s], t0[s])
        else:
            # the scan alone: the same bits as in the batch
            Ra, ta, ra = cm.match(ga, ng, R0[s], t0[s])
            assert CO.result_tuple(ra) == CO.result_tuple(res[s]) and np.array_equal(Ra.reshape(4), R[s]) and np.array_equal(ta, t[s])
    if n_scans > 2:
        assert res[n_scans // 2]["score"] == -1
    # in place: the registered poses over the initial ones
    d = [api.DeviceArray.from_host(x) for x in (pts, off, nga, R0, t0, np.stack([cm.angles(r) for r in R0]))]
    d_res = api.DeviceArray((n_scans,), api.CSM_RESULT_DTYPE)
    cm.match_batch_dev(d[0], d[1], d[2], n_scans, d[3], d[4], d[5], d[3], d[4], d_res)
    api.synchronize()
    assert d[3].download().tobytes() == R.tobytes() and d[4].download().tobytes() == t.tobytes()
    # beyond what was reserved: refused, not overrun
    with pytest.raises(api.SlamError) as e:
        cm.match_batch_dev(d[0], d[1], d[2], cm.info()["max_scans"] + 1, d[3], d[4], d[5], d[3], d[4], d_res)
    assert e.value.code == api.E_INVALID


# ------------------------------------------------------------------ end to end
@gpu
def test_basin_scans_into_icp():
    ks = CO.BASIN_KS[::2]
    m_ga, m_nga = CO.synth_map()
    om, cm = CO.OracleMatcher(m_ga, m_nga), api.CorrelativeMatcher(m_ga, m_nga)
    for cls in (0, 1):
        for level in (0, 1):
            assert same_table(cm.table(cls, level), om.table(cls, level))
    cases = [CO.basin_case(k) for k in ks]
    pts = np.concatenate([np.concatenate([c[0], c[1]]) for c in cases])
    off = np.cumsum([0] + [len(c[0]) + len(c[1]) for c in cases]).astype(np.int32)
    nga = np.array([len(c[0]) for c in cases], np.int32)
    R0, t0 = np.array([c[3].reshape(4) for c in cases]), np.array([c[4] for c in cases])
    batch = synth.ScanBatch(np.ascontiguousarray(pts), off, nga, R0, t0, None)
    R, t, res = cm.match_batch(batch)
    for s, (ga, ng, pose, r0, tt0) in enumerate(cases):
        Ro, to, ro = om.match(ga, ng, r0, tt0)
        assert CO.result_tuple(res[s]) == CO.result_tuple(ro) and np.array_equal(R[s], Ro.reshape(4)) and np.array_equal(t[s], to)
        print("scan %d: candidate %s, blocks evaluated %d (restatement %d) of %d" %
              (ks[s], CO.result_tuple(ro)[:4], res[s]["blocks_evaluated"], ro.blocks_evaluated, int(np.prod(om.block_dims))))
        assert res[s]["blocks_evaluated"] == ro.blocks_evaluated
    # ICP from the candidates: the device's fit against the oracle's from the same start
    icp = api.Icp(m_ga, m_nga, max_iter=100)
    d = [api.DeviceArray.from_host(x) for x in (batch.pts, off, nga, R, t)]
    d_R, d_t = api.DeviceArray((len(ks), 4), np.float64), api.DeviceArray((len(ks), 2), np.float64)
    icp.fit_batch_from_dev(d[0], d[1], d[2], len(ks), d[3], d[4], d_R, d_t, 5.0)
    api.synchronize()
    Rf, tf = d_R.download(), d_t.download()
    oicp, P = O.IcpModel(m_ga, m_nga), O.icp_params(max_iter=100, indist=5.0)
    for s, (ga, ng, pose, _, _) in enumerate(cases):
        Rw, tw, _, steps = oicp.fit(ga, ng, R[s], t[s], P)
        err = max(np.abs(Rf[s] - Rw.reshape(4)).max(), np.abs(tf[s] - tw).max())
        e = CO.pose_error(Rf[s], tf[s], pose)
        print("scan %d: device fit - oracle fit %.3g after %d steps; %.2f mm %.3f mrad from the truth" % (ks[s], err, steps, 1e3 * e[0], 1e3 * e[1]))
        assert err < 1e-9
        assert e[0] < 0.01 and e[1] < 1e-3
    icp.close()
    cm.close()


# ------------------------------------------------------------------ lifetime
def free_bytes():
    api.synchronize()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    rt = C.CDLL(paths[0])
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@gpu
def test_create_match_destroy_gives_the_memory_back():
    m = K.box_model()
    ga, nga = K.scan_of(m, 65, K.TRUE_POSE, 1)
    R0, t0 = K.pose_Rt(*K.TRUE_POSE)

    def cycle():
        cm = api.CorrelativeMatcher(m[0], m[1], half_x=8, half_y=8, half_theta=4)
        cm.reserve(3)
        R, t, r = cm.match(ga, nga, R0, t0)
        cm.close()
        return R.tobytes() + t.tobytes() + bytes(r)

    first = cycle()
    for _ in range(2):
        assert cycle() == first
    before = free_bytes()
    for _ in range(40):
        assert cycle() == first
    after = free_bytes()
    print("csm lifetime: free before %d, after 40 cycles %d (drift %d bytes)" % (before, after, before - after))
    assert before - after == 0
