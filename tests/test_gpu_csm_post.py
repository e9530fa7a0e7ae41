"""The posterior of a correlative match on the device (slam_csm_match_post*, slam_amd/csrc/csm.hip) against its restatement
(tests/csm_post_oracle.py over the scalar matcher's volume): the whole slam_csm_posterior byte for byte, in both search
forms; batches; refusals; handle lifetime.  The scans, windows and edges are tests/csm_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import csm_cases as K
import csm_oracle as CO
import csm_post_cases as PC
import csm_post_oracle as PO
from slam_amd import api, synth

gpu = pytest.mark.gpu


def oracle_post(om, ga, nga, R0, t0, wtab, pp, exhaustive=False):
    vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
    P = om.params
    return PO.posterior(vol, cnt, len(ga) + len(nga), wtab, P.resolution, P.theta_step, margin_per_point=pp.margin_per_point,
                        excl_xy=pp.excl_xy, excl_theta=pp.excl_theta, bounds=om.bounds(ga, nga, R0, t0), exhaustive=exhaustive)


def without_blocks(raw):
    """a posterior's bytes without blocks_evaluated, the one field that tells the two search forms apart"""
    return raw[:12] + raw[16:]


def held(cm, om, ga, nga, R0, t0, name=""):
    """match_post in both search forms: the pose and the result are match's, the posterior the restatement's, byte for byte;
    returns the pruned form's posterior"""
    wtab, pp, first = cm.post_table(), cm.post_params, None
    for ex in (0, 1):
        cm.set_exhaustive(ex)
        R, t, res, post = cm.match_post(ga, nga, R0, t0)
        Rm, tm, rm = cm.match(ga, nga, R0, t0)
        assert R.tobytes() == Rm.tobytes() and t.tobytes() == tm.tobytes() and bytes(res) == bytes(rm), (name, ex)
        want = oracle_post(om, ga, nga, R0, t0, wtab, pp, exhaustive=bool(ex))
        assert bytes(post) == PO.pack(want), (name, ex, [(f, getattr(post, f), want[f]) for f in PO.INT_FIELDS], post.m0, want["m0"])
        first = first or post
        assert without_blocks(bytes(post)) == without_blocks(bytes(first)), (name, ex)
    cm.set_exhaustive(0)
    return first


# ------------------------------------------------------------------ what the cases reach (no GPU)
def test_cases_reach_the_edges():
    box = K.box_model()
    om = CO.OracleMatcher(box[0], box[1])
    wtab = PO.weight_table(8.0)
    partial = pruned = ragged_within = with_second = without_second = last_entry = 0
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
        U = om.bounds(ga, nga, R0, t0)
        for mpp in PC.MARGINS:
            p = PO.posterior(vol, cnt, len(ga) + len(nga), wtab, 0.1, 0.01, margin_per_point=mpp, bounds=U)
            partial += 1 < p["n_within"] < vol.size
            pruned += p["blocks_evaluated"] < U.size
            with_second += p["second_score"] >= 0
            without_second += p["second_score"] < 0
            (k, b, a), top, M, d, mask = PO.within(vol, cnt, mpp)
            if win == (8, 8):
                ragged_within += bool(mask[:, 16, :].any() or mask[:, :, 16].any()) and not mask.all()
            last_entry += bool(M > 0 and (d[mask] * 256 // M).max() == 256)
            if mpp == 255:
                assert p["n_within"] == vol.size
            if name == "winner_in_ragged_block":
                assert (k, b, a) == (0, 16, 16)
    # some margins cut the volume, some lists are shorter than all blocks, candidates of a ragged block lie within a margin
    # that others miss, a second mode exists and is absent, and the table's last entry (d = M) is read
    reached = (partial, pruned, ragged_within, with_second, without_second, last_entry)
    assert min(reached) > 0, reached


# ------------------------------------------------------------------ every case, every margin
@pytest.fixture(scope="module")
def box():
    m = K.box_model()
    return m, CO.OracleMatcher(m[0], m[1]), api.CorrelativeMatcher(m[0], m[1])


@gpu
@pytest.mark.parametrize("mpp", PC.MARGINS)
def test_posterior_equals_the_restatement(box, mpp):
    _, om, cm = box
    cm.set_post_params(margin_per_point=mpp)
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        cm.set_window(win[0], win[1], ht, 0.01)
        post = held(cm, om, ga, nga, R0, t0, name)
        assert post.valid == 1 and post.m0 >= 65536
        if mpp == 255:
            assert post.n_within == (2 * win[0] + 1) * (2 * win[1] + 1) * (2 * ht + 1), name
        if name == "all_outside":
            assert post.n_within == 17 * 17 * 9 and post.m0 == post.n_within * 65536


@gpu
@pytest.mark.parametrize("mpp", PC.MARGINS)
def test_posterior_at_other_block_sizes(mpp):
    m = K.box_model()
    made = {}
    for name, D, ga, nga, R0, t0, win, ht in K.block_cases():
        if D not in made:
            made[D] = (CO.OracleMatcher(m[0], m[1], block=D), api.CorrelativeMatcher(m[0], m[1], block=D))
            made[D][1].set_post_params(margin_per_point=mpp)
        om, cm = made[D]
        om.set_window(win[0], win[1], ht, 0.01)
        cm.set_window(win[0], win[1], ht, 0.01)
        post = held(cm, om, ga, nga, R0, t0, "%s_D%d" % (name, D))
        assert post.valid == 1 and post.m0 >= 65536
        if mpp == 255:
            assert post.n_within == (2 * win[0] + 1) * (2 * win[1] + 1) * (2 * ht + 1), (name, D)
    for _, cm in made.values():
        cm.close()


@gpu
def test_other_weights_and_exclusions(box):
    _, om, cm = box
    name, ga, nga, R0, t0, win, ht = K.volume_cases()[7]          # 63 points, 17 x 17 x 9
    om.set_window(win[0], win[1], ht, 0.01)
    cm.set_window(win[0], win[1], ht, 0.01)
    for kw in (dict(beta=0.0), dict(beta=64.0, margin_per_point=40), dict(beta=0.37, excl_xy=0, excl_theta=0),
               dict(excl_xy=7, excl_theta=3, margin_per_point=100), dict(excl_xy=20, excl_theta=20, margin_per_point=255)):
        cm.set_post_params(**kw)
        post = held(cm, om, ga, nga, R0, t0, str(kw))
        if kw.get("excl_xy") == 20:
            assert post.second_score == -1                        # the box covers the window: no second mode


@gpu
def test_second_class_without_a_table():
    m_ga, m_nga = K.centre([0, 1, 2], [0, 0, 0]), K.box_model()[1]
    om, cm = CO.OracleMatcher(m_ga, m_nga), api.CorrelativeMatcher(m_ga, m_nga)
    cm.set_post_params()
    om.set_window(8, 8, 4, 0.01)
    cm.set_window(8, 8, 4, 0.01)
    for n in (5, 65):
        ga, nga = K.scan_of((K.box_model()[0], m_nga), n, K.TRUE_POSE, 500 + n, ga_share=0.4)
        R0, t0 = K.pose_Rt(K.TRUE_POSE[0] + 0.3, K.TRUE_POSE[1], K.TRUE_POSE[2] - 0.02)
        post = held(cm, om, ga, nga, R0, t0, "n%d" % n)
        assert post.margin == 16 * len(nga)                       # the GA points are not counted
    cm.close()


@gpu
def test_exact_tie_on_the_device():
    kw, m_ga, m_nga, ga, nga, R0, t0, winner, other, score = K.tie_case()
    om, cm = CO.OracleMatcher(m_ga, m_nga, **kw), api.CorrelativeMatcher(m_ga, m_nga, **kw)
    cm.set_post_params(margin_per_point=0)
    post = held(cm, om, ga, nga, R0, t0, "tie")
    assert (post.n_within, post.second_score, post.second_k, post.second_a, post.second_b) == (2, score, *other)
    assert list(post.mean) == [(-4.5) * 0.1, 0.5 * 0.1, 0.0]
    assert post.ambiguous(0)
    cm.close()


@gpu
@pytest.mark.parametrize("scene", ["room", "corridor"])
def test_scenes(scene):
    m_ga, m_nga, ga, nga, R0, t0 = PC.room_scene() if scene == "room" else PC.corridor_scene()
    om, cm = CO.OracleMatcher(m_ga, m_nga), api.CorrelativeMatcher(m_ga, m_nga)
    om.set_window(*PC.SCENE_WINDOW)
    cm.set_window(*PC.SCENE_WINDOW)
    cm.set_post_params()
    post = held(cm, om, ga, nga, R0, t0, scene)
    cc = [post.cov[0] / 0.01, post.cov[3] / 0.01, post.cov[5] / 1e-4]
    print("%s: n_within %d, blocks %d, cov in cells^2 / steps^2 %.3f %.3f %.3f, second %d" %
          (scene, post.n_within, post.blocks_evaluated, cc[0], cc[1], cc[2], post.second_score))
    if scene == "room":
        assert max(cc) < 0.5 and post.second_score == -1 and not post.ambiguous(1)
        assert post.information() is not None
    else:
        assert cc[0] >= 100.0 * cc[1] and post.ambiguous(1)
        assert post.covariance()[0, 0] > 100 * post.covariance()[1, 1]
    cm.close()


# ------------------------------------------------------------------ batches
@gpu
@pytest.mark.parametrize("n_scans", [1, 2, 37])
def test_batches(box, n_scans):
    _, om, cm = box
    om.set_window(8, 8, 4, 0.01)
    cm.set_window(8, 8, 4, 0.01)
    cm.set_post_params()
    wtab = cm.post_table()
    pts, off, nga, R0, t0 = K.batch_scans(n_scans)
    batch = synth.ScanBatch(pts, off, nga, R0, t0, None)
    first = None
    for ex in (0, 1, 0):
        cm.set_exhaustive(ex)
        R, t, res, post = cm.match_post_batch(batch)
        Rm, tm, resm = cm.match_batch(batch)
        assert R.tobytes() == Rm.tobytes() and t.tobytes() == tm.tobytes() and res.tobytes() == resm.tobytes()   # match_batch_dev's bits
        bits = b"".join(without_blocks(p.tobytes()) for p in post)
        first = first or bits
        assert bits == first                                      # twice the same bits, and the exhaustive form's
    cm.set_exhaustive(0)
    for s in range(n_scans):
        ga, ng = batch.scan(s)
        want = oracle_post(om, ga, ng, R0[s], t0[s], wtab, cm.post_params)
        assert post[s].tobytes() == PO.pack(want), s
        if len(ga) + len(ng) < 5:
            assert post[s]["valid"] == 0 and post[s]["second_score"] == -1 and post[s]["m0"] == 0
        else:
            Ra, ta, ra, pa = cm.match_post(ga, ng, R0[s], t0[s])  # the scan alone: the same bits as in the batch
            assert bytes(pa) == post[s].tobytes() and bytes(ra) == res[s].tobytes(), s
    if n_scans > 2:
        assert post[n_scans // 2]["valid"] == 0
    # beyond what was reserved, or over the start translations: refused, not overrun
    d = [api.DeviceArray.from_host(x) for x in (pts, off, nga, R0, t0, np.stack([cm.angles(r) for r in R0]))]
    d_R, d_t = api.DeviceArray((n_scans, 4), np.float64), api.DeviceArray((n_scans, 2), np.float64)
    d_res, d_post = api.DeviceArray((n_scans,), api.CSM_RESULT_DTYPE), api.DeviceArray((n_scans,), api.CSM_POST_DTYPE)
    for args in ((cm.info()["max_scans"] + 1, d_R, d_t), (n_scans, d_R, d[4])):
        with pytest.raises(api.SlamError) as e:
            cm.match_post_batch_dev(d[0], d[1], d[2], args[0], d[3], d[4], d[5], args[1], args[2], d_res, d_post)
        assert e.value.code == api.E_INVALID
    # without a result array, and R in place
    cm.match_post_batch_dev(d[0], d[1], d[2], n_scans, d[3], d[4], d[5], d[3], d_t, None, d_post)
    api.synchronize()
    assert d_post.download().tobytes() == post.tobytes() and d[3].download().tobytes() == R.tobytes()


# ------------------------------------------------------------------ the table and the refusals
@gpu
def test_post_table_is_the_formula(box):
    _, _, cm = box
    for beta in (8.0, 0.0, 0.37, 64.0):
        cm.set_post_params(beta=beta)
        got = cm.post_table()
        assert got.dtype == np.uint32 and np.array_equal(got, PO.weight_table(beta)), beta
        assert got[0] == 65536


@gpu
def test_refusals():
    m = K.box_model()
    ga, nga = K.scan_of(m, 65, K.TRUE_POSE, 1)
    R0, t0 = K.pose_Rt(*K.TRUE_POSE)
    cm = api.CorrelativeMatcher(m[0], m[1], half_x=8, half_y=8, half_theta=4)
    for call in (lambda: cm.match_post(ga, nga, R0, t0), cm.post_table):       # before set_post_params
        with pytest.raises(api.SlamError) as e:
            call()
        assert e.value.code == api.E_INVALID
    for kw in (dict(margin_per_point=256), dict(margin_per_point=-1), dict(beta=float("nan")), dict(beta=64.5), dict(beta=-1.0),
               dict(excl_xy=-1), dict(excl_theta=-1)):
        with pytest.raises(api.SlamError) as e:
            cm.set_post_params(**kw)
        assert e.value.code == api.E_INVALID, kw
    with pytest.raises(api.SlamError):
        cm.post_table()                                            # a refused set leaves the handle without a table
    cm.set_post_params()
    R, t, res, post = cm.match_post(ga, nga, R0, t0)
    assert post.valid == 1
    # the guard: 65536 * 32766^2 * 163835 >= 2^63; set_window itself accepts the window and match still answers
    assert not PO.guard_ok(2 * 16383 + 1, 1, 5)
    cm.set_window(16383, 0, 2, 0.01)
    with pytest.raises(api.SlamError) as e:
        cm.match_post(ga, nga, R0, t0)
    assert e.value.code == api.E_INVALID
    assert PO.guard_ok(2 * 16383 + 1, 1, 3)
    cm.set_window(16383, 0, 1, 0.01)
    R, t, res, post = cm.match_post(ga, nga, R0, t0)
    Rm, tm, rm = cm.match(ga, nga, R0, t0)
    assert post.valid == 1 and bytes(res) == bytes(rm)
    # a scan of four points is the host form's error, as in slam_csm_match
    with pytest.raises(api.SlamError) as e:
        cm.match_post(ga[:0], nga[:4], R0, t0)
    assert e.value.code == api.E_TOO_FEW_SCENE
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
def test_create_match_post_destroy_gives_the_memory_back():
    m = K.box_model()
    ga, nga = K.scan_of(m, 65, K.TRUE_POSE, 1)
    R0, t0 = K.pose_Rt(*K.TRUE_POSE)

    def cycle():
        cm = api.CorrelativeMatcher(m[0], m[1], half_x=8, half_y=8, half_theta=4)
        cm.set_post_params()
        cm.reserve(3)
        R, t, r, p = cm.match_post(ga, nga, R0, t0)
        cm.close()
        return R.tobytes() + t.tobytes() + bytes(r) + bytes(p)

    first = cycle()
    for _ in range(2):
        assert cycle() == first
    before = free_bytes()
    for _ in range(40):
        assert cycle() == first
    after = free_bytes()
    print("csm posterior lifetime: free before %d, after 40 cycles %d (drift %d bytes)" % (before, after, before - after))
    assert before - after == 0
