"""The particle filter on the device (slam_pf_*, slam_amd.api.ParticleFilter, docs/PARTICLE_FILTER.md) against the numpy
restatement of tests/pf_cases.py: random words, particles, log-weights, weights, every integer sum, the decision and the
resampled set are equal with no tolerance; the one exception is theta of the estimate, held to 1e-12 because two libms may differ
in atan2's last place."""
import contextlib

import numpy as np
import pytest

import csm_plane_cases as P
import pf_cases as F
from slam_amd import api

gpu = pytest.mark.gpu
STATE_INTS = ("t", "n", "resampled", "degenerate", "best", "A_max", "W", "S2", "MX", "MY", "MC", "MS", "n_resamples", "refused")


def pair(n, **kw):
    """a device filter and its restatement over the same tables"""
    pf = api.ParticleFilter(n, **kw)
    cs, G, wtab = pf.tables()
    p = pf.params
    ref = F.Filter(cs, G, wtab, n_particles=p.n_particles, n_angles=p.n_angles, gauss_bits=p.gauss_bits, weight_len=p.weight_len,
                   weight_shift=p.weight_shift, resample_num=p.resample_num, resample_den=p.resample_den, weight_scale=p.weight_scale, seed=p.seed)
    return pf, ref


def same_particles(pf, ref):
    x, y, k = pf.particles()
    assert np.array_equal(x, ref.x, equal_nan=True) and np.array_equal(y, ref.y, equal_nan=True), (x[:4], ref.x[:4])
    assert np.array_equal(k, ref.k)


def same_state(s, want):
    got = {f: int(getattr(s, f)) for f in STATE_INTS}
    assert got == {f: int(want[f]) for f in STATE_INTS}, (got, want)
    if want["W"]:
        assert s.x == want["x"] and s.y == want["y"] and abs(s.theta - want["theta"]) <= 1e-12, (s.x, s.y, s.theta, want)
    else:
        assert np.isnan(s.x) and np.isnan(s.y) and np.isnan(s.theta)


def same_everything(pf, ref, want):
    same_state(pf.state(), want)
    same_particles(pf, ref)
    acc, w = pf.weights()
    assert np.array_equal(acc, ref.acc) and np.array_equal(w, ref.w)


# ------------------------------------------------------------------------------------------------------------ random words
@gpu
def test_random_words_are_philox():
    for v in F.PHILOX_VECTORS:                                                   # the restatement itself, once more where the device runs
        assert F.philox(np.array(v[0]), v[1]).tolist() == list(v[2])
    pf = api.ParticleFilter(64, seed=0x299f31d0a4093822)
    for t in (0, 1, 2 ** 32 - 1):
        for p0, n, purpose in ((0, 600, 0), (60, 8, 1), (250, 12, 2), (2 ** 32 - 5, 9, 0), (0x243f6a88, 1, 0x13198a2e)):
            got = pf.random_words(p0, n, t, purpose)
            assert np.array_equal(got, F.words(pf.params.seed, (p0 + np.arange(n)) & F.MASK, t, purpose)), (t, p0)
    assert pf.random_words(0, 0, 0, 0).shape == (0, 4)
    pf.close()


# ----------------------------------------------------------------------------------------------------------------- predict
@gpu
@pytest.mark.parametrize("A,b", ((64, 4), (65536, 16)))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 1025, 4097))
def test_predict_equals_the_restatement(n, A, b):
    pf, ref = pair(n, n_angles=A, gauss_bits=b, seed=77 + n)
    rs = np.random.RandomState(n)
    x, y, k = rs.uniform(-20, 20, n), rs.uniform(-20, 20, n), rs.randint(0, A, n)
    k[0] = A - 1
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    same_particles(pf, ref)                                                       # the round trip
    motions = ((0.12, -0.01, 0.02, 0.03, 1.5, 3), (0.3, 0.0, 0.0, 0.0, 0.0, -(A + 7)), (-0.2, 0.1, 0.05, 0.01, 0.0, A + 3),
               (0.0, 0.0, 1.0, 2.0, A / 8.0, -1), (1e-3, 1e3, 0.5, 0.5, 1000.0, (1 << 20) - 1))
    for i, m in enumerate(motions):                                               # five steps in a row: the counter
        pf.predict(m), ref.predict(m)
        same_particles(pf, ref)
        assert pf.state().t == ref.t == i + 1
    assert not np.array_equal(ref.x, x)
    pf.init_gaussian(1.5, -2.5, A - 2, 0.2, 0.1, 4.0), ref.init_gaussian(1.5, -2.5, A - 2, 0.2, 0.1, 4.0)
    same_particles(pf, ref)
    assert pf.state().t == 5 and (pf.weights()[0] == 0).all()
    pf.close()


@gpu
def test_a_motion_that_breaks_the_rules_is_refused_on_the_device_too():
    pf, ref = pair(300)
    pf.init_gaussian(0, 0, 0, 0.1, 0.1, 2.0), ref.init_gaussian(0, 0, 0, 0.1, 0.1, 2.0)
    d_m = api.DeviceArray((1,), api.PF_MOTION_DTYPE)
    for m in ((0.1, 0.0, np.nan, 0.0, 0.0, 0), (0.1, 0.0, 0.1, 0.1, 2.0 ** 20, 0), (0.1, 0.0, 0.1, 0.1, 1.0, -(1 << 20)), (0.1, 0.0, 0.1, 0.1, 1.0, 5)):
        with pytest.raises(api.SlamError) if not F.motion_ok(m) else contextlib.nullcontext():
            pf.predict(m)                                                         # the host form refuses before the device
        if F.motion_ok(m):
            ref.predict(m)
        d_m.upload(np.array([m], api.PF_MOTION_DTYPE))
        pf.predict_dev(d_m)
        ref.predict(m)
        same_particles(pf, ref)
    s = pf.state()
    assert (s.t, s.refused) == (ref.t, ref.refused) == (2, 3)
    pf.close()


@gpu
def test_a_filter_created_with_null_params_has_the_defaults():
    import ctypes as C
    L, h, s = api.lib(), C.c_void_p(), api.PfState()
    api.check(L.slam_pf_create(None, C.byref(h)))
    try:
        api.check(L.slam_pf_read_state(h, C.byref(s)))
        assert (s.n, s.t) == (F.DEFAULTS["n_particles"], 0) == (1024, 0)
    finally:
        L.slam_pf_destroy(h)


# -------------------------------------------------------------------------------------------------------------- resampling
@pytest.fixture(scope="module")
def big_filter():
    pf = api.ParticleFilter(1 << 18)
    yield pf
    pf.close()


@gpu
@pytest.mark.parametrize("name", sorted(F.resample_cases()))
def test_resample_indices_equal_the_restatement(big_filter, name):
    w = F.resample_cases()[name]
    for r in F.offsets_of(w):
        got = big_filter.resample_indices(w, r)
        assert np.array_equal(got, F.resample_search(w, r)), (name, r)
    st = api.Stream()
    assert np.array_equal(big_filter.resample_indices(w, 12345678901234567, stream=st), F.resample_search(w, 12345678901234567))
    assert np.array_equal(big_filter.resample_indices(np.where(w > 0, w + (1 << 20), 0), 3), F.resample_search(np.where(w > 0, F.ONE, 0), 3))


# ------------------------------------------------------------------------------------------------------------------ update
@pytest.fixture(scope="module")
def room():
    """the 97 x 83 plane of tests/csm_plane_cases.py with a 150-point scan inside it, and a matcher over it"""
    c = P.case("97x83_inside")
    cm = api.CorrelativeMatcher.from_plane(c["plane"], c["ox"], c["oy"], resolution=c["res"])
    yield c, cm, (c["ox"], c["oy"], c["plane"])
    cm.close()


def scatter(c, n, seed, A):
    """particles about the plane's window (the scan's points are in the lattice frame: the identity pose scores highest)"""
    rs = np.random.RandomState(seed)
    x, y = rs.normal(0.0, 0.4, n), rs.normal(0.0, 0.4, n)
    k = rs.randint(-A // 64, A // 64, n) % A
    return x, y, k


def steps_equal(pf, ref, c, cm, tab, steps, centre=(0.0, 0.0), dev=False, pts=None, n_ga=None):
    pts = c["pts"] if pts is None else pts
    n_ga = c["n_ga"] if n_ga is None else n_ga
    st = api.Stream() if dev else None
    d_pts = api.DeviceArray.from_host(pts) if dev else None
    out = []
    for i in range(steps):
        if i:
            m = (0.02, 0.01, 0.03, 0.03, 2.0, 1)
            pf.predict(m), ref.predict(m)
        want = ref.update((tab, tab), pts, n_ga, c["res"], centre[0], centre[1])
        if dev:
            pf.update_dev(d_pts, len(pts), n_ga, matcher=cm, centre=centre, stream=st)
            st.synchronize()
        else:
            pf.update(pts[:n_ga], pts[n_ga:], matcher=cm, centre=centre)
        same_everything(pf, ref, want)
        out.append(want)
    return out


@gpu
@pytest.mark.parametrize("n", (1, 255, 1025))
@pytest.mark.parametrize("dev", (False, True))
def test_update_never_resampling_accumulates(room, n, dev):
    c, cm, tab = room
    pf, ref = pair(n, resample_num=0, weight_scale=4096.0)
    x, y, k = scatter(c, n, 5, 4096)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    states = steps_equal(pf, ref, c, cm, tab, 4, dev=dev)
    assert all(s["resampled"] == 0 for s in states) and states[-1]["A_max"] > states[0]["A_max"] > 0 and ref.n_resamples == 0
    assert n == 1 or len(set(ref.w.tolist())) > 3
    pf.close()


@gpu
@pytest.mark.parametrize("n", (1, 256, 257, 1500))
@pytest.mark.parametrize("dev", (False, True))
def test_update_always_resampling_copies_and_zeroes(room, n, dev):
    c, cm, tab = room
    pf, ref = pair(n, resample_num=2, resample_den=1, weight_scale=2048.0)
    x, y, k = scatter(c, n, 6, 4096)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    states = steps_equal(pf, ref, c, cm, tab, 3, dev=dev)
    assert all(s["resampled"] == 1 for s in states) and (ref.acc == 0).all() and ref.n_resamples == 3
    assert n == 1 or len(np.unique(states[0]["src"])) < n                        # some particle was copied twice
    pf.close()


@gpu
def test_the_default_threshold_one_unit_on_either_side():
    """four particles over a flat plane: one keeps the whole scan inside it, three keep none of it, so w = (65536, v, v, v) with v the
    second entry of a two-entry weight table.  2 W^2 < 4 S2 holds up to some v* and fails from v* + 1 on."""
    c = P.case("tie")
    cm = api.CorrelativeMatcher.from_plane(c["plane"], c["ox"], c["oy"], resolution=c["res"])
    tab = (c["ox"], c["oy"], c["plane"])

    def decided(v):
        W, S2 = F.ONE + 3 * v, F.ONE * F.ONE + 3 * v * v
        return 2 * W * W < 4 * S2

    v_star = max(v for v in range(F.ONE) if decided(v))
    assert decided(v_star) and not decided(v_star + 1) and 10000 < v_star < 10300
    for v, want_flag in ((v_star, 1), (v_star + 1, 0)):
        pf, ref = pair(4, weight_len=2, weight_shift=0)
        wtab = np.array([F.ONE, v], np.uint32)
        pf.set_tables(wtab=wtab)
        ref.wtab = wtab.astype(np.int64)
        x, y, k = np.array([0.0, 500.0, 0.0, -500.0]), np.array([0.0, 0.0, 500.0, 0.0]), np.zeros(4, np.int32)
        pf.set_particles(x, y, k), ref.set_particles(x, y, k)
        want = steps_equal(pf, ref, c, cm, tab, 1)[0]
        assert want["resampled"] == want_flag and ref.w.tolist() == [F.ONE, v, v, v] and want["best"] == 0
        pf.close()
    cm.close()


@gpu
@pytest.mark.parametrize("num,den", ((0, 1), (2, 1), (1, 2)))
def test_non_finite_particles_take_no_part(room, num, den):
    c, cm, tab = room
    n = 300
    pf, ref = pair(n, resample_num=num, resample_den=den, weight_scale=8192.0)
    x, y, k = scatter(c, n, 8, 4096)
    x[0], y[7], x[255], y[256], x[299] = np.nan, np.inf, -np.inf, np.nan, np.inf
    x[100] = 1.0e5                                                               # finite: q saturates; it scores nothing
    y[101] = -1.0e300
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    states = steps_equal(pf, ref, c, cm, tab, 2)
    assert states[0]["best"] not in (0, 7, 255, 256, 299)
    if num == 0:
        assert (ref.w[[0, 7, 255, 256, 299]] == 0).all() and ref.w[100] > 0 and np.isnan(ref.x[0]) and np.isinf(ref.x[299])
    if num == 2:
        assert np.isfinite(ref.x).all() and np.isfinite(ref.y).all()             # none of them was ever copied
    pf.close()


@gpu
def test_q_saturates():
    c = P.case("97x83_outside")
    cm = api.CorrelativeMatcher.from_plane(c["plane"], c["ox"], c["oy"], resolution=c["res"])
    pf, ref = pair(3, resample_num=0)
    x, y, k = np.array([1.0e5, -8191.5, 8191.9999999]), np.array([-1.0e300, 8192.0, 0.25]), np.array([0, 1024, 4095], np.int32)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    want = steps_equal(pf, ref, c, cm, (c["ox"], c["oy"], c["plane"]), 1)[0]
    assert want["MX"] == F.ONE * (F.Q_LIMIT + int(-8191.5 * 65536) + F.Q_LIMIT) and want["W"] == 3 * F.ONE
    pf.close(), cm.close()


@gpu
def test_no_finite_particle_is_degenerate(room):
    c, cm, tab = room
    pf, ref = pair(70, resample_num=2, resample_den=1)
    x, y, k = np.full(70, np.nan), np.full(70, np.inf), np.arange(70, dtype=np.int32)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    want = steps_equal(pf, ref, c, cm, tab, 2)[1]
    assert want["degenerate"] == 1 and want["resampled"] == 0 and want["W"] == 0 and want["best"] == -1
    pf.close()


@gpu
def test_a_scan_wholly_outside_the_table_weighs_every_particle_alike():
    c = P.case("97x83_outside")
    cm = api.CorrelativeMatcher.from_plane(c["plane"], c["ox"], c["oy"], resolution=c["res"])
    pf, ref = pair(513)
    x, y, k = scatter(c, 513, 9, 4096)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    want = steps_equal(pf, ref, c, cm, (c["ox"], c["oy"], c["plane"]), 2)[1]
    assert want["A_max"] == 0 and want["W"] == 513 * F.ONE and want["resampled"] == 0 and want["best"] == 0
    pf.close(), cm.close()


@gpu
@pytest.mark.parametrize("dev", (False, True))
def test_the_windows_centre_is_subtracted(room, dev):
    c, cm, tab = room
    centre = (37.5, -12.25)
    pf, ref = pair(400, weight_scale=4096.0)
    x, y, k = scatter(c, 400, 10, 4096)
    pf.set_particles(x + centre[0], y + centre[1], k), ref.set_particles(x + centre[0], y + centre[1], k)
    states = steps_equal(pf, ref, c, cm, tab, 3, centre=centre, dev=dev)
    assert states[0]["A_max"] > 150 * 20
    other = F.Filter(ref.cs, ref.G, ref.wtab, n_particles=400, weight_scale=4096.0)
    other.set_particles(x + centre[0], y + centre[1], k)
    assert other.update((tab, tab), c["pts"], c["n_ga"], c["res"])["A_max"] != states[0]["A_max"]   # the centre matters here
    pf.close()


# ------------------------------------------------------------------------------------------------------------------- graph
@gpu
def test_predict_and_update_replay_in_a_graph(room):
    c, cm, tab = room
    n = 700
    pf, ref = pair(n, weight_scale=2048.0)
    x, y, k = scatter(c, n, 12, 4096)
    pf.set_particles(x, y, k), ref.set_particles(x, y, k)
    d_pts, d_m = api.DeviceArray.from_host(c["pts"]), api.DeviceArray((1,), api.PF_MOTION_DTYPE)
    motions = ((0.05, 0.0, 0.02, 0.02, 1.0, 2), (-0.03, 0.04, 0.05, 0.01, 3.0, -4), (0.0, -0.02, 0.01, 0.04, 0.0, 4095))
    st = api.Stream()
    d_m.upload(np.array([motions[0]], api.PF_MOTION_DTYPE))
    with api.Graph(st) as graph:
        pf.predict_dev(d_m, stream=st)
        pf.update_dev(d_pts, len(c["pts"]), c["n_ga"], matcher=cm, stream=st)
    st.synchronize()
    same_particles(pf, ref)                                                       # capturing ran nothing
    assert pf.state().t == 0
    for m in motions:
        d_m.upload(np.array([m], api.PF_MOTION_DTYPE))                            # (a synchronous copy: it is there before the launch)
        graph.launch()
        st.synchronize()
        ref.predict(m)
        want = ref.update((tab, tab), c["pts"], c["n_ga"], c["res"])
        same_everything(pf, ref, want)
    assert pf.state().t == 3 and ref.n_resamples >= 1
    pf.close()


# -------------------------------------------------------------------------------------------------------------- end to end
class DeviceLoop:
    """the shape pf_cases.run_loop drives, over a GridMatcher's filter"""

    def __init__(self, pf):
        self.pf = pf

    def init_gaussian(self, *a):
        self.pf.init_gaussian(*a)

    def predict(self, m):
        self.pf.predict(m)

    def update(self, tabs, pts, n_ga, res):
        s = self.pf.update(pts[:n_ga], pts[n_ga:])
        return dict(x=s.x, y=s.y, state=s)


@pytest.fixture(scope="module")
def grid_matcher():
    import csm_oracle as CO
    L = F.LOOP
    m_ga, m_nga = CO.synth_map()
    g = api.Grid(L["size"], L["size"], L["res"], min_cluster_points=0)
    g.add_endpoints(np.concatenate([m_ga, m_nga]).astype(np.float32), np.zeros((0, 2), np.float32))
    g.finalize()
    gm = api.GridMatcher(g, L["sigma"])
    gm.update()
    api.synchronize()
    plane = P.likelihood_plane(g.read_occupancy(), g.size_x, g.size_y, g.resolution, L["sigma"], L["R"])
    yield gm, plane
    gm.close()


@gpu
@pytest.mark.parametrize("seed", F.LOOP["seeds"])
def test_twenty_scans_in_the_grid_equal_the_restatement_and_beat_dead_reckoning(grid_matcher, seed):
    gm, plane = grid_matcher
    assert gm.max_cells == F.LOOP["R"] and gm.centre == (0.0, 0.0)
    pf = gm.particle_filter(1024, seed=seed)
    cs, G, wtab = pf.tables()
    ref = F.Filter(cs, G, wtab, seed=seed)
    tab = (-(F.LOOP["size"] // 2), -(F.LOOP["size"] // 2), plane)
    seen = []
    want_errs = F.run_loop(ref, (tab, tab), each=lambda i, f, st: seen.append((dict(st), f.x.copy(), f.y.copy(), f.k.copy(), f.acc.copy(), f.w.copy())))

    def each(i, f, st):
        want, x, y, k, acc, w = seen[i]
        same_state(st["state"], want)
        gx, gy, gk = f.pf.particles()
        gacc, gw = f.pf.weights()
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gk, k) and np.array_equal(gacc, acc) and np.array_equal(gw, w), i

    errs = F.run_loop(DeviceLoop(pf), None, each=each)
    assert errs == want_errs
    wins = sum(a < b for a, b in errs)
    print("seed %d: filter / dead reckoning at the last step %.4f / %.4f m, nearer at %d of 20 steps" % (seed, errs[-1][0], errs[-1][1], wins))
    assert errs[-1][0] < errs[-1][1] and wins >= 15
    pf.close()
