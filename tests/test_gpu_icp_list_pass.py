"""The list form's pass (list_search, icp.hip) at the edges of its window and of a team's passes.

The window reads eleven CONSECUTIVE entries from the first one it examines, in one batch, and masks what lies past the last:
entries of the next list, or the cell tables behind the last list of the blob.  So: lists shorter than, as long as and
longer than the window, queries that start at a list's first and last entry, the last list of the blob, both classes and
the point-to-line mode, exact ties (duplicated model points; two DIFFERENT points at one float distance), and scans whose sizes sit around the boundaries of a team's
passes and cooperative rounds, in pairs and one per workgroup, with every query far from the map.

Every result is the CPU oracle's, compared as tests/test_gpu_icp_pair.py::check compares; every case first asserts, on the
CPU (the oracle's kd-tree, the index built on the host), that its input holds what it claims.

What no case here can catch: a mask that lets an entry of the NEXT list into the window.  Halo lists of neighbouring cells hold
the same model points, so such an entry is a true candidate or a tie, and the exact pass gives the right answer either way; only
the speed would suffer."""
import numpy as np
import pytest

import oracle_lib as O
from slam_amd import api, synth

pytestmark = pytest.mark.gpu
POS_TOL, ANG_TOL = 1e-4, 1e-5
SIZES = [1, 2, 5, 10, 11, 12]   # entries per cluster: below, at and above the window's 11
LIST_OVERREAD = 96              # icp_model.hpp: bytes behind the last entry that lie inside the blob


def yaw(R):
    R = np.asarray(R).reshape(-1, 4)
    return np.arctan2(R[:, 2], R[:, 0])


def ang_diff(a, b):
    d = a - b
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)


def check(m_ga, m_nga, batch, max_iter, pair, first=1, mode=None, indist=5.0):
    """GPU against oracle: step counts and n_corr equal, poses, delta, two runs bit-identical.  Returns the handle's info."""
    p2l = mode == api.ICP_P2L
    kw = dict(mode=api.ICP_P2L, normals_k=10) if p2l else {}
    icp = api.Icp(m_ga, m_nga, max_iter=max_iter, min_delta=-1.0, pair_scans=pair, spread_scans=-1, first_iterations=first,
                  far_div=1, **kw)
    info = icp.index_info()
    R, t, res, _ = icp.fit_batch(batch, indist=indist)
    R2, t2, res2, _ = icp.fit_batch(batch, indist=indist)
    icp.close()
    assert info["two_forms"] and info["first_iterations"] == first   # the list form takes over after `first` iterations
    assert np.array_equal(R, R2) and np.array_equal(t, t2) and np.array_equal(res["n_corr"], res2["n_corr"])
    model = O.IcpModel(m_ga, m_nga, normals_k=10) if p2l else O.IcpModel(m_ga, m_nga)
    prm = O.icp_params(max_iter, -1.0, indist, O.NN_KDTREE, O.MODE_P2L) if p2l else O.icp_params(max_iter, -1.0, indist)
    Ro, to, iters, ncorr, delta = model.fit_batch(batch.pts, batch.scan_off, batch.scan_nga, batch.R, batch.t, prm)
    odd = np.abs(res["delta"] - delta) >= 1e-9
    if odd.any():
        # an exact float distance tie somewhere in these scans: the kd-tree takes the candidate it visits last (kdtree.cpp:612-618),
        # the GPU and the brute-force arbiter (kdtree.cpp:360-375) the lowest index -- the arbiter decides, as in test_gpu_icp.py
        print("scans decided by the arbiter:", np.flatnonzero(odd))
        arb = O.icp_params(max_iter, -1.0, indist, O.NN_BRUTE, O.MODE_P2L if p2l else O.MODE_P2P)
        Rb, tb, ib, nb, db = model.fit_batch(batch.pts, batch.scan_off, batch.scan_nga, batch.R, batch.t, arb)
        Ro[odd], to[odd], iters[odd], ncorr[odd], delta[odd] = Rb[odd], tb[odd], ib[odd], nb[odd], db[odd]
    print("max |dt| %.3g  max |dyaw| %.3g  max |ddelta| %.3g" % (np.abs(t - to).max(), ang_diff(yaw(R), yaw(Ro)).max(),
                                                                np.abs(res["delta"] - delta).max()))
    assert np.array_equal(res["iters"], iters), (res["iters"], iters)
    assert np.array_equal(res["n_corr"], ncorr), (res["n_corr"], ncorr)
    assert np.abs(t - to).max() < POS_TOL and ang_diff(yaw(R), yaw(Ro)).max() < ANG_TOL
    assert np.abs(res["delta"] - delta).max() < 1e-9
    return info


def list_lengths(m_ga, m_nga, **kw):
    """Entries of every halo list, per class, read from the lists' blob as the HOST build lays it out: entries (float2), then
    a table of u16 list starts per class, then the key tables; the blob ends no sooner than LIST_OVERREAD bytes behind the
    entries.  The number of cells is the one for which the tables' sizes and the starts' last values add up."""
    icp = api.Icp(m_ga, m_nga, build_on_host=1, **kw)
    blob = icp.index_blob(1)
    icp.close()
    a16 = lambda v: (v + 15) & ~15
    found = []
    for nc in range(1, 1 << 16):
        tables = 2 * a16(2 * (nc + 1)) + 2 * a16(4 * (nc // 16 + 1))
        ptsb = blob.size - max(tables, LIST_OVERREAD)
        if ptsb < 0:
            break
        if ptsb % 16:
            continue
        s0 = blob[ptsb:ptsb + 2 * (nc + 1)].view(np.uint16).astype(np.int64)
        s1 = blob[ptsb + a16(2 * (nc + 1)):ptsb + a16(2 * (nc + 1)) + 2 * (nc + 1)].view(np.uint16).astype(np.int64)
        if s0[0] or s1[0] or (np.diff(s0) < 0).any() or (np.diff(s1) < 0).any() or a16(8 * (s0[-1] + s1[-1])) != ptsb:
            continue
        found.append((np.diff(s0), np.diff(s1), blob.size - ptsb))
    # (cell counts that round to the same table sizes parse alike and differ in empty lists at the end only)
    assert found and all(np.array_equal(f[k][f[k] > 0], found[0][k][found[0][k] > 0]) for f in found for k in (0, 1)), len(found)
    return found[0]


def cluster_model(dup=1):
    """Per class one short row of points per size in SIZES, 2 cm apart, the rows 3 m from each other: a halo list holds (part
    of) one row.  Class GA: rows along x; class NGA: rows along y.  dup: every point that many times over (exact ties)."""
    ga, ng = [], []
    for k, n in enumerate(SIZES):
        i = np.arange(n) * 0.02
        ga.append(np.stack([3.0 * k + i, np.full(n, 0.3 * k)], 1))
        ng.append(np.stack([np.full(n, 2.0 + 0.3 * k), 4.0 + 3.0 * k + i], 1))
    return np.repeat(np.concatenate(ga), dup, 0), np.repeat(np.concatenate(ng), dup, 0)


def cluster_scans(m_ga, m_nga, n_scans, per_point=8):
    """Scans that look at every model point `per_point` times: 3 mm of noise across a row, and along it up to 12 cm -- past
    both ends of every row, where a query's start in the list is the list's first or last entry."""
    pts, off, nga, Rs, ts = [], [0], [], [], []
    for s in range(n_scans):
        rs = np.random.RandomState(100 + s)
        q = []
        for m, along in ((m_ga, 0), (m_nga, 1)):
            w = np.repeat(m, per_point, 0)
            e = rs.normal(0.0, 0.003, w.shape)
            e[:, along] = np.tile(np.linspace(-0.12, 0.12, per_point), len(m))   # every point: both ends
            q.append(w + e)
        th = 0.001 * (s + 1)
        R, t = synth.pose_to_Rt(0.01 * (s + 1), -0.01, th)
        pts += [(qq - t) @ R for qq in q]   # sensor frame: R^T (q - t)
        off.append(off[-1] + len(q[0]) + len(q[1]))
        nga.append(len(q[0]))
        R0, t0 = synth.pose_to_Rt(0.0, 0.0, 0.0)
        Rs.append(R0.reshape(4))
        ts.append(t0)
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(Rs), np.array(ts), np.zeros((n_scans, 3)))


def nn_dist(model_xy, q):
    tree = O.KdTree(np.asarray(model_xy, np.float32))
    return np.sqrt(np.array([tree.nn1(x, y)[0] for x, y in np.asarray(q, np.float32)]))


@pytest.mark.parametrize("pair", [2, -1])
@pytest.mark.parametrize("mode", ["p2p", "p2l"])
def test_window_edges_short_lists_and_last_list(mode, pair):
    """lists of 1, 2, 5, 10, 11 and 12 entries in both classes (point-to-line: one class), queries past both ends of each, the
    last list of the blob among them; a scan of more than one pass of a pair's team, so that the PASS searches them"""
    m_ga, m_nga = cluster_model()
    p2l = mode == "p2l"
    kw = dict(mode=api.ICP_P2L, normals_k=10) if p2l else {}
    l0, l1, behind = list_lengths(m_ga, m_nga, **kw)
    assert behind >= LIST_OVERREAD                                   # what the window may read past the last list is blob
    for lens in ((l1,) if p2l else (l0, l1)):
        assert set(SIZES) <= set(lens.tolist()), sorted(set(lens.tolist()))
    batch = cluster_scans(m_ga, m_nga, 2)
    assert batch.scan_off[1] > 512 + 128                             # two passes of 512 lanes, one of 1024
    q_ga, q_ng = batch.scan(0)
    for k, n in enumerate(SIZES):                                    # queries beyond both ends of every row, along its key
        # (at the initial pose, the identity, sensor and world frame are one; registering moves a query by the scan's true pose,
        # at most 2 cm and 2 mrad at 19 m: 6 cm or less, and the outermost queries are placed 12 cm past the ends.  That a row's list is keyed along the row is
        # the build's choice -- the axis of larger extent -- and not asserted.)
        assert (q_ga[:, 0] < 3.0 * k - 0.06).any() and (q_ga[:, 0] > 3.0 * k + 0.02 * (n - 1) + 0.06).any()
        assert (q_ng[:, 1] < 4.0 + 3.0 * k - 0.06).any() and (q_ng[:, 1] > 4.0 + 3.0 * k + 0.02 * (n - 1) + 0.06).any()
    info = check(m_ga, m_nga, batch, 5, pair, first=(2 if p2l else 1), mode=api.ICP_P2L if p2l else None)
    near = np.concatenate([nn_dist(m_ga, q_ga), nn_dist(m_nga, q_ng)]) < info["list_certified_radius"]
    print("queries within the certified radius at the initial pose: %.2f" % near.mean())
    assert near.mean() > 0.5                                         # most queries are the window's to decide


@pytest.mark.parametrize("pair", [2, -1])
@pytest.mark.parametrize("mode", ["p2p", "p2l"])
def test_exact_ties_reach_the_exact_pass(mode, pair):
    """every model point twice: whatever the window finds, its second best equals its best.  The two candidates have the same
    coordinates (and, point-to-line, normals from the same neighbourhood), so this case shows that a window full of ties
    still ends in the oracle's sums; that a tie is NOTICED is the case of two different points below."""
    m_ga, m_nga = cluster_model(dup=2)
    p2l = mode == "p2l"
    assert len(np.unique(m_ga, axis=0)) * 2 == len(m_ga) and len(np.unique(m_nga, axis=0)) * 2 == len(m_nga)
    l0, l1, _ = list_lengths(m_ga, m_nga, **(dict(mode=api.ICP_P2L, normals_k=10) if p2l else {}))
    for lens in ((l1,) if p2l else (l0, l1)):
        assert set(2 * n for n in SIZES) <= set(lens.tolist())
    check(m_ga, m_nga, cluster_scans(m_ga, m_nga, 2, per_point=4), 4, pair, first=(2 if p2l else 1), mode=api.ICP_P2L if p2l else None)


def sized_batch(sizes, dx):
    """scans of exactly `sizes` points of the synthetic world, every initial pose `dx` metres off along x AND y (the walls run
    along the axes: off along one only, a wall along it still has its points under the queries)"""
    pts, off, nga, Rs, ts = [], [0], [], [], []
    for k, n in enumerate(sizes):
        ga, ng, pose = synth.make_scan(5 * k, 256, n_beams=n + 80)
        assert len(ga) + len(ng) >= n
        ga = ga[:min(len(ga), n // 2)]
        ng = ng[:n - len(ga)]
        assert len(ga) + len(ng) == n
        pts += [ga, ng]
        off.append(off[-1] + n)
        nga.append(len(ga))
        R, t = synth.pose_to_Rt(pose[0] + dx, pose[1] + dx, pose[2])
        Rs.append(R.reshape(4))
        ts.append(t)
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(Rs), np.array(ts), np.zeros((len(sizes), 3)))


@pytest.fixture(scope="module")
def world():
    return synth.make_map()


def far_share(world, batch, radius):
    m_ga, m_nga = world
    far = []
    for s in range(batch.n_scans):
        R, t = batch.R[s].reshape(2, 2), batch.t[s]
        ga, ng = batch.scan(s)
        far += [nn_dist(m_ga, ga @ R.T + t) >= radius, nn_dist(m_nga, ng @ R.T + t) >= radius]
    return np.concatenate(far).mean()


@pytest.mark.parametrize("pair,sizes", [(2, [127, 2600, 128, 1153, 129, 1081, 512, 1025, 513, 1024, 640, 641]),
                                        (1, [1023, 1088, 1024, 2049, 1025, 1087, 1089, 2047, 2048]),
                                        (-1, [1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049])])
def test_pass_boundaries_with_far_queries(world, pair, sizes):
    """sizes around the passes and rounds of a team of 512 and of 1024 lanes, partners of different pass counts, scans of the
    synthetic world half a metre off that the list form takes over after ONE iteration, while they are still settling"""
    batch = sized_batch(sizes, 0.36)   # 0.5 m off in all
    info = check(world[0], world[1], batch, 6, pair)
    share = far_share(world, batch, info["list_certified_radius"])
    after = far_share_after(world[0], world[1], batch, info["list_certified_radius"], 1)
    print("queries beyond the certified radius at the initial pose: %.2f, after the first iteration: %.2f" % (share, after))
    assert share > 0.9   # (what the ring form's first iteration sees; what the list form then sees is printed: these scans
                         # converge -- the case whose queries STAY far is test_every_query_of_every_pass_is_left_to_the_queue)


# ---------------------------------------------------------------------------------------------------- ties between two points
TIE_H = 1.0 / 64          # the two points of a pair lie at (k, +-TIE_H)
TIE_SIGN = [1, -1, -1, 1, 1, -1, -1, 1]   # which of a pair comes first in the model (the lowest index wins a tie): the sum of the
                                          # signs and of sign * x are zero, so the choices pull neither sideways nor round


def corridor():
    """A world mirrored in the x axis, every coordinate a small dyadic number: pairs of points at (8 + k, +-1/64), walls at
    y = +-1, caps at x = -1 and 33.  A query on the axis is at EXACTLY one float distance from the two points of a pair, and
    the registration keeps it there: the sums are mirrored, so the pose stays (tx, 0, 0) up to the last bits of a double,
    far below what moves a float distance."""
    m = []
    for k, sg in enumerate(TIE_SIGN):
        m += [(8.0 + k, sg * TIE_H), (8.0 + k, -sg * TIE_H)]
    for j in range(-8, 33 * 8 + 1):
        m += [(j / 8.0, 1.0), (j / 8.0, -1.0)]
    for i in range(-7, 8):
        m += [(-1.0, i / 8.0), (33.0, i / 8.0)]
    m_nga = np.array(m)
    m_ga = np.array([(40.0, 1.0), (40.0, -1.0), (41.0, 1.0), (41.0, -1.0), (42.0, 0.0)])   # a class no query belongs to
    q = [(8.0 + k + 1.0 / 16, 0.0) for k in range(len(TIE_SIGN))]                       # the tie queries come first: in the pass
    for j in range(-8, 33 * 8):
        q += [(j / 8.0 + 1.0 / 32, 1.0 - 1.0 / 32), (j / 8.0 + 1.0 / 32, -1.0 + 1.0 / 32)]
    for i in range(-7, 8):
        q += [(-1.0 + 1.0 / 32, i / 8.0), (33.0 - 1.0 / 32, i / 8.0)]
    q = np.array(q)
    R0, t0 = synth.pose_to_Rt(-1.0 / 64, 0.0, 0.0)   # off along the axis only
    batch = synth.ScanBatch(np.ascontiguousarray(np.concatenate([q, q])), np.array([0, len(q), 2 * len(q)], np.int32),
                            np.zeros(2, np.int32), np.array([R0.reshape(4)] * 2), np.array([t0] * 2), np.zeros((2, 3)))
    return m_ga, m_nga, batch


def f32_dist2(m, qx, qy):
    """fl(fl(dx * dx) + fl(dy * dy)) in float, as the searches compute it"""
    m = np.asarray(m, np.float32)
    dx, dy = m[:, 0] - np.float32(qx), m[:, 1] - np.float32(qy)
    return (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)


@pytest.mark.parametrize("pair", [2, -1])
@pytest.mark.parametrize("mode", ["p2p"])   # (point-to-line: the pairs' normals are not mirrored by the pairs' order, the pose leaves
def test_a_tie_between_two_different_points_goes_to_the_arbiter(mode, pair):   # the axis in its first step -- 0.1 mm -- and no tie is left)
    """queries at one float distance from two DIFFERENT model points, in every list-form iteration: the window must notice
    (second best == best) and leave them to the exact pass, whose choice -- the lowest index -- is the brute-force arbiter's.
    The pairs are ordered so that the arbiter takes the upper point of some and the lower point of others: a window that
    kept its own first or last find would move the pose, the sums and delta away from the arbiter's."""
    m_ga, m_nga, batch = corridor()
    p2l = mode == "p2l"
    first, max_iter = (2 if p2l else 1), 5
    model = O.IcpModel(m_ga, m_nga, normals_k=10) if p2l else O.IcpModel(m_ga, m_nga)
    arb = O.icp_params(max_iter, -1.0, 5.0, O.NN_BRUTE, O.MODE_P2L if p2l else O.MODE_P2P)
    q = batch.scan(0)[1]
    assert len(q) > 512 and len(q) - 512 <= 128 and len(q) > 256       # one pass of either team holds the tie queries
    # on the CPU: at every pose a list-form iteration starts from, each tie query is at ONE float distance from the two points
    # of its pair, nothing is nearer, and that distance is inside the certified radius (asserted below, once the handle says it)
    _, _, tr, steps = model.fit(np.zeros((0, 2)), q, batch.R[0], batch.t[0], arb)
    assert steps == max_iter
    tie_d = []
    model_all = np.concatenate([m_ga, m_nga]) if p2l else m_nga
    for it in range(first, max_iter):
        R, t = tr[it - 1, :4].reshape(2, 2), tr[it - 1, 4:6]                # the pose after iteration it - 1
        for k in range(len(TIE_SIGN)):
            w = R @ q[k] + t
            d = f32_dist2(model_all, np.float32(w[0]), np.float32(w[1]))
            best = np.flatnonzero(d == d.min())
            assert len(best) == 2 and model_all[best[0], 1] == -model_all[best[1], 1] != 0, (it, k, best)
            tie_d.append(float(np.sqrt(d.min())))
    # the arbiter's choice matters: the kd-tree, which takes another of the two, ends elsewhere
    kd = O.icp_params(max_iter, -1.0, 5.0, O.NN_KDTREE, O.MODE_P2L if p2l else O.MODE_P2P)
    Rb, tb, ib, nb, db = model.fit_batch(batch.pts, batch.scan_off, batch.scan_nga, batch.R, batch.t, arb)
    Rk, tk, _, _, dk = model.fit_batch(batch.pts, batch.scan_off, batch.scan_nga, batch.R, batch.t, kd)
    print("arbiter against kd-tree: |dt| %.3g |ddelta| %.3g" % (np.abs(tb - tk).max(), np.abs(db - dk).max()))
    assert np.abs(tb - tk).max() > 2 * POS_TOL   # (0.35 mm)
    kw = dict(mode=api.ICP_P2L, normals_k=10) if p2l else {}
    icp = api.Icp(m_ga, m_nga, max_iter=max_iter, min_delta=-1.0, pair_scans=pair, spread_scans=-1, first_iterations=first,
                  far_div=1, **kw)
    info = icp.index_info()
    R, t, res, trace = icp.fit_batch(batch, trace=True)
    icp.close()
    assert info["two_forms"] and info["first_iterations"] == first
    assert max(tie_d) < info["list_certified_radius"]
    assert np.array_equal(res["iters"], ib) and np.array_equal(res["n_corr"], nb)
    assert np.abs(t - tb).max() < POS_TOL and ang_diff(yaw(R), yaw(Rb)).max() < ANG_TOL
    assert np.abs(res["delta"] - db).max() < 1e-9
    for s in range(2):                                                     # every step's pose and delta, not the last alone
        assert np.abs(trace[s, :max_iter, :7] - tr[:, :7]).max() < 1e-7, s


# ---------------------------------------------------------------------------------------------------- every query in the queue
def lattice_world():
    """Model points on two square lattices of 1 m (class GA: 40 x 30 from (0, 0); class NGA: 60 x 50 from (0.5, 100.5))."""
    ga = np.stack(np.meshgrid(np.arange(40.0), np.arange(30.0)), -1).reshape(-1, 2)
    ng = np.stack(np.meshgrid(np.arange(60.0), np.arange(50.0)), -1).reshape(-1, 2) + [0.5, 100.5]
    return ga, ng


def far_batch(sizes):
    """Scans whose every point lies 0.45 m from a lattice point of its class, a quarter of them to each side: each is pulled
    0.45 m, all together nowhere, so the registration stays where it starts and every query stays 0.45 m from the map in
    every iteration."""
    ga, ng = lattice_world()
    off4 = np.array([(0.45, 0.0), (-0.45, 0.0), (0.0, 0.45), (0.0, -0.45)])
    pts, off, nga, Rs, ts = [], [0], [], [], []
    for s, n in enumerate(sizes):
        rs = np.random.RandomState(700 + s)
        n_ga = 4 * min(n // 8, len(ga) // 4)
        n_ng = n - n_ga
        assert n_ng <= len(ng)
        for m, k in ((ga, n_ga), (ng, n_ng)):
            pick = m[rs.permutation(len(m))[:k]]
            pts.append(pick + off4[np.arange(k) % 4])
        off.append(off[-1] + n)
        nga.append(n_ga)
        R, t = synth.pose_to_Rt(0.0, 0.0, 0.0)
        Rs.append(R.reshape(4))
        ts.append(t)
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(Rs), np.array(ts), np.zeros((len(sizes), 3)))


def far_share_after(m_ga, m_nga, batch, radius, iters):
    """the share of queries farther than `radius` from the map at the pose the oracle reaches after `iters` iterations"""
    model = O.IcpModel(m_ga, m_nga)
    R, t, _, _, _ = model.fit_batch(batch.pts, batch.scan_off, batch.scan_nga, batch.R, batch.t, O.icp_params(iters, -1.0, 5.0))
    posed = synth.ScanBatch(batch.pts, batch.scan_off, batch.scan_nga, R, t, None)
    return far_share((m_ga, m_nga), posed, radius)


@pytest.mark.parametrize("pair,sizes", [(2, [1081, 1079]),
                                        (2, [127, 2600, 128, 1153, 129, 1081, 512, 1025, 513, 1024, 640, 641]),
                                        (1, [1024, 1088, 2048]), (-1, [1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049])])
def test_every_query_of_every_pass_is_left_to_the_queue(pair, sizes):
    """EVERY query beyond the certified radius in every list-form iteration -- asserted on the CPU at the poses the oracle
    reaches after 1 and after 3 iterations: every lane of every pass has a query for its wavefront's region of the queue, the
    regions fill in the first pass, and the second pass's queries find them full.  First the one workgroup of two scans of
    two passes and a tail each, then the sizes around the boundaries of the passes and rounds."""
    m_ga, m_nga = lattice_world()
    batch = far_batch(sizes)
    info = check(m_ga, m_nga, batch, 5, pair)
    for iters in (1, 3):
        share = far_share_after(m_ga, m_nga, batch, info["list_certified_radius"], iters)
        print("queries beyond the certified radius after %d iterations: %.3f" % (iters, share))
        assert share == 1.0
