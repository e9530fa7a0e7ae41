"""The ring searches of the batch kernels read, per lattice row, only the cells under the chord of the disk of the best so
far, probe a level entered without a candidate before reading it, and read a seeded query's larger-than-3x3 disk in one pass
(icp_search.hpp: row_chord, probe_level, nn_search_impl, nn_search_seeded_impl).  Pruning must never change the neighbour:
distance and index against the brute-force arbiter bit for bit, ties to the lowest original index, registrations against the
CPU oracle -- and every case first proves, on the host, that its inputs reach the pruning code (ring_restatement.py)."""
import numpy as np
import pytest

import oracle_lib as O
import ring_restatement as RR
from slam_amd import api
from test_gpu_icp_pair import ANG_TOL, POS_TOL, ang_diff, check, yaw

pytestmark = pytest.mark.gpu
CELL = 0.25   # dyadic pitch, lattice origin at (0, 0): rows and columns lie on multiples of 0.25


def wall(x0, y0, x1, y1, n):
    t = np.linspace(0.0, 1.0, n)[:, None]
    return np.array([[x0, y0]]) + t * np.array([[x1 - x0, y1 - y0]])


def nearest_model():
    """~2000 points, both classes: walls ON row / column boundaries (y = 3, x = 5, ...: multiples of the pitch, dyadic point
    spacing), walls inside cells, empty rows between them, one lone point in an otherwise empty corner region."""
    ga = np.concatenate([
        wall(0.0, 0.0, 12.0, 0.0, 193),         # y = 0: the lattice's first row boundary, spacing 1/16
        wall(2.0, 3.0, 10.0, 3.0, 257),         # on a row boundary, spacing 1/32
        wall(5.0, 4.0, 5.0, 9.0, 161),          # on a column boundary
        wall(1.1, 7.6, 4.3, 7.6, 200),          # inside cells
        wall(13.13, 0.4, 13.13, 6.2, 190),      # inside cells, a column
        np.array([[15.5, 11.5]]),               # the lone point of the far corner
    ])
    nga = np.concatenate([
        wall(0.0, 0.0, 0.0, 9.0, 145),          # x = 0: the first column boundary
        wall(7.0, 5.5, 11.0, 5.5, 129),         # on a row boundary (22 * 0.25)
        wall(9.25, 6.0, 9.25, 10.0, 129),       # on a column boundary (37 * 0.25)
        wall(2.03, 1.37, 8.9, 2.11, 300),       # oblique, inside cells
        wall(11.4, 7.7, 14.2, 9.9, 260),
        np.array([[15.75, 0.125], [15.5, 11.75]]),   # lone points: an empty corner each
    ])
    return ga, nga


def nearest_queries(xy, rs):
    """~4000 queries of one class: off the walls by 0.05-3 m, outside the lattice on every side, fx or fy an exact integer,
    nearest distance an exact multiple of the pitch (the disk tangent to a row edge), nearest point the first or last of a
    row span."""
    xy = xy.astype(np.float32)
    n = len(xy)
    q = []
    ang = rs.uniform(0, 2 * np.pi, 1500)
    q.append(xy[rs.randint(0, n, 1500)] + (rs.uniform(0.05, 3.0, 1500) * np.array([np.cos(ang), np.sin(ang)])).T)
    out = rs.uniform(0.01, 3.0, (800, 1))                                  # outside the lattice, every side
    side = np.array([[-1, 0], [1, 0], [0, -1], [0, 1]])[rs.randint(0, 4, 800)]
    inside = np.stack([rs.uniform(-1, 17, 800), rs.uniform(-1, 13, 800)], 1)
    edge = np.where(side == 0, inside, np.where(side < 0, 0.0, np.array([[15.75, 11.75]]))) + side * out
    q.append(edge)
    g = np.stack([rs.randint(0, 64, 600) * CELL, rs.uniform(0, 12, 600)], 1)   # fx an exact integer
    q.append(g)
    q.append(g[:, ::-1] * np.array([[1.0, 1.0]]))                          # fy an exact integer (x up to 12, y a multiple)
    k = rs.randint(1, 9, 500)[:, None] * CELL                              # straight off a wall point by k pitches: disk tangent
    axis = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]])[rs.randint(0, 4, 500)]  # to a row (column) edge when the wall is on one
    q.append(xy[rs.randint(0, n, 500)] + axis * k)
    ends = np.array([xy[np.argmin(xy @ d)] for d in ([1, 0], [-1, 0], [0, 1], [0, -1], [1, 1], [-1, -1], [1, -1], [-1, 1])])
    q.append(ends[rs.randint(0, len(ends), 300)] + rs.uniform(-1.5, 1.5, (300, 2)))   # around the walls' end points
    return np.concatenate(q).astype(np.float32)


@pytest.fixture(scope="module")
def nearest_world():
    """model, queries and the arbiter's answers, computed once for all lanes / force_global variants"""
    m_ga, m_nga = nearest_model()
    rs = np.random.RandomState(808)
    per_cls = []
    for model in (m_ga, m_nga):
        xy = model.astype(np.float32)
        q = nearest_queries(model, rs)
        ref = np.array([O.brute_nn1(xy, a, b) for a, b in q])
        per_cls.append((xy, q, ref[:, 0].astype(np.float32), ref[:, 1].astype(np.int32)))
    return m_ga, m_nga, per_cls


def reach_counts_unseeded(info, all_xy, xy, q, every=8):
    """what the unseeded search does with (a sample of) the queries: levels probed, rows clipped by their chord"""
    L = RR.Lattice(info, all_xy)
    ix = RR.CellIndex(L, xy)
    count = {}
    for k in range(0, len(q), every):
        RR.unseeded(ix, q[k], count=count)
    return count


@pytest.mark.parametrize("lanes", [1, 4, 8, 16, 64])
@pytest.mark.parametrize("force_global", [0, 1])
def test_unseeded_nearest_is_bit_exact_under_chords_and_probe(nearest_world, lanes, force_global):
    m_ga, m_nga, per_cls = nearest_world
    icp = api.Icp(m_ga, m_nga, lanes_per_point=lanes, force_global=force_global, cell_size=CELL)
    info = icp.index_info()
    assert info["in_lds"] == (not force_global) and info["cell"] == CELL
    all_xy = np.concatenate([m_ga, m_nga])
    for cls, (xy, q, ref_d, ref_i) in enumerate(per_cls):
        count = reach_counts_unseeded(info, all_xy, xy, q)
        assert count.get("probed", 0) > 0 and count.get("clipped", 0) > 0, count   # the inputs reach the new code
        dis, idx = icp.nearest(cls, q)
        bad = np.nonzero((dis != ref_d) | (idx != ref_i))[0]
        assert len(bad) == 0, (cls, len(bad), q[bad[:5]], dis[bad[:5]], ref_d[bad[:5]], idx[bad[:5]], ref_i[bad[:5]])
    icp.close()


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("orient", ["row", "column"])
def test_tie_at_the_end_of_a_chord_goes_to_the_lower_index(cls, orient):
    """Dyadic 3-4-5: the query is 1.25 m (five cells) from A and from B, the same float; A has the lower original index and
    lies in the LAST cell of its row's chord, the disk's edge passing through that cell.
    row:    A = q + (1, 0.75) in row 19, whose chord ends in column 20, A's; B = q + (0, 1.25), two rows farther, in the next
            ring level.  Level 4 is entered without a candidate and probed (A is what the probe finds) and read under A's
            disk; level 8, under the same disk, finds B: a tie, and the exact pass must still read A's cell.
    column: A = q + (1.25, 0) in the query's own row, ON the disk's edge in the last cell of that row's chord (column 21, in
            level 8); B = q + (0.75, 1) in row 20 is what level 4's probe and scan find first."""
    qp = np.array([4.125, 4.125])
    A, B = (qp + [1.0, 0.75], qp + [0.0, 1.25]) if orient == "row" else (qp + [1.25, 0.0], qp + [0.75, 1.0])
    far = np.array([[0.0, 0.0], [8.0, 8.0], [0.0, 8.0], [8.0, 0.0], [7.5, 0.5]])    # the lattice's corners; farther than 1.25 m
    pts = np.concatenate([[A], far, [B]])
    m_ga, m_nga = (pts, far) if cls == 0 else (far, pts)
    icp = api.Icp(m_ga, m_nga, cell_size=CELL)
    info = icp.index_info()
    xy = pts.astype(np.float32)
    q = qp.astype(np.float32)[None, :]
    d_ref, i_ref = O.brute_nn1(xy, q[0, 0], q[0, 1])
    assert i_ref == 0 and d_ref == np.float32(1.5625)
    assert ((xy[[0, -1]] - q) ** 2).sum(1).tolist() == [1.5625, 1.5625]
    L = RR.Lattice(info, np.concatenate([m_ga, m_nga]))
    ix = RR.CellIndex(L, xy)
    count = {}
    RR.unseeded(ix, q[0], count=count)
    assert count.get("probed", 0) > 0 and count.get("clipped", 0) > 0, count
    fx, fy = (float(v) for v in L.frac(q[0]))
    row_a, col_a = int(A[1] / CELL), int(A[0] / CELL)
    assert RR.chord(fx, fy, row_a, (1.25 + float(L.margin)) / CELL, 0, L.nx - 1)[1] == col_a   # A's cell ends its row's chord
    dis, idx = icp.nearest(cls, q)
    assert dis[0] == np.float32(d_ref) and idx[0] == i_ref
    icp.close()


# ---- the seeded path and the probe inside the batch kernels -----------------------------------------------------------------
def room_model(rs):
    """~2000 points of an axis-aligned room with two inner walls, N(0, 0.01^2) noise per coordinate (no exact ties)"""
    segs = [(-8, -6, 8, -6), (8, -6, 8, 6), (8, 6, -8, 6), (-8, 6, -8, -6), (-3, -6, -3, -1), (2, 1.5, 6, 1.5)]
    ga_segs, nga_segs = segs[:3] + segs[4:5], segs[3:4] + segs[5:]
    out = []
    for ss in (ga_segs, nga_segs):
        ln = np.array([abs(c - a) + abs(d - b) for a, b, c, d in ss])
        pts = [wall(a, b, c, d, int(round(1000 * l / ln.sum()))) for (a, b, c, d), l in zip(ss, ln)]
        out.append(np.concatenate(pts) + rs.normal(0.0, 0.01, (sum(len(p) for p in pts), 2)))
    return out[0], out[1]


def room_batch(m_ga, m_nga, sizes, rs):
    """scans = samples of the room's walls seen from a pose, with initial errors of 0.3-1.5 m and 0.03-0.06 rad"""
    from slam_amd import synth
    pts, off, nga, Rs, ts, poses = [], [0], [], [], [], []
    for k, n in enumerate(sizes):
        x, y, th = rs.uniform(-2, 2), rs.uniform(-2, 2), rs.uniform(-np.pi, np.pi)
        R, t = synth.pose_to_Rt(x, y, th)
        n_ga = int(n * len(m_ga) / (len(m_ga) + len(m_nga)))
        sel = [m[rs.choice(len(m), c, replace=False)] + rs.normal(0.0, 0.01, (c, 2)) for m, c in ((m_ga, n_ga), (m_nga, n - n_ga))]
        for w in sel:
            pts.append((w - t) @ R)               # world -> sensor frame
        off.append(off[-1] + n)
        nga.append(n_ga)
        a = rs.uniform(0, 2 * np.pi)
        e_xy = rs.uniform(0.3, 1.5) * np.array([np.cos(a), np.sin(a)])
        e_th = rs.uniform(0.03, 0.06) * rs.choice([-1.0, 1.0])
        R0, t0 = synth.pose_to_Rt(x + e_xy[0], y + e_xy[1], th + e_th)
        Rs.append(R0.reshape(4))
        ts.append(t0)
        poses.append((x, y, th))
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(Rs), np.array(ts), np.array(poses))


@pytest.fixture(scope="module")
def room():
    rs = np.random.RandomState(4242)
    m_ga, m_nga = room_model(rs)
    batches = {ns: room_batch(m_ga, m_nga, [300, 1081, 1081, 300][:ns], np.random.RandomState(100 + ns)) for ns in (2, 3, 4)}
    return m_ga, m_nga, {0: O.IcpModel(m_ga, m_nga), 1: O.IcpModel(m_ga, m_nga, normals_k=10)}, batches


MAX_ITER = 4


def reach_counts_fit(info, m_ga, m_nga, model, batch, p2l):
    """From the oracle's pose trace: seeded queries whose disk exceeds 3 x 3 cells, rows clipped by their chord, levels probed
    (iteration 0 is unseeded; later iterations are seeded with the neighbour of the iteration before)."""
    all_xy = np.concatenate([m_ga, m_nga])
    L = RR.Lattice(info, all_xy)
    idx = [RR.CellIndex(L, all_xy)] if p2l else [RR.CellIndex(L, m_ga), RR.CellIndex(L, m_nga)]
    prm = O.icp_params(MAX_ITER, -1.0, 5.0, O.NN_KDTREE, O.MODE_P2L if p2l else O.MODE_P2P)
    un, se = {}, {}
    for s in range(batch.n_scans):
        ga, nga = batch.scan(s)
        _, _, tr, steps = model.fit(ga, nga, batch.R[s], batch.t[s], prm)
        poses = [(batch.R[s].reshape(2, 2), batch.t[s])] + [(tr[k, :4].reshape(2, 2), tr[k, 4:6]) for k in range(steps - 1)]
        for pts, ix in ((np.concatenate([ga, nga]), idx[0]),) if p2l else ((ga, idx[0]), (nga, idx[1])):
            pts = pts[::5]
            prev = None
            for it, (Rk, tk) in enumerate(poses[:2]):
                q = (pts @ Rk.T + tk).astype(np.float32)
                if prev is None:
                    for v in q:
                        RR.unseeded(ix, v, gate=np.inf if p2l else 25.0, count=un)
                else:
                    for v, sd in zip(q, prev):
                        RR.seeded(ix, v, sd, gate=np.inf if p2l else 25.0, count=se)
                prev = ix.nearest(q)
    return un, se


def check_p2l(room, batch, pair):
    """test_gpu_icp_pair.check for the point-to-line step: the oracle with the reference's kd-tree, the brute-force arbiter for a
    scan that met an exact distance tie (the kd-tree takes the candidate it visits last, the device the lowest index)"""
    m_ga, m_nga, models, _ = room
    icp = api.Icp(m_ga, m_nga, mode=api.ICP_P2L, normals_k=10, max_iter=MAX_ITER, min_delta=-1.0, pair_scans=pair, spread_scans=-1)
    R, t, res, _ = icp.fit_batch(batch)
    R2, t2, res2, _ = icp.fit_batch(batch)
    icp.close()
    assert np.array_equal(R, R2) and np.array_equal(t, t2) and np.array_equal(res["n_corr"], res2["n_corr"])
    model = models[1]
    for s in range(batch.n_scans):
        ga, nga = batch.scan(s)
        ok = False
        for nn in (O.NN_KDTREE, O.NN_BRUTE):
            Ro, to, tr, steps = model.fit(ga, nga, batch.R[s], batch.t[s], O.icp_params(MAX_ITER, -1.0, 5.0, nn, O.MODE_P2L))
            ok = np.abs(t[s] - to).max() < POS_TOL and ang_diff(yaw(R[s]), yaw(Ro)).max() < ANG_TOL
            if ok:
                break
        assert ok and steps == res["iters"][s] == MAX_ITER and res["n_corr"][s] == len(ga) + len(nga), s


@pytest.mark.parametrize("p2l", [0, 1])
@pytest.mark.parametrize("pair", [1, 2])
@pytest.mark.parametrize("n_scans", [2, 3, 4])
def test_seeded_one_pass_and_probe_match_the_oracle(room, n_scans, pair, p2l):
    m_ga, m_nga, models, batches = room
    batch = batches[n_scans]
    kw = dict(mode=api.ICP_P2L, normals_k=10) if p2l else {}
    icp = api.Icp(m_ga, m_nga, max_iter=MAX_ITER, min_delta=-1.0, pair_scans=pair, spread_scans=-1, **kw)
    info = icp.index_info()
    icp.close()
    un, se = reach_counts_fit(info, m_ga, m_nga, models[p2l], batch, p2l)
    print("unseeded", un, "seeded", se)
    assert se.get("big", 0) > 0 and se.get("onepass", 0) > 0, se          # seed disks beyond 3 x 3 cells, read in one pass
    assert un.get("clipped", 0) > 0 and se.get("clipped", 0) > 0, (un, se)  # rows whose chord drops a cell of the square
    assert un.get("probed", 0) > 0, un                                       # levels of radius >= 2 entered without a candidate
    if p2l:
        check_p2l(room, batch, pair)
    else:
        check((m_ga, m_nga, models[0]), batch, MAX_ITER, -1.0, pair, certify=True)   # ... and every step to the brute-force step
