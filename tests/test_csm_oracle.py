"""The correlative scan matcher's scalar restatement (tests/cpp/csm_oracle.cpp) on its own: tables worked by hand, the
properties the pruned search rests on, and the reason the matcher exists -- scans that ICP alone loses and that the
matcher's candidate brings back to the noise floor.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import csm_cases as K
import csm_oracle as CO
import oracle_lib as O
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stamp(K_, res, sigma):
    i = np.arange(-K_, K_ + 1)
    d2 = (i[None, :] ** 2 + i[:, None] ** 2).astype(np.float64)
    return np.rint(255.0 * np.exp(-(d2 * (res * res)) / (2.0 * (sigma * sigma)))).astype(np.uint8)


# ------------------------------------------------------------------ hand-worked tables
def test_default_kernel_is_six_cells():
    # 3 * 0.2 / 0.1 is 6.000000000000001 in doubles: the contract's ceil(3 sigma / resolution - 1e-9) is 6, not 7
    om = CO.OracleMatcher(np.zeros((0, 2)), K.centre(np.arange(5), np.zeros(5)))
    assert om.params.kernel_cells == 6
    assert om.table(1)[2].shape == (13, 5 + 12)


def test_four_collinear_points_stamp_four_times():
    res, sigma, Kc = 0.1, 0.2, 2
    cells = [(-3, 1), (-1, 1), (0, 1), (4, 1)]          # gaps of 2, 1 and 4 cells: overlapping, adjacent and disjoint copies
    m = K.centre([c[0] for c in cells], [c[1] for c in cells])
    om = CO.OracleMatcher(np.zeros((0, 2)), m, resolution=res, sigma=sigma, kernel_cells=Kc, block=2)
    ox, oy, T = om.table(1)
    assert (ox, oy, T.shape) == (-3 - Kc, 1 - Kc, (2 * Kc + 1, 4 + 3 + 1 + 2 * Kc))
    st = stamp(Kc, res, sigma)
    assert st[Kc, Kc] == 255 and st[0, 0] == round(255 * np.exp(-8 * 0.01 / 0.08))
    want = np.zeros_like(T)
    for cx, cy in cells:
        x0, y0 = cx - Kc - ox, cy - Kc - oy
        want[y0:y0 + 2 * Kc + 1, x0:x0 + 2 * Kc + 1] = np.maximum(want[y0:y0 + 2 * Kc + 1, x0:x0 + 2 * Kc + 1], st)
    assert np.array_equal(T, want)
    assert (T == 255).sum() == 4
    # the empty class has no table at either level
    assert om.table(0)[2].shape == (0, 0) and om.table(0, 1)[2].shape == (0, 0)
    # the order of the points does not show
    om2 = CO.OracleMatcher(np.zeros((0, 2)), m[::-1].copy(), resolution=res, sigma=sigma, kernel_cells=Kc, block=2)
    assert np.array_equal(om2.table(1)[2], T)


def test_cell_is_floor_not_truncation():
    # x = -0.05 lies in cell -1 (truncation would say 0); x = 0.5 is exactly on an edge (0.5 / 0.1 = 5.0): cell 5; x = 0.3 is
    # 2.9999999999999996 cells: cell 2; y = -0.2 is exactly -2.0 cells: cell -2
    m = np.array([[-0.05, -0.2], [0.5, -0.2], [0.3, -0.2], [0.05, -0.2]])
    om = CO.OracleMatcher(np.zeros((0, 2)), m, kernel_cells=1, sigma=0.05, block=2)
    ox, oy, T = om.table(1)
    assert (ox, oy) == (-2, -3) and T.shape == (3, 5 - (-1) + 1 + 2)
    assert [int(c) + ox for c in np.nonzero(T[1] == 255)[0]] == [-1, 0, 2, 5]


def test_three_points_make_no_table():
    m3 = K.centre([0, 1, 2], [0, 0, 0])
    m4 = K.centre([0, 1, 2, 3], [0, 0, 0, 0])
    om = CO.OracleMatcher(m3, m4, kernel_cells=1, block=2)
    assert om.table(0)[2].shape == (0, 0) and om.table(1)[2].shape == (3, 6)
    # ... and its scan points score nothing and are not counted
    ga, nga = K.centre([0, 1, 2], [0, 0, 0]), K.centre([0, 1, 2, 3], [0, 0, 0, 0])
    om.set_window(2, 2, 0, 0.01)
    vol, cnt = om.volume(ga, nga, np.eye(2), np.zeros(2), counted=True)
    assert cnt[0] == 4 and vol[0, 2, 2] == 4 * 255
    R, t, res = om.match(ga, nga, np.eye(2), np.zeros(2))
    assert CO.result_tuple(res) == (0, 2, 2, 1020, 4, 1020)


# ------------------------------------------------------------------ properties
@pytest.fixture(scope="module")
def box():
    return K.box_model()


def sliding_max(T, D):
    h, w = T.shape
    P = np.zeros((h + 2 * (D - 1), w + 2 * (D - 1)), np.uint8)
    P[D - 1:D - 1 + h, D - 1:D - 1 + w] = T
    W = np.zeros((h + D - 1, w + D - 1), np.uint8)
    for j in range(D):
        for i in range(D):
            W = np.maximum(W, P[j:j + h + D - 1, i:i + w + D - 1])
    return W


@pytest.mark.parametrize("D,Kc", [(2, 1), (8, 6), (3, 2)])
def test_bound_table_is_the_sliding_maximum(box, D, Kc):
    om = CO.OracleMatcher(box[0], box[1], kernel_cells=Kc, block=D)
    for c in (0, 1):
        ox, oy, T = om.table(c)
        wx, wy, W = om.table(c, 1)
        assert (wx, wy) == (ox - (D - 1), oy - (D - 1)) and W.shape == (T.shape[0] + D - 1, T.shape[1] + D - 1)
        assert np.array_equal(W, sliding_max(T, D))
        assert (W[D - 1:, D - 1:] >= T).all()            # W >= T on every block: W[u, v] covers T[u .. u + D, v .. v + D]


def block_max(vol, D):
    n_th, n_y, n_x = vol.shape
    by, bx = (n_y + D - 1) // D, (n_x + D - 1) // D
    P = np.full((n_th, by * D, bx * D), -1, np.int64)
    P[:, :n_y, :n_x] = vol
    return P.reshape(n_th, by, D, bx, D).max(axis=(2, 4))


def test_bound_covers_every_candidate_of_its_block(box):
    rs = np.random.RandomState(5)
    for trial in range(12):
        D, Kc = [(8, 6), (2, 1), (5, 3)][trial % 3]
        om = CO.OracleMatcher(box[0], box[1], kernel_cells=Kc, block=D)
        om.set_window(int(rs.randint(0, 12)), int(rs.randint(0, 12)), int(rs.randint(0, 4)), 0.02)
        ga, nga = K.scan_of(box, int(rs.randint(5, 200)), K.TRUE_POSE, 400 + trial)
        R0, t0 = K.pose_Rt(*(np.array(K.TRUE_POSE) + rs.uniform(-0.5, 0.5, 3) * (1, 1, 0.1)))
        vol, U = om.volume(ga, nga, R0, t0), om.bounds(ga, nga, R0, t0)
        assert (U >= block_max(vol, D)).all()


def check_two_level(om, ga, nga, R0, t0):
    """two-level == exhaustive == the volume's first maximum; returns the result"""
    vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
    flat = int(np.argmax(vol))                           # numpy: the first of equal maxima
    k, b, a = np.unravel_index(flat, vol.shape)
    want = (int(k), int(a), int(b), int(vol.max()), int(cnt[k]), 255 * int(cnt[k]))
    R1, t1, r1 = om.match(ga, nga, R0, t0)
    R2, t2, r2 = om.match(ga, nga, R0, t0, exhaustive=True)
    assert CO.result_tuple(r1) == want and CO.result_tuple(r2) == want
    assert np.array_equal(R1, R2) and np.array_equal(t1, t2)
    assert r2.blocks_evaluated == int(np.prod(om.block_dims)) and 1 <= r1.blocks_evaluated <= r2.blocks_evaluated
    cs = om.angles(R0)[k]
    assert np.array_equal(R1, np.array([[cs[0], -cs[1]], [cs[1], cs[0]]]))
    P = om.params
    assert t1[0] == t0[0] + float(a - P.half_x) * P.resolution and t1[1] == t0[1] + float(b - P.half_y) * P.resolution
    return r1


def test_two_level_equals_exhaustive(box):
    om = CO.OracleMatcher(box[0], box[1])
    pruned = []
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        r = check_two_level(om, ga, nga, R0, t0)
        pruned.append((name, r.blocks_evaluated, int(np.prod(om.block_dims))))
        if name == "all_outside":
            assert CO.result_tuple(r)[:4] == (0, 0, 0, 0)    # an all-zero volume answers index 0 with score 0 ...
            assert r.blocks_evaluated == int(np.prod(om.block_dims))   # ... and nothing can be pruned
    print(pruned)


def test_exact_tie_takes_the_lowest_flat_index():
    kw, m_ga, m_nga, ga, nga, R0, t0, winner, other, score = K.tie_case()
    om = CO.OracleMatcher(m_ga, m_nga, **kw)
    vol, U = om.volume(ga, nga, R0, t0), om.bounds(ga, nga, R0, t0)
    # what the case is built for: two maxima, in two blocks whose bounds both EQUAL the maximum
    assert vol.max() == score and sorted(zip(*np.nonzero(vol == score))) == sorted([(winner[0], winner[2], winner[1]), (other[0], other[2], other[1])])
    assert U[0, 0, 0] == score and U[0, 0, 1] == score and U.max() == score
    r = check_two_level(om, ga, nga, R0, t0)
    assert (r.k, r.a, r.b, r.score) == (*winner, score)


def test_short_scan_is_left_alone(box):
    om = CO.OracleMatcher(box[0], box[1])
    ga, nga = K.scan_of(box, 4, K.TRUE_POSE, 1)
    R0, t0 = K.pose_Rt(1.0, 2.0, 0.5)
    R, t, r = om.match(ga, nga, R0, t0)
    assert r.score == -1 and np.array_equal(R, R0) and np.array_equal(t, t0)


# ------------------------------------------------------------------ the basin
@pytest.fixture(scope="module")
def basin():
    m_ga, m_nga = CO.synth_map()
    return CO.OracleMatcher(m_ga, m_nga), O.IcpModel(m_ga, m_nga), O.icp_params(max_iter=100, indist=5.0)


EXHAUSTIVE_KS = (0, 128)    # the full 241 x 81 x 81 volume, five seconds each: the two-level form pinned at full size


@pytest.mark.parametrize("k", CO.BASIN_KS)
def test_matcher_recovers_what_icp_loses(basin, k):
    om, icp, P = basin
    ga, nga, pose, R0, t0 = CO.basin_case(k)
    # the precondition: ICP alone, 100 iterations from truth + (3.0, -3.0, 1.0), ends far from the truth
    R, t, _, _ = icp.fit(ga, nga, R0, t0, P)
    lost = CO.pose_error(R, t, pose)
    assert lost[0] > 1.0 or lost[1] > 0.5, lost
    Rm, tm, res = om.match(ga, nga, R0, t0)
    if k in EXHAUSTIVE_KS:
        Re, te, rex = om.match(ga, nga, R0, t0, exhaustive=True)
        assert CO.result_tuple(rex) == CO.result_tuple(res) and np.array_equal(Re, Rm) and np.array_equal(te, tm)
    # within 2 cells and 1 angular step of the truth (the quantisation alone allows resolution / sqrt 2 and half a step)
    em = CO.pose_error(Rm, tm, pose)
    assert em[0] <= 2 * om.params.resolution and em[1] <= om.params.theta_step + 1e-12, em
    R2, t2, _, _ = icp.fit(ga, nga, Rm, tm, P)
    e2 = CO.pose_error(R2, t2, pose)
    n_blocks = int(np.prod(om.block_dims))
    print("scan %d: ICP alone %.2f m %.2f rad; candidate %s, %d of %d blocks; ICP from it %.2f mm %.3f mrad" %
          (k, lost[0], lost[1], CO.result_tuple(res)[:4], res.blocks_evaluated, n_blocks, 1e3 * e2[0], 1e3 * e2[1]))
    assert e2[0] < 0.01 and e2[1] < 1e-3, e2
    assert res.blocks_evaluated < n_blocks // 100


# ------------------------------------------------------------------ the ctypes mirrors
def test_csm_structs_mirror_the_header(tmp_path):
    structs = {"slam_csm_params": api.CsmParams, "slam_csm_result": api.CsmResult}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (f, name, f))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert len(out.strip().splitlines()) == 2
    for line in out.strip().splitlines():
        parts = line.split()
        cls = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), (parts[0], parts[1], C.sizeof(cls))
        assert len(parts) - 2 == len(cls._fields_)
        for p in parts[2:]:
            f, off = p.split("=")
            assert getattr(cls, f).offset == int(off), (parts[0], f, off, getattr(cls, f).offset)
    assert api.CSM_RESULT_DTYPE.itemsize == C.sizeof(api.CsmResult)


def test_defaults_are_the_issue_values():
    from slam_amd import build
    build.build()
    for p in (api.csm_default_params(), CO.default_params()):
        assert (p.resolution, p.sigma, p.kernel_cells, p.block, p.half_x, p.half_y, p.half_theta, p.theta_step, p.exhaustive) == \
            (0.1, 0.2, 0, 8, 40, 40, 120, 0.01, 0)
