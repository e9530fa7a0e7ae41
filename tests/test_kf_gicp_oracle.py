"""The restatement of the store's Generalized ICP (tests/cpp/kf_gicp_oracle.cpp) held to things worked by hand: the
neighbour lists' order, C' on planes, lines and sparse points, the Jacobian against finite differences, an exact rigid copy,
every stop state, the scene plane-to-plane exists for, the struct mirrors and the share of identity covariances on the
keyframes the device tests use.  No device is needed.  docs/KF_GICP.md section 5 lists the bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kf_edge_oracle as K
import kf_gicp_cases as G
import kf_gicp_oracle as O
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


def numpy_lists(xyz, k, radius):
    """(index, f32 d^2, count) by numpy: candidates within the radius, sorted by (d^2, index)."""
    p = np.ascontiguousarray(xyz[:, :3], np.float32)
    d = p[:, None, :] - p[None, :, :]
    d = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d.dtype == np.float32
    n = len(p)
    idx, d2, cnt = np.full((n, k), -1, np.int32), np.zeros((n, k), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        cand = np.nonzero(d[i].astype(np.float64) <= radius * radius)[0]
        order = cand[np.lexsort((cand, d[i][cand]))][:k]
        idx[i, :len(order)], d2[i, :len(order)], cnt[i] = order, d[i][order], len(order)
    return idx, d2, cnt


def test_neighbour_lists_follow_distance_then_index():
    xyz = G.lattice_cloud(200, 3)
    gp = O.default_gicp(k_correspondences=20, cov_radius=0.4)
    c = O.OracleCloud(xyz, gp=gp)
    idx, d2, cnt = numpy_lists(xyz, 20, 0.4)
    ties = sum(int((np.diff(d2[i, :cnt[i]]) == 0).sum()) for i in range(len(xyz)))
    print("equal neighbouring distances in the lists: %d; list lengths %d..%d" % (ties, cnt.min(), cnt.max()))
    assert ties > 200 and cnt.max() == 20 and cnt.min() < 20
    assert np.array_equal(c.index, idx) and np.array_equal(c.dist2.view(np.uint32), d2.view(np.uint32)) and np.array_equal(c.count, cnt)
    assert np.all(c.index[:, 0] == np.arange(len(xyz))) and np.all(c.dist2[:, 0] == 0)   # the point itself comes first


def plane_patch():
    g = G.grid(0.25 * np.arange(9), 0.25 * np.arange(9))
    return np.stack([g[:, 0], g[:, 1], np.zeros(len(g))], 1).astype(np.float32)


def test_plane_patch_gives_exactly_diag_1_1_eps():
    c = O.OracleCloud(plane_patch(), gp=O.default_gicp(cov_radius=0.75))
    assert c.count.min() >= 4
    assert np.array_equal(c.cov, np.tile([1.0, 0, 0, 1.0, 0, EPS], (len(c.cov), 1)))


def test_patch_turned_about_x_puts_eps_on_y():
    p = plane_patch()
    turned = np.stack([p[:, 0], -p[:, 2], p[:, 1]], 1).astype(np.float32)    # a quarter turn about x: z <- y, y <- -z
    c = O.OracleCloud(turned, gp=O.default_gicp(cov_radius=0.75))
    assert np.array_equal(c.cov, np.tile([1.0, 0, 0, EPS, 0, 1.0], (len(c.cov), 1)))


def test_line_of_points():
    d = np.array([2.0, 1.0, 2.0]) / 3.0
    line = (np.arange(40)[:, None] * 0.125 * 3 * d[None, :]).astype(np.float32)   # exact: multiples of 2^-3
    c = O.OracleCloud(line, gp=O.default_gicp(k_correspondences=8, cov_radius=1.6))   # five neighbours at the ends
    assert c.count.min() >= 4
    worst = 0.0
    for c6 in c.cov:
        S = O.sym(c6)
        w = np.linalg.eigvalsh(S)
        worst = max(worst, abs(w[0] - EPS), abs(w[1] - 1), abs(w[2] - 1), abs(d @ S @ d - 1))
    print("line: eigenvalues and d'C'd off by at most %.3g" % worst)
    assert worst <= 1e-12


def test_point_with_three_neighbours_gets_the_identity():
    xyz = np.concatenate([G.random_cloud(40, 5, 4.0) + 100, [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]]]).astype(np.float32)
    c = O.OracleCloud(xyz, gp=O.default_gicp(cov_radius=0.5))
    assert list(c.count[-3:]) == [3, 3, 3]
    assert np.array_equal(c.cov[-3:], np.tile([1.0, 0, 0, 1.0, 0, 1.0], (3, 1)))


def test_cloud_of_k_minus_one_points_is_refused():
    with pytest.raises(ValueError):
        O.OracleCloud(G.random_cloud(19, 1, 1.0))
    O.OracleCloud(G.random_cloud(20, 1, 1.0))


def expm_twist(xi):
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx if th > 0 else 0)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, v
    return T


def test_jacobian_against_central_differences_of_the_cost():
    """With an isotropic C'p, M does not depend on the rotation, the cost of a pair is r' M r and its gradient in xi is 2 g."""
    rs = np.random.RandomState(2)
    worst = 0.0
    for _ in range(8):
        T = G.rigid(yaw=rs.uniform(-1, 1), shift=rs.uniform(-2, 2, 3))
        p, q = rs.uniform(-3, 3, 3).astype(np.float32), rs.uniform(-3, 3, 3).astype(np.float32)
        A = rs.normal(size=(3, 3))
        Cq = A @ A.T + 0.1 * np.eye(3)
        Cq6, Cp6 = Cq[np.triu_indices(3)], np.array([0.7, 0, 0, 0.7, 0, 0.7])
        _, g, _ = O.pair_terms(T, p, q, Cp6, Cq6)
        fd = np.zeros(6)
        for k in range(6):
            e = np.zeros(6)
            e[k] = 1e-6
            cp = O.pair_terms(expm_twist(e) @ T, p, q, Cp6, Cq6)[2]
            cm = O.pair_terms(expm_twist(-e) @ T, p, q, Cp6, Cq6)[2]
            fd[k] = (cp - cm) / 2e-6
        worst = max(worst, np.abs(fd - 2 * g).max() / np.abs(2 * g).max())
    print("J' M r against central differences: %.3g relative" % worst)
    assert worst <= 1e-6


def run_case(name):
    c = G.CASES[name]
    kp, gp = K.default_params(**c["store"]), O.default_gicp(**c["gicp"])
    tgt, src = O.OracleCloud(c["target"], kp, gp), O.OracleCloud(c["source"], kp, gp)
    return c, O.register_gicp(tgt, src, np.asarray(c["init"], np.float32), gp)


def test_exact_rigid_copy_is_recovered():
    for name in ("copy-shift", "copy-still"):
        c, r = run_case(name)
        err = np.abs(r["transform64"] - c["truth"]).max()
        print("%s: %d iterations, state %d, |T - truth| = %.3g, margin %.3g" % (name, r["iterations"], r["state"], err, r["margin"]))
        assert r["state"] == api.KF_TRANSFORM and r["converged"] == 1 and r["pairs"] == 192
        assert err <= 1e-12


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_hand_worked_cases_reach_their_state(name):
    c, r = run_case(name)
    print("%s: state %d, %d iterations, %d pairs, trace %s, margin %.3g" %
          (name, r["state"], r["iterations"], r["pairs"], r["pairs_trace"][:r["iterations"] + 1], r["margin"]))
    assert r["state"] == c["state"] and r["pairs"] == c["pairs"]
    assert r["converged"] == (1 if c["state"] in (api.KF_ITERATIONS, api.KF_TRANSFORM) else 0)
    if c["iterations"] is not None:
        assert r["iterations"] == c["iterations"]
    if c["truth"] is not None and c["state"] == api.KF_TRANSFORM:
        assert np.abs(r["transform64"] - c["truth"]).max() <= c.get("truth_tol", 1e-12)
    assert r["margin"] > 1e-9       # no stop test is close: the device is not excused on any of them
    if name == "nan-init":
        assert np.isnan(r["transform64"][:3]).all()
    if name == "line":
        assert r["hessian"][0, 0] == 0.0


def test_every_stop_state_is_reached():
    states = {run_case(n)[1]["state"] for n in G.CASES}
    assert states == {api.KF_ITERATIONS, api.KF_TRANSFORM, api.KF_NO_CORRESPONDENCES, api.KF_DEGENERATE}


def test_gate_pair_is_dropped_here_and_kept_by_the_icp_edge():
    c, r = run_case("gate")
    kp = K.default_params(**c["store"])
    icp = K.register_edge(K.OracleKeyframe(c["target"], kp), c["source"], np.eye(4, dtype=np.float32), params=kp)
    assert r["pairs_trace"][0] == 0 and icp["pairs_trace"][0] == 8


def test_plane_to_plane_beats_point_to_point_on_interleaved_samples():
    """Two clouds sample the same floor and walls half a pitch apart.  Point to point pulls samples onto samples; plane to
    plane lets them slide.  Both restatements from the same start; no number is fixed in advance, only the inequality."""
    tgt, src, truth = G.interleaved_scene()
    kp = K.default_params(leaf_size=0.125, gate=0.75)
    gp = O.default_gicp(max_iterations=50)
    init = (G.INTERLEAVED_START @ truth).astype(np.float32)
    g = O.register_gicp(O.OracleCloud(tgt, kp, gp), O.OracleCloud(src, kp, gp), init, gp)
    p = K.register_edge(K.OracleKeyframe(tgt, kp), src, init, params=kp)
    eg, ep = K.pose_error(g["transform64"], truth), K.pose_error(p["transform64"], truth)
    print("GICP: %.4g m, %.4g rad (%d iterations, state %d); point to point: %.4g m, %.4g rad (%d iterations, state %d)" %
          (eg + (g["iterations"], g["state"]) + ep + (p["iterations"], p["state"])))
    assert g["converged"] == 1 and p["converged"] == 1
    assert eg[0] < ep[0] and eg[1] <= ep[1] + 1e-12


def test_python_structs_mirror_the_header(tmp_path):
    structs = {"slam_kf_gicp_params": api.KfGicpParams, "slam_kf_gicp_result": api.KfGicpResult}
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
    for line in subprocess.check_output([str(exe)], text=True).strip().splitlines():
        parts = line.split()
        cls = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), (parts[0], parts[1], C.sizeof(cls))
        for p in parts[2:]:
            f, off = p.split("=")
            assert getattr(cls, f).offset == int(off), (parts[0], f, off)
    assert api.KF_DEGENERATE == 6


def test_default_settings_leave_no_identity_covariances_on_the_test_keyframes():
    """The keyframes the device tests register, filtered at 0.5 m by a restatement of the voxel filter's centroids: with the
    default radius (twice the lattice edge, 1.5 m) every point of keyframes 0, 1, 2 and 4 has at least cov_min_neighbours = 4
    neighbours.  Keyframe 8 breaks that with one point of 4 543 (0.02 %), so for the rest of EDGE_KS the bound is 1 %."""
    for k in K.EDGE_KS:
        xyz = K.cloud(k)[0][:, :3].astype(np.float64)
        cell = np.floor(xyz / 0.5).astype(np.int64)
        _, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
        cen = np.zeros((len(cnt), 3))
        np.add.at(cen, inv.ravel(), xyz)
        f = (cen / cnt[:, None]).astype(np.float32)
        c = O.OracleCloud(f)
        share = float((c.count < 4).mean())
        print("keyframe %d: %d points, %.1f %% with the full 20 neighbours, %.2f %% fall back to the identity" %
              (k, len(f), 100 * (c.count == 20).mean(), 100 * share))
        assert share == 0.0 if k in (0, 1, 2, 4) else share <= 0.01, k
