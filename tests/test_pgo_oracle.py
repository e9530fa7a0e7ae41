"""The pose-graph optimiser's contract (docs/PGO.md) on the CPU: tests/cpp/pgo_oracle.cpp against closed forms, finite
differences and numpy; every rule has a mutation behind a switch that a named test catches; and the host-only calls of
slam_pgo_* (the graph is host state) with their argument errors.  tests/test_gpu_pgo.py holds the device to the restatement."""
import numpy as np
import pytest

import pgo_cases as K
import pgo_oracle as O
from slam_amd import api, build


@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def random_pose(rng, spread=3.0):
    q = rng.standard_normal(4)
    return np.concatenate([rng.uniform(-spread, spread, 3), q / np.linalg.norm(q)])


# ------------------------------------------------------------------ the vector maps
def test_mqt_round_trips_flips_and_saturates():
    rng = np.random.default_rng(0)
    for _ in range(50):
        v = np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(-0.5, 0.5, 3)])
        assert np.allclose(O.to_mqt(O.from_mqt(v)), v, rtol=0, atol=1e-15)
        assert np.allclose(O.from_mqt(v), K.from_mqt(v), rtol=0, atol=1e-15)
    p = np.array([1.0, 2.0, 3.0, 0.1, -0.2, 0.3, -np.sqrt(1 - 0.14)])          # w < 0: the vector part changes sign
    assert np.allclose(O.to_mqt(p), [1, 2, 3, -0.1, 0.2, -0.3]) and np.allclose(O.to_mqt(p, flip=False), [1, 2, 3, 0.1, -0.2, 0.3])
    big = O.from_mqt([0, 0, 0, 3.0, 0.0, 4.0])                                # n2 > 1: normalised vector part, w = 0
    assert np.allclose(big, [0, 0, 0, 0.6, 0.0, 0.8, 0.0])
    edge = O.from_mqt([0, 0, 0, 1.0, 0.0, 0.0])                               # n2 == 1 is not "> 1"
    assert np.array_equal(edge, [0, 0, 0, 1.0, 0.0, 0.0, 0.0])


def test_update_is_right_multiplied_and_renormalised():
    rng = np.random.default_rng(1)
    for _ in range(20):
        X, d = random_pose(rng), np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.3, 0.3, 3)])
        want = K.compose(X, K.from_mqt(d))
        assert np.allclose(O.oplus(X, d), want, rtol=0, atol=1e-14)
        assert abs(np.linalg.norm(O.oplus(X, d)[3:]) - 1.0) < 4e-16
        assert not np.allclose(O.oplus(X, d, left=True), want, atol=1e-3)


def _edge_graph(rng, mutation=O.MUT_NONE):
    g = O.OracleGraph(mutation=mutation)
    Xi, Xj, Z = random_pose(rng), random_pose(rng), random_pose(rng)
    g.add_vertex(0, Xi, False)
    g.add_vertex(1, Xj, False)
    g.add_edge(0, 1, Z, K.information(rng))
    return g, Xi, Xj


def test_jacobians_against_central_differences():
    """200 random (Xi, Xj, Z); h = 1e-6, bound 1e-7 (the truncation error of the difference is about h^2 = 1e-12 times the
    third derivative, its rounding about 1e-16 / h = 1e-10 times |e|)"""
    rng, h, worst = np.random.default_rng(2), 1e-6, 0.0
    for _ in range(200):
        g, Xi, Xj = _edge_graph(rng)
        J = g.jacobians(0)
        for v, X in ((0, Xi), (1, Xj)):
            num = np.zeros((6, 6))
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                g.set_vertex(v, O.oplus(X, d))
                ep = g.chi2()[1][0]
                g.set_vertex(v, O.oplus(X, -d))
                em = g.chi2()[1][0]
                g.set_vertex(v, X)
                num[:, a] = (ep - em) / (2 * h)
            worst = max(worst, np.abs(num - J[v]).max())
    print("Jacobians against central differences: worst %.3g" % worst)
    assert worst <= 1e-7


def test_jacobians_cover_the_negative_w_branch():
    """of the 200 triples above about half have w < 0 in the error quaternion: there e differs without the flip"""
    rng, seen = np.random.default_rng(2), 0
    for _ in range(200):
        g, _, _ = _edge_graph(rng)
        seen += _no_flip_differs(g, g.chi2()[1][0])
    assert 50 <= seen <= 150, seen


def _no_flip_differs(g, e_flip):
    O.lib().pgoo_set_mutation(g.h, O.MUT_NO_FLIP)
    e_raw = g.chi2()[1][0]
    O.lib().pgoo_set_mutation(g.h, O.MUT_NONE)
    return not np.array_equal(e_raw, e_flip)


def test_error_does_not_depend_on_the_sign_of_a_quaternion():
    """q and -q are one rotation: e (through toVectorMQT's w >= 0) and chi2 are the same.  Without the flip they are not."""
    case = K.loop_graph(24, 2, 1)
    flipped = K.Case("flipped", case.poses * np.where(np.arange(case.n) % 3 == 1, -1.0, 1.0)[:, None] ** np.array([0, 0, 0, 1, 1, 1, 1]),
                     case.fixed, case.edges)
    a, b = case.fill(O.OracleGraph()).chi2(), flipped.fill(O.OracleGraph()).chi2()
    assert np.array_equal(a[1], b[1]) and a[0] == b[0]
    m = flipped.fill(O.OracleGraph(mutation=O.MUT_NO_FLIP)).chi2()
    negated = [k for k in range(len(case.edges)) if np.array_equal(m[1][k, 3:], -a[1][k, 3:]) and a[1][k, 3:].any()]
    assert negated and np.array_equal(m[1][:, :3], a[1][:, :3])
    assert abs(m[0] - a[0]) > 1e-8 * a[0]        # the information couples translation and rotation: chi2 moves with the sign
    r = flipped.fill(O.OracleGraph()).read_vertices()
    assert (r[:, 6] >= 0).all() and np.allclose(np.abs(r), np.abs(case.poses), rtol=0, atol=1e-12)


# ------------------------------------------------------------------ closed forms
def test_two_vertices_and_one_edge_end_at_x0_z():
    rng = np.random.default_rng(3)
    X0, Z = random_pose(rng), random_pose(rng, 1.0)
    g = O.OracleGraph()
    g.add_vertex(0, X0, True)
    g.add_vertex(1, K.compose(K.compose(X0, Z), K.from_mqt([0.2, -0.1, 0.1, 0.05, -0.04, 0.03])), False)
    g.add_edge(0, 1, Z, K.information(rng))
    res = g.optimize(10)
    dm, dr = K.pose_errors(g.read_vertices()[1], K.compose(X0, Z))
    print("pair: chi2 %.3g -> %.3g, %.3g m %.3g rad from X0 Z" % (res.chi2_initial, res.chi2_final, dm[0], dr[0]))
    assert res.chi2_final < K.CHI2_ZERO and dm[0] < 1e-12 and dr[0] < 1e-12


def test_pure_translation_triangles_against_lstsq():
    """identity rotations, so e = (tj - ti) - z in its first three rows: one undamped step is the least-squares solution of
    sqrt(W) J delta = -sqrt(W) e (numpy.linalg.lstsq on the stacked rows), and the iteration ends where that step is zero"""
    rng = np.random.default_rng(4)
    ident = np.array([0, 0, 0, 1.0])
    for _ in range(5):
        t = rng.uniform(-3, 3, (3, 3))
        pairs = [(0, 1), (1, 2), (0, 2)]
        z = [t[j] - t[i] + rng.normal(0, 0.05, 3) for i, j in pairs]
        w = [np.concatenate([rng.uniform(50, 500, 3), [1e4, 1e4, 1e4]]) for _ in pairs]
        g = O.OracleGraph()
        g.add_vertex(0, np.concatenate([t[0], ident]), True)
        for k in (1, 2):
            g.add_vertex(k, np.concatenate([t[k] + rng.normal(0, 0.3, 3), ident]), False)
        for (i, j), zz, ww in zip(pairs, z, w):
            g.add_edge(i, j, np.concatenate([zz, ident]), np.diag(ww))
        e = g.chi2()[1]
        pos = g.read_vertices()[:, :3]
        assert np.allclose(e[:, :3], [pos[j] - pos[i] - zz for (i, j), zz in zip(pairs, z)], atol=1e-14) and not e[:, 3:].any()
        A, rhs = np.zeros((18, 12)), np.zeros(18)
        for k, ((i, j), ww) in enumerate(zip(pairs, w)):
            Ji, Jj = g.jacobians(k)
            s = np.sqrt(ww)[:, None]
            if i:
                A[6 * k:6 * k + 6, 6 * (i - 1):6 * i] = s * Ji
            A[6 * k:6 * k + 6, 6 * (j - 1):6 * j] = s * Jj
            rhs[6 * k:6 * k + 6] = -s[:, 0] * e[k]
        sol = np.linalg.lstsq(A, rhs, rcond=None)[0].reshape(2, 6)
        step = g.step(0.0)
        assert step["pivot"] == 0 and not step["delta"][0].any()
        assert np.abs(step["delta"][1:] - sol).max() < 1e-10 * max(1.0, np.abs(sol).max())
        res = g.optimize(10)
        assert np.abs(g.step(0.0)["delta"]).max() < 1e-7 and res.chi2_final < res.chi2_initial


# ------------------------------------------------------------------ the generator's graphs
LOOPS = [(24, 2), (60, 2), (120, 3)]
_loop_runs = {}


def loop_run(n, laps):
    if (n, laps) not in _loop_runs:
        case = K.loop_graph(n, laps, 1)
        dense, banded = case.fill(O.OracleGraph()), case.fill(O.OracleGraph(banded=True))
        perm, w = dense.rcm()
        lam = 1e-5 * np.diag(dense.system()[0]).max()
        sd, sb = dense.step(lam), banded.step(lam)
        _loop_runs[(n, laps)] = (case, dense, dense.optimize(10), banded, banded.optimize(10), w, sd, sb)
    return _loop_runs[(n, laps)]


@pytest.mark.parametrize("n,laps", LOOPS)
def test_loop_graphs_descend_and_approach_the_truth(n, laps):
    case, g, res, _, _, w, _, _ = loop_run(n, laps)
    assert len(case.edges) == {24: 59, 60: 149, 120: 359}[n]
    chi2 = res.chi2_initial
    for lam, rho, c, accepted in O.trace(res):
        if accepted:
            assert c <= chi2
            chi2 = c
    assert chi2 == res.chi2_final < 0.05 * res.chi2_initial
    before, after = K.pose_errors(case.poses, case.truth)[0], K.pose_errors(g.read_vertices(), case.truth)[0]
    natural = max(abs(i - j) for i, j, _, _ in case.edges if i > 0)
    print("N %d: E %d, chi2 %.6g -> %.6g, position error %.3g -> %.3g m (max), w %d under RCM, %d in natural order"
          % (n, len(case.edges), res.chi2_initial, res.chi2_final, before.max(), after.max(), w, natural))
    assert after.max() < 0.5 * before.max() and after.mean() < 0.5 * before.mean()
    assert w < natural


@pytest.mark.parametrize("n,laps", LOOPS)
def test_dense_and_banded_solves_agree(n, laps):
    """the spread a change of elimination order alone makes: recorded (docs/PGO.md); tests/test_gpu_pgo.py allows the device
    100 x the step's.  The bound here is what the project allows a pose test at all."""
    case, g, res, gb, resb, w, sd, sb = loop_run(n, laps)
    dm, dr = K.pose_errors(g.read_vertices(), gb.read_vertices())
    step = np.abs(sd["delta"] - sb["delta"]).max() / np.abs(sd["delta"]).max()
    rel = abs(res.chi2_final - resb.chi2_final) / res.chi2_final
    print("N %d: dense against banded-RCM: one step's delta %.3g relative, final poses %.3g m %.3g rad, chi2 %.3g relative"
          % (n, step, dm.max(), dr.max(), rel))
    assert dm.max() < K.POSE_TOL_M and dr.max() < K.POSE_TOL_RAD and rel < 1e-9 and step < 1e-9


# ------------------------------------------------------------------ the LM rules
def test_rule_graphs_hold_their_conditions():
    r = K.rule_graph(K.RULE_REJECT_SEED).fill(O.OracleGraph()).optimize(10)
    n = K.compared_trials(r)
    assert any(not t.accepted and t.rho < -0.1 for t in r.trace[:n]) and n >= 3
    r = K.rule_graph(K.RULE_STREAK_SEED).fill(O.OracleGraph()).optimize(10)
    n = K.compared_trials(r)
    assert n >= 3 and [t.accepted for t in r.trace[:3]] == [0, 0, 0]


def test_lambda_follows_the_accept_and_reject_rules():
    r = K.rule_graph(K.RULE_STREAK_SEED).fill(O.OracleGraph()).optimize(10)
    tr = O.trace(r)
    nu = 2.0
    for (lam, rho, c, acc), (lam_next, _, _, _) in zip(tr, tr[1:]):
        if acc:
            factor, nu = max(1.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)), 2.0
        else:
            factor, nu = nu, 2.0 * nu
        assert lam_next == pytest.approx(lam * factor, rel=1e-15)
        assert acc == (rho > 0 and np.isfinite(c))


def test_update_rule_predicts_the_decrease():
    """a small damped step falls by what the linear model says (rho near 1); with the increment on the left the Jacobians
    no longer belong to the update and it does not"""
    case = K.loop_graph(24, 2, 1)
    lam = 1e3 * np.diag(case.fill(O.OracleGraph()).system()[0]).max()
    rho = {}
    for m in (O.MUT_NONE, O.MUT_LEFT_UPDATE):
        s = case.fill(O.OracleGraph(mutation=m)).step(lam)
        rho[m] = (s["chi2_before"] - s["chi2_after"]) / (s["scale"] + 1e-3)
    print("rho of a small step: %.6f, left-multiplied %.6f" % (rho[O.MUT_NONE], rho[O.MUT_LEFT_UPDATE]))
    assert abs(rho[O.MUT_NONE] - 1.0) < 0.01 and abs(rho[O.MUT_LEFT_UPDATE] - 1.0) > 0.1


def test_scale_carries_its_1e_3():
    """at the optimum delta is zero and scale is zero: rho = 0 / 1e-3 = 0 stops the call (RHO_ZERO); without the 1e-3 it is 0 / 0"""
    X0, Z = K.rpy_pose(1, 2, 0.5, 0, 0, 0), K.rpy_pose(1, 0, 0, 0, 0, 0)
    stop = {}
    for m in (O.MUT_NONE, O.MUT_SCALE_NO_EPS):
        g = O.OracleGraph(mutation=m)
        g.add_vertex(0, X0, True)
        g.add_vertex(1, K.compose(X0, Z), False)
        g.add_edge(0, 1, Z, np.eye(6))
        res = g.optimize(10)
        stop[m] = (res.stop_reason, res.iterations)
    assert stop[O.MUT_NONE] == (api.PGO_STOP_RHO_ZERO, 1) and stop[O.MUT_SCALE_NO_EPS] == (api.PGO_STOP_ITERATIONS, 10)


def test_lambda_starts_anew_in_every_call():
    case = K.loop_graph(24, 2, 1)
    for m, same in ((O.MUT_NONE, True), (O.MUT_KEEP_LAMBDA, False)):
        g = case.fill(O.OracleGraph(mutation=m))
        g.optimize(3)
        lam0 = 1e-5 * np.diag(g.system()[0]).max()
        res = g.optimize(3)
        assert (res.trace[0].lambda_ == lam0) == same


def test_max_trials_stops_a_call():
    g = O.OracleGraph()
    g.add_vertex(0, [0, 0, 0, 0, 0, 0, 1], True)
    g.add_vertex(1, [1, 0, 0, 0, 0, 0, 1], False)
    g.add_edge(0, 1, [1.5, 0, 0, 0, 0, 0, 1], -np.eye(6))
    res = g.optimize(10)
    assert (res.stop_reason, res.n_trials) == (api.PGO_STOP_MAX_TRIALS, 10) and not any(t.accepted for t in res.trace[:10])
    with pytest.raises(ValueError):      # no fixed vertex
        O.OracleGraph().optimize(10)


# ------------------------------------------------------------------ the library's host-only calls
def test_host_calls_need_no_device_and_check_their_arguments(L):
    g = api.PoseGraph()
    ident = [0, 0, 0, 0, 0, 0, 1.0]

    def refused(f, *a):
        with pytest.raises(api.SlamError) as e:
            f(*a)
        assert e.value.code == api.E_INVALID, e.value
        return str(e.value)

    assert "dense and in order" in refused(g.add_vertex, 1, ident)
    g.add_vertex(0, [1, 2, 3, 0, 0, 0, -2.0], True)                       # normalised on the way in, w >= 0 on the way out
    assert np.array_equal(g.read_vertices(), [[1, 2, 3, 0, 0, 0, 1.0]])
    refused(g.add_vertex, 0, ident)
    refused(g.add_vertex, 1, [0, 0, 0, 0, 0, 0, 0.0])
    refused(g.add_vertex, 1, [np.nan, 0, 0, 0, 0, 0, 1.0])
    g.add_vertex(1, ident, False)
    refused(g.set_vertex, 2, ident)
    refused(g.set_vertex, -1, ident)
    refused(g.set_vertex, 1, [0, 0, 0, np.inf, 0, 0, 1.0])
    g.set_vertex(1, [4, 5, 6, 0.6, 0, 0, 0.8])
    assert np.array_equal(g.read_vertices()[1], [4, 5, 6, 0.6, 0, 0, 0.8])   # unit to rounding already: kept bit for bit
    refused(g.add_edge, 0, 0, ident, np.eye(6))
    refused(g.add_edge, 0, 2, ident, np.eye(6))
    refused(g.add_edge, -1, 1, ident, np.eye(6))
    refused(g.add_edge, 0, 1, [0, 0, 0, 0, 0, 0, 0.0], np.eye(6))
    refused(g.add_edge, 0, 1, ident, np.full((6, 6), np.nan))
    g.add_edge(1, 0, ident, np.eye(6))
    assert g.size() == (2, 1)
    g.clear()
    assert g.size() == (0, 0) and g.read_vertices().shape == (0, 7)
    g.close()
    with pytest.raises(api.SlamError) as e:
        api.PoseGraph(max_trials=0)
    assert e.value.code == api.E_INVALID
    p = api.pgo_default_params()
    assert (p.max_trials, p.tau, p.good_lower, p.good_upper, p.ordering, p.max_band_bytes) == \
        (10, 1e-5, 1.0 / 3.0, 2.0 / 3.0, api.PGO_ORDER_RCM, 1 << 30)


def test_result_structures_mirror_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"slam_pgo_params": api.PgoParams, "slam_pgo_trial": api.PgoTrial, "slam_pgo_result": api.PgoResult}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (f, name, f.rstrip("_")))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    for line in subprocess.check_output([str(exe)], text=True).strip().splitlines():
        parts = line.split()
        cls = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), parts[:2]
        for p in parts[2:]:
            f, off = p.split("=")
            assert getattr(cls, f).offset == int(off), (parts[0], f)
    assert api.PGO_TRACE == 64


@pytest.mark.skipif(api.device_count() > 0, reason="a GPU is present")
def test_device_calls_fail_loudly_without_a_device(L):
    g = K.small_shapes()["triangle"].fill(api.PoseGraph())
    before = g.read_vertices()
    for call in (lambda: g.optimize(10), g.chi2, g.read_system, lambda: g.step(1.0)):
        with pytest.raises(api.SlamError) as e:
            call()
        assert e.value.code == api.E_HIP and "no HIP device" in str(e.value)
    assert np.array_equal(g.read_vertices(), before)
    g.close()
