"""slam_pgo_* on the device against tests/cpp/pgo_oracle.cpp (docs/PGO.md has the contract and the measured figures).

Stages (e, chi2, the blocks and b) are held to CHAIN_TOL of the array's largest magnitude.  One step's delta is held to 100 x
the spread between the restatement's own two solves (dense in natural order, banded under RCM) for that graph, with a floor
of 1e-12 relative, and its residual to 100 x the restatement's own.  optimize(10) is held to 1e-4 m / 1e-5 rad and 1e-9
relative in chi2; the trace is compared trial by trial up to the first trial whose margin |chi2 - chi2'| is below
MARGIN_TOL x chi2 in the restatement.

Inside the compared part the bound on rho and lambda is derived, not observed: both sides know chi2 and chi2' to
CHI2_RTOL = 1e-12 relative at worst (sums of a few hundred terms of like sign, three orders above the unit roundoff), so
rho = (chi2 - chi2') / scale differs relatively by at most 2 CHI2_RTOL / margin + CHAIN_TOL, where margin is that trial's
|chi2 - chi2'| / chi2; lambda's factor max(1/3, min(1 - (2 rho - 1)^3, 2/3)) has a slope of at most 6 over a value of at least
1/3, so lambda's relative bound grows by 18 |d rho| per accepted trial from CHAIN_TOL (max diag H) at the first."""
import ctypes as C

import numpy as np
import pytest

import pgo_cases as K
import pgo_oracle as O
from slam_amd import api

pytestmark = pytest.mark.gpu

CHI2_RTOL = 1e-12
DELTA_FLOOR = 1e-12
# not trace graphs: without a cycle and with one block per vertex their chi2 is zero (CHI2_ZERO) after two trials; every other
# graph has at least three compared trials (checked on the restatement, and asserted below)
NO_TRACE = ("pair", "star6")


def _cases():
    c = dict(K.small_shapes())
    c["loop24"] = K.loop_graph(24, 2, 1)
    c["loop60"] = K.loop_graph(60, 2, 1)
    c["loop120"] = K.loop_graph(120, 3, 1)
    for n in (63, 64, 65, 257):
        c["edges%d" % n] = K.repeated_edges(c["loop24"], n, "edges%d" % n)
    c["rule_reject"] = K.rule_graph(K.RULE_REJECT_SEED)
    c["rule_streak"] = K.rule_graph(K.RULE_STREAK_SEED)
    return c


CASES = _cases()
# (case, ordering): every shape under RCM; the two-lap loop and N = 60 under NATURAL too (w = 13 and 31)
RUNS = [(name, api.PGO_ORDER_RCM) for name in CASES if name != "loop60"] + [("loop24", api.PGO_ORDER_NATURAL), ("loop60", api.PGO_ORDER_NATURAL)]
RUN_IDS = ["%s-%s" % (n, "rcm" if o == api.PGO_ORDER_RCM else "natural") for n, o in RUNS]
_ref = {}


def reference(name):
    """What the restatement says about a case, computed once: stages, one step by both solves, optimize(10)."""
    if name in _ref:
        return _ref[name]
    case = CASES[name]
    g = case.fill(O.OracleGraph())
    chi2, e, chi2_e = g.chi2()
    H, b = g.system()
    free = [v for v in range(case.n) if not case.fixed[v]]
    lam = 1e-5 * max(H[6 * v + c, 6 * v + c] for v in free for c in range(6))
    dense, banded = g.step(lam, banded=False), g.step(lam, banded=True)
    perm, w = g.rcm()
    res = g.optimize(10)
    _ref[name] = dict(chi2=chi2, e=e, chi2_e=chi2_e, H=H, b=b, lam=lam, dense=dense, banded=banded, perm=perm, w=w, res=res,
                      poses=g.read_vertices(), free=free)
    return _ref[name]


def device_graph(name, ordering=api.PGO_ORDER_RCM, **kw):
    return CASES[name].fill(api.PoseGraph(ordering=ordering, **kw))


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert api.device_count() > 0
    api.set_device(0)


def near(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, np.finfo(np.float64).tiny)
    worst = float(np.abs(a - b).max()) / scale if b.size else 0.0
    print("%s: worst %.3g of the largest magnitude %.3g (bound %.3g)" % (what, worst, scale, tol))
    assert worst <= tol, what


@pytest.mark.parametrize("name,ordering", RUNS, ids=RUN_IDS)
def test_stages_match_the_restatement(name, ordering):
    ref, case = reference(name), CASES[name]
    g = device_graph(name, ordering)
    chi2, e, chi2_e = g.chi2()
    near(e, ref["e"], K.CHAIN_TOL, "e")
    near(chi2_e, ref["chi2_e"], K.CHAIN_TOL, "chi2 per edge")
    near([chi2], [ref["chi2"]], K.CHAIN_TOL, "chi2")
    s = g.read_system()
    if ordering == api.PGO_ORDER_RCM:
        assert s["w"] == ref["w"] and np.array_equal(s["perm"], ref["perm"])
    else:
        assert np.array_equal(s["perm"], ref["free"])
    pos = {int(v): r for r, v in enumerate(s["perm"])}
    assert all(pos[r] >= pos[c] and pos[r] - pos[c] <= s["w"] for r, c in zip(s["rows"], s["cols"]))
    assert len(s["rows"]) == sum(min(r, s["w"]) + 1 for r in range(len(s["perm"])))
    near(K.dense_from_blocks(s, case.n), ref["H"], K.CHAIN_TOL, "H")
    near(s["b"], ref["b"], K.CHAIN_TOL, "b")
    g.close()


@pytest.mark.parametrize("name,ordering", RUNS, ids=RUN_IDS)
def test_one_step_matches_the_restatement(name, ordering):
    ref, case = reference(name), CASES[name]
    g = device_graph(name, ordering)
    d = g.step(ref["lam"])
    assert d["pivot"] == 0 and ref["dense"]["pivot"] == 0
    want = ref["dense"]["delta"]
    top = np.abs(want).max()
    spread = np.abs(ref["banded"]["delta"] - want).max() / top
    bound = max(100.0 * spread, DELTA_FLOOR)
    got = np.abs(d["delta"] - want).max() / top
    print("%s delta: device against dense %.3g relative, dense against banded %.3g, bound %.3g" % (name, got, spread, bound))
    A = ref["H"] + ref["lam"] * np.eye(6 * case.n)
    fr = np.array([6 * v + c for v in ref["free"] for c in range(6)])
    rhs = ref["b"].reshape(-1)[fr]
    res_dev = np.abs(A[np.ix_(fr, fr)] @ d["delta"].reshape(-1)[fr] - rhs).max()
    res_ref = np.abs(A[np.ix_(fr, fr)] @ want.reshape(-1)[fr] - rhs).max()
    res_bound = max(100.0 * res_ref, 1e-12 * np.abs(rhs).max())
    print("%s residual: device %.3g, restatement %.3g, bound %.3g" % (name, res_dev, res_ref, res_bound))
    assert got <= bound
    assert res_dev <= res_bound
    assert np.all(d["delta"][np.array(case.fixed)] == 0.0)
    near([d["chi2_before"], d["chi2_after"], d["scale"]], [ref["dense"]["chi2_before"], ref["dense"]["chi2_after"], ref["dense"]["scale"]],
         K.CHAIN_TOL, "chi2 before, after and scale")
    # it applies nothing
    assert np.array_equal(g.read_vertices(), device_graph(name, ordering).read_vertices())
    g.close()


@pytest.mark.parametrize("name,ordering", RUNS, ids=RUN_IDS)
def test_optimize_matches_the_restatement(name, ordering):
    ref = reference(name)
    g = device_graph(name, ordering)
    res = g.optimize(10)
    want = ref["res"]
    dm, dr = K.pose_errors(g.read_vertices(), ref["poses"])
    # a chi2 below CHI2_ZERO is zero on both sides (a graph without a cycle); otherwise 1e-9 relative
    rel = 0.0 if max(res.chi2_final, want.chi2_final) < K.CHI2_ZERO else abs(res.chi2_final - want.chi2_final) / want.chi2_final
    print("%s: poses %.3g m %.3g rad, chi2 %.6g -> %.6g (%.3g relative to the restatement's), w %d, %d trials, stop %d"
          % (name, dm.max(), dr.max(), res.chi2_initial, res.chi2_final, rel, res.half_bandwidth, res.n_trials, res.stop_reason))
    assert dm.max() <= K.POSE_TOL_M and dr.max() <= K.POSE_TOL_RAD
    assert rel <= 1e-9 and abs(res.chi2_initial - want.chi2_initial) <= 1e-9 * want.chi2_initial
    assert res.chi2_final <= res.chi2_initial
    assert res.free_vertices == len(ref["free"]) and res.band_bytes == res.free_vertices * (res.half_bandwidth + 1) * 288
    n = K.compared_trials(want)
    print("%s: %d of %d trials compared" % (name, n, want.n_trials))
    assert (n >= 3 or name in NO_TRACE) and res.n_trials >= n
    # chi2' = e' W e moves by 2 |W e| |de|: |W e| <= sqrt(|W| chi2'), and e, a difference of coordinates, is known to
    # CHI2_RTOL of the largest coordinate -- what is left of the bound where chi2' falls far below chi2 on the way to zero
    case = CASES[name]
    w_top = 6.0 * max(np.abs(e[3]).max() for e in case.edges)
    e_abs = CHI2_RTOL * max(1.0, np.abs(case.poses).max())
    lam_tol = K.CHAIN_TOL
    for k in range(n):
        a, b = res.trace[k], want.trace[k]
        rho_tol = 2.0 * CHI2_RTOL / want.margins[k] + K.CHAIN_TOL
        assert a.accepted == b.accepted, k
        assert abs(a.lambda_ - b.lambda_) <= lam_tol * abs(b.lambda_), (k, a.lambda_, b.lambda_)
        assert abs(a.rho - b.rho) <= rho_tol * abs(b.rho), (k, a.rho, b.rho)
        assert abs(a.chi2 - b.chi2) <= 1e-9 * abs(b.chi2) + 2.0 * np.sqrt(w_top * abs(b.chi2)) * e_abs, (k, a.chi2, b.chi2)
        if b.accepted:
            lam_tol += 18.0 * rho_tol * abs(b.rho)
    g.close()


def test_rule_graphs_reject_inside_the_compared_part():
    """the rejected trials the LM-rule graphs were chosen for are among the trials the device is compared on"""
    for name, need in (("rule_reject", 1), ("rule_streak", 3)):
        want = reference(name)["res"]
        n = K.compared_trials(want)
        rejected = [k for k in range(n) if not want.trace[k].accepted]
        assert len(rejected) >= need, (name, rejected, n)
    g = device_graph("rule_reject")
    res = g.optimize(10)
    assert res.trace[0].accepted == 0 and res.trace[0].rho < -0.1
    g.close()


def _bits(g, res):
    return g.read_vertices().tobytes(), res.chi2_initial, res.chi2_final, [(t.lambda_, t.rho, t.chi2, t.accepted) for t in res.trace[:res.n_trials]]


@pytest.mark.parametrize("name", ["chain8", "loop24", "edges257", "loop120"])
def test_the_same_call_twice_gives_the_same_bits(name):
    a, b = device_graph(name), device_graph(name)
    assert _bits(a, a.optimize(10)) == _bits(b, b.optimize(10))
    sa, sb = a.step(0.5), b.step(0.5)
    assert sa["delta"].tobytes() == sb["delta"].tobytes() and sa["scale"] == sb["scale"]
    a.close(), b.close()


def test_a_graph_grown_after_an_optimize_equals_a_fresh_one():
    case, nv = CASES["loop24"], 16
    ne = sum(1 for e in case.edges if e[1] < nv)
    assert all(e[1] < nv for e in case.edges[:ne]) and all(e[1] >= nv for e in case.edges[ne:])
    grown = api.PoseGraph()
    case.fill(grown, vertices=(0, nv), edges=(0, ne))
    grown.optimize(10)
    mid = grown.read_vertices()
    case.fill(grown, vertices=(nv, case.n), edges=(ne, len(case.edges)))
    fresh = api.PoseGraph()
    for k in range(nv):
        fresh.add_vertex(k, mid[k], case.fixed[k])
    case.fill(fresh, vertices=(nv, case.n), edges=(0, len(case.edges)))
    assert _bits(grown, grown.optimize(10)) == _bits(fresh, fresh.optimize(10))
    grown.close(), fresh.close()


def test_a_pivot_that_is_not_positive_is_a_flag_and_an_exit():
    case = CASES["pair"]
    for g, kind in ((api.PoseGraph(), "device"), (O.OracleGraph(), "restatement")):
        for k in range(2):
            g.add_vertex(k, case.poses[k], case.fixed[k])
        g.add_edge(0, 1, case.edges[0][2], -np.eye(6))
        before = g.read_vertices().tobytes()
        res = g.optimize(10)
        assert (res.stop_reason, res.n_trials, res.iterations) == (api.PGO_STOP_MAX_TRIALS, 10, 1), kind
        assert all(t.accepted == 0 and t.chi2 == np.finfo(np.float64).max for t in res.trace[:10]), kind
        assert g.read_vertices().tobytes() == before and res.chi2_final == res.chi2_initial, kind
        if kind == "device":
            assert g.step(0.0)["pivot"] == 1 and not g.step(0.0)["delta"].any()
            g.close()


def test_errors_and_the_empty_graph():
    g = device_graph("loop24", max_band_bytes=1024)
    with pytest.raises(api.SlamError) as e:
        g.optimize(10)
    assert e.value.code == api.E_NOMEM and "max_band_bytes" in str(e.value)
    assert np.array_equal(g.read_vertices(), device_graph("loop24").read_vertices())
    g.close()
    case = CASES["chain8"]
    g = api.PoseGraph()
    for k in range(case.n):
        g.add_vertex(k, case.poses[k], False)
    for i, j, z, w in case.edges:
        g.add_edge(i, j, z, w)
    with pytest.raises(api.SlamError) as e:
        g.optimize(10)
    assert e.value.code == api.E_INVALID and "fixed" in str(e.value)
    g.close()
    g = api.PoseGraph()
    with pytest.raises(api.SlamError) as e:
        g.optimize(10)
    assert e.value.code == api.E_INVALID
    assert g.chi2()[0] == 0.0 and g.read_vertices().shape == (0, 7)
    g.add_vertex(0, [0, 0, 0, 0, 0, 0, 1], True)
    res = g.optimize(10)          # nothing is free: no iteration, no trial
    assert (res.iterations, res.n_trials, res.free_vertices, res.chi2_final) == (0, 0, 0, 0.0)
    g.close()


def _hip_runtime():
    api.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    rt = C.CDLL(paths[0])
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rt.hipMemGetInfo.restype = C.c_int
    return rt


def _free_bytes(rt):
    api.synchronize()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_two_hundred_lifetimes_leak_nothing():
    rt, first, after_ten = _hip_runtime(), None, None
    for k in range(200):
        g = device_graph("chain8")
        res = g.optimize(10)
        bits = _bits(g, res)
        g.close()
        first = first or bits
        assert bits == first
        if k == 9:
            after_ten = _free_bytes(rt)
    after = _free_bytes(rt)
    print("lifetime: free after 10 cycles %d, after 200 %d (drift %d)" % (after_ten, after, after_ten - after))
    assert after >= after_ten - (2 << 20)
