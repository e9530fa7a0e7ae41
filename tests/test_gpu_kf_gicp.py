"""slam_kf_compute_covariances and slam_kf_register_gicp (slam_amd/csrc/kf_gicp.hip) against the scalar restatement
tests/cpp/kf_gicp_oracle.cpp: neighbour lists and covariances bit for bit, the iteration with and without its stop rule,
the hand-worked requests of tests/kf_gicp_cases.py, batch independence, the LDS boundary, the untouched ICP path and the
argument errors.  Bounds: docs/KF_GICP.md section 5."""
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import kf_edge_oracle as K
import kf_gicp_cases as G
import kf_gicp_oracle as O
from slam_amd import api

POS_TOL, ANG_TOL = 1e-4, 1e-5   # BASELINE.json, as tests/test_gpu_icp.py
CHAIN_TOL = 1e-9                # reassociated f64 sums and nothing else (tests/test_gpu_icp.py:86)
MARGIN_TOL = 1e-9
TEST_SECONDS = 300


@pytest.fixture(autouse=True)
def time_limit():
    """Every test here ends after TEST_SECONDS, and the session with it: nothing more is started on the GPU."""
    def expired(signum, frame):
        pytest.exit("GPU test exceeded %d s" % TEST_SECONDS, returncode=3)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_edge(a, b):
    """Every field of a slam_kf_edge_result, and the trace where there is one, the same bits."""
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("transform", "transform64", "information")) and \
        all(a[k] == b[k] for k in ("iterations", "state", "converged", "pairs", "num_corr", "singular")) and \
        np.array_equal(bits(np.float64(a["mse"])), bits(np.float64(b["mse"]))) and \
        np.array_equal(bits(np.float32(a["ss"])), bits(np.float32(b["ss"]))) and \
        ("pairs_trace" not in a or np.array_equal(a["pairs_trace"], b["pairs_trace"]))


def same_result(a, b):
    return same_edge(a, b) and np.array_equal(bits(a["hessian"]), bits(b["hessian"])) and a["fitness_pairs"] == b["fitness_pairs"] and \
        all(np.array_equal(bits(np.float64(a[k])), bits(np.float64(b[k]))) for k in ("cost", "fitness"))


class Store:
    """Clouds in a store with GICP parameters, and their restatement twins built from the store's filtered clouds."""

    def __init__(self, clouds, store=None, gicp=None, twins=True):
        self.store = api.KeyframeStore(**(store or {}))
        self.gp = api.kf_gicp_default_params(**(gicp or {}))
        self.store.set_gicp_params(self.gp)
        self.filtered, self.ora = [], []
        for c in clouds:
            kid = self.store.add_keyframe(c)
            f = self.store.read_keyframe(kid)[:, :3]
            self.filtered.append(f)
            self.ora.append(O.OracleCloud(f, self.store.params, self.gp) if twins else None)

    def oracle(self, frm, to, init, gp=None, **kw):
        return O.register_gicp(self.ora[frm], self.ora[to], init, gp or self.gp, **kw)


# ------------------------------------------------------------------ neighbour lists and covariances
def crowded(n, seed):
    return (np.random.RandomState(seed).uniform(0.05, 0.35, (n, 3))).astype(np.float32)


Q = dict(leaf_size=0.25)   # jittered_cloud's voxels

SHAPES = {
    # name: (cloud, store parameters, gicp parameters)
    "n20": lambda: (G.jittered_cloud(20, 20, 12), Q, {}),
    "n21": lambda: (G.jittered_cloud(21, 21, 12), Q, {}),
    "n63": lambda: (G.jittered_cloud(63, 63, 12), Q, {}),
    "n64": lambda: (G.jittered_cloud(64, 64, 12), Q, {}),
    "n65": lambda: (G.jittered_cloud(65, 65, 12), Q, {}),
    "n257": lambda: (G.jittered_cloud(257, 257, 16), Q, {}),
    "ties": lambda: (G.lattice_cloud(300, 3), dict(leaf_size=2.0 ** -5), dict(cov_radius=0.4)),
    "k32": lambda: (G.jittered_cloud(400, 32, 16), Q, dict(k_correspondences=32, cov_radius=3.0)),
    "crowded-cell": lambda: (crowded(2000, 7), dict(leaf_size=2.0 ** -9), {}),
    "sparse": lambda: (np.concatenate([G.jittered_cloud(570, 9, 200), G.jittered_cloud(30, 10, 5) + np.float32(60)]), Q, {}),
    "keyframe-leaf-0.5": lambda: (K.cloud(2)[0], {}, {}),
    "keyframe-leaf-1.5-gate-10": lambda: (K.cloud(2)[0], dict(leaf_size=1.5, gate=10.0), {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_neighbour_lists_and_covariances_equal_the_restatement(shape):
    cloud, store, gicp = SHAPES[shape]()
    s = Store([cloud], store, gicp)
    s.store.compute_covariances(0)
    s.store.compute_covariances(0)      # idempotent
    idx, d2, cnt = s.store.neighbours(0)
    cov = s.store.covariances(0)
    o = s.ora[0]
    info = s.store.info(0)
    identity = int((cnt < s.gp.cov_min_neighbours).sum())
    print("%s: %d points, %d cells, fullest %d; lists %d..%d long, %d full, %d identity covariances" %
          (shape, len(cnt), info["n_cells"], info["max_cell_points"], cnt.min(), cnt.max(), (cnt == s.gp.k_correspondences).sum(), identity))
    if shape[0] == "n":
        assert len(cnt) == int(shape[1:])
    if shape == "crowded-cell":
        assert info["max_cell_points"] == len(cnt) >= 1990
    if shape == "sparse":
        assert identity > len(cnt) // 2 and identity < len(cnt)
    if shape == "keyframe-leaf-1.5-gate-10":
        assert info["n_cells"] <= 60 and info["max_cell_points"] >= 30     # a few dozen cells of dozens of points (39 and 48 on the CPU)
    assert np.array_equal(cnt, o.count)
    assert np.array_equal(idx, o.index)
    assert np.array_equal(d2.view(np.uint32), o.dist2.view(np.uint32))
    assert np.array_equal(cov.view(np.uint64), o.cov.view(np.uint64))


# ------------------------------------------------------------------ make_cloud3d edges
KS = (0, 1, 2, 4)


class Scene(Store):
    def __init__(self, **gicp):
        self.poses = [K.cloud(k)[1] for k in KS]
        super().__init__([K.cloud(k)[0] for k in KS], None, gicp)

    def init(self, to, perturb=K.PERTURB):
        return K.relative_init(self.poses[0], self.poses[to], perturb)


@pytest.fixture(scope="module")
def scene():
    return Scene()


PERMS = (1, 2, 3)   # seeds of the three fixed permutations of the source points


@pytest.mark.gpu
@pytest.mark.parametrize("to", [1, 2, 3])
def test_fixed_iterations_follow_the_restatement(scene, to):
    """Stop rule off (negative epsilons): pairs of every iteration equal; total transform within max(1e-9, 10 s), s the
    largest move of the restatement's own result under three fixed permutations of the source points."""
    init = scene.init(to)
    n = len(scene.filtered[to])
    for iters in (1, 2, 5):
        gp = api.kf_gicp_default_params(max_iterations=iters, transformation_epsilon=-1.0, rotation_epsilon=-1.0)
        dev = scene.store.register_gicp([(0, to, init)], params=gp, trace=8)[0]
        ora = scene.oracle(0, to, init, gp, trace=8)
        s = 0.0
        for seed in PERMS:
            perm = np.random.RandomState(seed).permutation(n)
            s = max(s, np.abs(scene.oracle(0, to, init, gp, order=perm)["transform64"] - ora["transform64"]).max())
        bound = max(CHAIN_TOL, 10 * s)
        err = np.abs(dev["transform64"] - ora["transform64"]).max()
        print("edge 0-%d, %d iterations: pairs %s, |dT| = %.3g, permutation spread s = %.3g, bound %.3g" %
              (KS[to], iters, dev["pairs_trace"][:iters], err, s, bound))
        assert (dev["iterations"], dev["state"], dev["converged"]) == (iters, api.KF_ITERATIONS, 1)
        assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"]) and dev["pairs"] == ora["pairs"]
        assert err <= bound
    scene.store.set_gicp_params(scene.gp)


def check_sums(dev, ora, n):
    """fitness and cost, and the LUM block's counters, where the f32 transforms are the same bits: True when checked."""
    if not np.array_equal(bits(dev["transform"]), bits(ora["transform"])):
        return False
    assert dev["fitness_pairs"] == ora["fitness_pairs"] == dev["num_corr"] == ora["num_corr"]
    # the same f32 terms summed in another order: n 2^-53 sum|term| on the sum
    assert abs(dev["fitness"] - ora["fitness"]) * ora["fitness_pairs"] <= n * 2.0 ** -53 * ora["fitness_sum"]
    assert dev["singular"] == ora["singular"]
    assert abs(float(dev["ss"]) - float(ora["ss"])) <= n * 2.0 ** -24 * abs(float(ora["ss"]))
    return True


@pytest.mark.gpu
def test_default_settings_follow_the_restatement(scene):
    excused, checked = 0, 0
    for to in (1, 2, 3):
        init = scene.init(to)
        dev = scene.store.register_gicp([(0, to, init)], params=scene.gp, trace=16)[0]
        ora = scene.oracle(0, to, init, trace=16)
        dp, da = K.pose_error(dev["transform64"], ora["transform64"])
        truth = K.true_relative(scene.poses[0], scene.poses[to])
        n = len(scene.filtered[to])
        rel_cost = abs(dev["cost"] - ora["cost"]) / ora["cost"]
        print("edge 0-%d: %d iterations (restatement %d), state %d (%d), margin %.3g, pose %.3g m %.3g rad from the restatement, "
              "%.3g m %.3g rad from the truth; cost %.6g (%.3g relative), fitness %.6g over %d" %
              ((KS[to], dev["iterations"], ora["iterations"], dev["state"], ora["state"], ora["margin"], dp, da) +
               K.pose_error(dev["transform64"], truth) + (dev["cost"], rel_cost, dev["fitness"], dev["fitness_pairs"])))
        if (dev["iterations"], dev["state"]) != (ora["iterations"], ora["state"]):
            assert ora["margin"] < MARGIN_TOL
            excused += 1
            continue
        assert dp <= POS_TOL and da <= ANG_TOL
        assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"]) and dev["pairs"] == ora["pairs"]
        assert rel_cost <= n * 2.0 ** -24
        checked += check_sums(dev, ora, n)
    assert excused <= 1 and checked >= 1


# ------------------------------------------------------------------ the hand-worked requests
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_hand_worked_cases_equal_the_restatement(name):
    c = G.CASES[name]
    s = Store([c["target"], c["source"]], c["store"], c["gicp"])
    assert [len(f) for f in s.filtered] == [len(c["target"]), len(c["source"])]     # every point its own voxel
    init = np.asarray(c["init"], np.float32)
    dev = s.store.register_gicp([(0, 1, init)], trace=32)[0]
    again = s.store.register_gicp([(0, 1, init), (0, 1, init)], trace=32)
    ora = s.oracle(0, 1, init, trace=32)
    both = np.stack([dev["transform64"], ora["transform64"]])
    nan = np.isnan(both)
    assert np.array_equal(nan[0], nan[1])
    err = float(np.abs(both[0] - both[1])[~nan[0]].max())
    print("%s: state %d, %d iterations, pairs %s, |dT| = %.3g" % (name, dev["state"], dev["iterations"], dev["pairs_trace"][:dev["iterations"] + 1], err))
    assert ora["margin"] > MARGIN_TOL
    for k in ("state", "iterations", "converged", "pairs", "fitness_pairs", "num_corr", "singular"):
        assert dev[k] == ora[k], k
    assert (dev["state"], dev["pairs"]) == (c["state"], c["pairs"])
    assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"])
    assert err <= 1e-12
    assert np.array_equal(bits(dev["transform"]), bits(dev["transform64"].astype(np.float32)))
    if c["truth"] is not None and c["state"] == api.KF_TRANSFORM:
        assert np.abs(dev["transform64"] - c["truth"]).max() <= c.get("truth_tol", 1e-12)
    if c.get("exact"):
        assert np.array_equal(bits(dev["hessian"]), bits(ora["hessian"])) and dev["cost"] == ora["cost"]
    assert same_result(dev, again[0]) and same_result(dev, again[1])


@pytest.mark.gpu
def test_pair_at_the_gate_is_dropped_here_and_kept_by_the_icp_edge():
    c = G.CASES["gate"]
    s = Store([c["target"], c["source"]], c["store"], c["gicp"])
    init = np.eye(4, dtype=np.float32)
    g = s.store.register_gicp([(0, 1, init)], trace=4)[0]
    e = s.store.register_edges([(0, 1, init)], trace=4)[0]
    assert g["pairs_trace"][0] == 0 and g["state"] == api.KF_NO_CORRESPONDENCES and g["fitness_pairs"] == 0
    assert e["pairs_trace"][0] == 8


# ------------------------------------------------------------------ batches
def starts(scene, to, n, seed):
    rs = np.random.RandomState(seed)
    return [scene.init(to, (rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4), rs.uniform(-0.06, 0.06))) for _ in range(n)]


@pytest.mark.gpu
def test_twenty_starts_alone_and_together_give_the_same_bits(scene):
    inits = starts(scene, 1, 20, 4)
    scene.store.set_gicp_params(scene.gp)
    alone = [scene.store.register_gicp([(0, 1, m)], trace=16)[0] for m in inits]
    for _ in range(2):
        together = scene.store.register_gicp([(0, 1, m) for m in inits], trace=16)
        assert all(same_result(a, b) for a, b in zip(alone, together))
    print("iterations of the 20 starts: %s" % [r["iterations"] for r in alone])
    assert len({r["transform64"].tobytes() for r in alone}) > 1


def sheet(n):
    """n points half a metre apart on a gently folded sheet, every one its own voxel at leaf 1/8."""
    i = np.arange(n)
    return np.stack([0.5 * (i % 80), 0.5 * (i // 80), 0.125 * ((i * 7) % 5)], 1).astype(np.float32)


@pytest.mark.gpu
def test_targets_at_the_lds_boundary_staged_and_through_l2():
    """Targets of 6 144 (the last that is staged) and 6 145 points in one call: the same bits whether the store stages or not,
    and the restatement's pairs."""
    src = sheet(600) + np.float32(1 / 16)
    s = Store([sheet(6144), sheet(6145), src], dict(leaf_size=0.125), dict(k_correspondences=8, cov_radius=1.2, max_iterations=4))
    assert [len(f) for f in s.filtered] == [6144, 6145, 600]
    init = np.eye(4, dtype=np.float32)
    req = [(0, 2, init), (1, 2, init)]
    staged = s.store.register_gicp(req, trace=8)
    s.store.set_params(target_in_lds=0)
    through = s.store.register_gicp(req, trace=8)
    s.store.set_params(target_in_lds=1)
    alone = [s.store.register_gicp([r], trace=8)[0] for r in req]
    for e in range(2):
        assert same_result(staged[e], through[e]) and same_result(staged[e], alone[e])
        ora = s.oracle(e, 2, init, trace=8)
        assert np.array_equal(staged[e]["pairs_trace"], ora["pairs_trace"]) and staged[e]["pairs"] == 600
        assert (staged[e]["state"], staged[e]["iterations"]) == (ora["state"], ora["iterations"])
        assert np.abs(staged[e]["transform64"] - ora["transform64"]).max() <= CHAIN_TOL


@pytest.mark.gpu
def test_icp_edges_are_the_same_bits_before_and_after_covariances():
    store = api.KeyframeStore()
    poses = []
    for k in (0, 1):
        xyz, pose = K.cloud(k)
        store.add_keyframe(xyz)
        poses.append(pose)
    init = K.relative_init(poses[0], poses[1])
    before = store.register_edges([(0, 1, init)], trace=64)[0]
    store.compute_covariances(0)
    store.compute_covariances(1)
    store.register_gicp([(0, 1, init)])
    after = store.register_edges([(0, 1, init)], trace=64)[0]
    for k in ("transform", "transform64", "information", "pairs_trace"):
        assert np.array_equal(bits(before[k]), bits(after[k])), k
    for k in ("iterations", "state", "converged", "pairs", "mse", "num_corr", "singular", "ss"):
        assert before[k] == after[k], k


ORDERS = {"gicp-first": ("gicp", "icp"), "icp-first": ("icp", "gicp")}
ORDER_CHILD = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_kf_gicp as t; t.order_child(sys.argv[1], sys.argv[2])"


def order_request():
    poses = [K.cloud(k)[1] for k in (0, 1)]
    return [(0, 1, K.relative_init(poses[0], poses[1]))]


def order_run(solvers):
    """A fresh store with keyframes 0 and 1, then one request per solver in the order given: {solver: result}."""
    store = api.KeyframeStore()
    for k in (0, 1):
        store.add_keyframe(K.cloud(k)[0])
    assert 4096 < store.info(0)["n_points"] <= 6144      # the target: more dynamic LDS than the default 64 KB
    req = order_request()
    return {s: (store.register_gicp(req, trace=16) if s == "gicp" else store.register_edges(req, trace=64))[0] for s in solvers}


def order_child(order, path):
    """What a child process of the test below runs: its own first launches of both kernels, results to an .npz."""
    api.set_device(0)
    got = order_run(ORDERS[order])
    np.savez(path, **{"%s/%s" % (s, k): np.asarray(v) for s, r in got.items() for k, v in r.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_either_solver_first_in_a_fresh_process_gives_what_each_gives_alone(order, tmp_path):
    """The two kernels share a host path that raises each kernel's dynamic-LDS limit under that kernel's own flag.  Only a
    target of 4 097 .. 6 144 points asks for more than the default 64 KB, and the limit, once raised, holds for the kernel in
    the whole process, whichever store raised it.  So each order runs in a child process of its own, where neither kernel has
    been launched before: a flag set by the other solver would leave the second kernel at the default limit and its launch
    refused (the child then fails).  The child's results are the bits of the same requests made here, each on its own store."""
    tests = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "results.npz")
    child = subprocess.run([sys.executable, "-c", ORDER_CHILD % (os.path.dirname(tests), tests), order, out],
                           capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    z = np.load(out)
    got = {s: {k.split("/")[1]: z[k][()] for k in z.files if k.startswith(s + "/")} for s in ORDERS[order]}
    gicp_alone, icp_alone = order_run(["gicp"])["gicp"], order_run(["icp"])["icp"]
    assert gicp_alone["pairs"] > 1000 and icp_alone["pairs"] > 1000
    assert same_result(got["gicp"], gicp_alone) and same_edge(got["icp"], icp_alone)


# ------------------------------------------------------------------ refusals
def refused(call):
    with pytest.raises(api.SlamError) as e:
        call()
    assert e.value.code == api.E_INVALID


@pytest.mark.gpu
def test_refusals_are_error_codes():
    store = api.KeyframeStore(leaf_size=0.25)
    small = store.add_keyframe(G.jittered_cloud(19, 1, 8))
    big = store.add_keyframe(G.jittered_cloud(40, 2, 8))
    init = np.eye(4, dtype=np.float32)
    refused(lambda: store.compute_covariances(small))        # fewer than k points, as PCL refuses them
    refused(lambda: store.compute_covariances(-1))
    refused(lambda: store.covariances(big))                   # none yet
    refused(lambda: store.neighbours(big))
    refused(lambda: store.set_gicp_params(k_correspondences=33))
    store.set_gicp_params(cov_radius=100.0)                   # more than eight lattice edges
    refused(lambda: store.compute_covariances(big))
    store.set_gicp_params()
    refused(lambda: store.register_gicp([(big, 7, init)]))    # an unknown keyframe
    refused(lambda: store.register_gicp([(big, small, init)]))
    store.compute_covariances(big)
    refused(lambda: store.set_gicp_params(k_correspondences=10))   # fixed once a keyframe holds covariances
    store.set_gicp_params(max_iterations=3)                   # the iteration's own parameters stay free
    r = store.register_gicp([(big, big, init)])[0]
    assert r["state"] in (api.KF_ITERATIONS, api.KF_TRANSFORM) and r["pairs"] == 40
