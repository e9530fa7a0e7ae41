"""slam_kf_* (slam_amd/csrc/kf_edge.hip) against the restatement on the branches benign clouds never take: the hand-worked
edges of tests/kf_edge_cases.py (reflected, planar, collinear and coincident pairs, one to three pairs, a pair at the gate,
every stop state, a NaN init), targets on both sides of the LDS staging boundary in one batch, and the gated search where
the lattice ends and in a crowded cell.  tests/test_kf_edge_cases.py shows on the CPU that the restatement reaches every
branch named here.  Bounds: docs/KF_EDGE.md section 6."""
import signal

import numpy as np
import pytest

import kf_edge_cases as KC
import kf_edge_oracle as K
from slam_amd import api
from test_gpu_kf_edge import ANG_TOL, CHAIN_TOL, MARGIN_TOL, POS_TOL, check_information, same_result

SOLVE_TOL = KC.SOLVE_TOL
TEST_SECONDS = 300
TRACE = 32
CASES = KC.cases()
NAMES = [c["name"] for c in CASES]


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


def param_key(c):
    return tuple(sorted(c["store"].items())) + tuple(sorted(c["icp"].items()))


class Keyframes:
    """A store and, per keyframe, the filtered cloud it holds and its restatement twin (built from the store's own cloud,
    as Scene of tests/test_gpu_kf_edge.py does)."""

    def __init__(self, **kw):
        self.store = api.KeyframeStore(**kw)
        self.filtered, self.ora = [], []

    def add(self, xyz, expect=None):
        kid = self.store.add_keyframe(xyz)
        assert kid == len(self.filtered)
        f = self.store.read_keyframe(kid)
        if expect is not None:
            assert self.store.info(kid)["n_points"] == len(f) == expect
        self.filtered.append(f)
        self.ora.append(K.OracleKeyframe(f[:, :3], self.store.params))
        return kid

    def oracle_edge(self, frm, to, init, **kw):
        return K.register_edge(self.ora[frm], self.filtered[to][:, :3], init, params=self.store.params, trace=TRACE, lum_detail=True, **kw)


class Groups:
    """One store per parameter set; the cases with setup_gicp's values share one."""

    def __init__(self):
        self.sets, self.where = {}, {}
        for c in CASES:
            key = param_key(c)
            if key not in self.sets:
                self.sets[key] = (Keyframes(**dict(key)), [])
            kfs, edges = self.sets[key]
            frm, to = kfs.add(c["tgt"], c["n_tgt"]), kfs.add(c["src"], c["n_src"])
            self.where[c["name"]] = (key, len(edges))
            edges.append((frm, to, c["init"]))
        self.cache = {}

    def alone(self, name):
        """the device's result for the case registered in a call of its own, and the restatement's"""
        if name not in self.cache:
            key, e = self.where[name]
            kfs, edges = self.sets[key]
            self.cache[name] = (kfs.store.register_edges([edges[e]], trace=TRACE)[0], kfs.oracle_edge(*edges[e]))
        return self.cache[name]


@pytest.fixture(scope="module")
def groups():
    return Groups()


def f32_of(t64):
    return np.asarray(t64, np.float64).astype(np.float32)


def same_f32(a, b):
    """bit-equal, a NaN standing for a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def step_rotation(T, init):
    """the product of the steps: total . init^-1 (an f32 init of a generic yaw is orthonormal to 1e-8 only)"""
    return np.asarray(T, np.float64)[:3, :3] @ np.linalg.inv(np.asarray(init, np.float64)[:3, :3])


def image(T, p):
    return np.asarray(p, np.float64)[:, :3] @ T[:3, :3].T + T[:3, 3]


def check_discrete(dev, ora):
    for k in ("iterations", "state", "converged", "pairs", "num_corr", "singular"):
        assert dev[k] == ora[k], (k, dev[k], ora[k])
    assert np.array_equal(dev["pairs_trace"], ora["pairs_trace"])


def check_lum(dev, ora):
    """the f32 transform is the rounded f64 one; LUM to its reassociation bounds, or the identity fallback of the same kind"""
    assert same_f32(dev["transform"], f32_of(dev["transform64"]))
    if dev["singular"] == 0:
        if same_f32(dev["transform"], ora["transform"]):
            check_information(dev, ora)
            return True
        return False
    assert ora["singular"] == 1 and np.array_equal(dev["information"], np.eye(6))
    ss_d, ss_o = float(dev["ss"]), float(ora["ss"])
    assert (ss_d < 1e-13 and ss_o < 1e-13) or (not np.isfinite(ss_d) and not np.isfinite(ss_o)), (ss_d, ss_o)
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hand_worked_edge_follows_the_restatement(groups, name):
    c = CASES[NAMES.index(name)]
    dev, ora = groups.alone(name)
    T, To = dev["transform64"], ora["transform64"]
    finite = np.isfinite(To)
    dT = np.abs(T - To)[finite].max()
    print("\n%-15s %d / %d iterations, state %d / %d, pairs %s / %s, margin %.3g, LUM n %d / %d ss %.3g / %.3g singular %d / %d, |dT| %.3g"
          % (name, dev["iterations"], ora["iterations"], dev["state"], ora["state"], dev["pairs_trace"][:dev["iterations"] + 1].tolist(),
             ora["pairs_trace"][:ora["iterations"] + 1].tolist(), ora["margin"], dev["num_corr"], ora["num_corr"], float(dev["ss"]),
             float(ora["ss"]), dev["singular"], ora["singular"], dT))
    assert ora["margin"] > MARGIN_TOL and ora["state"] == c["state"]     # (the CPU test holds the restatement to the whole case)
    stepped = dev["iterations"] > 0
    if c["name"] == "generic-plane":     # the rank of a noisy plane is not pinned: properties and the pose only
        dpos, dang = K.pose_error(T, To)
        print("    device - restatement %.3g m %.3g rad" % (dpos, dang))
        assert stepped and dev["state"] == api.KF_TRANSFORM and dpos < POS_TOL and dang < ANG_TOL
    else:
        check_discrete(dev, ora)
        assert np.array_equal(np.isfinite(T), finite) and dT < SOLVE_TOL
        assert dev["pairs_trace"][0] == ora["pairs_trace"][0] and (c["first"] is None or dev["pairs_trace"][0] == c["first"])
        if c["mse"] is not None:
            assert dev["mse"] == c["mse"]
        assert abs(dev["mse"] - ora["mse"]) <= 1e-12 * max(1.0, ora["mse"])
        if not stepped:
            assert np.array_equal(T, np.asarray(c["init"], np.float64), equal_nan=True)
        elif c["T"] is not None and c["image"]:
            src = groups.sets[groups.where[name][0]][0].filtered[2 * groups.where[name][1] + 1]
            assert np.abs(image(T, src) - image(c["T"], src)).max() < SOLVE_TOL
        elif c["T"] is not None:
            print("    |T - hand-worked| %.3g" % np.abs(T - c["T"]).max())
            assert np.abs(T - c["T"]).max() < SOLVE_TOL
    if stepped:     # whatever the restatement says: a proper rotation that fits the hand-worked pairs no worse
        R = step_rotation(T, c["init"])
        print("    steps: |R R' - I| %.3g, |det R - 1| %.3g" % (np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1)))
        assert np.abs(R @ R.T - np.eye(3)).max() < SOLVE_TOL and abs(np.linalg.det(R) - 1) < SOLVE_TOL
        if c["match"] is not None:
            res_d, res_o = KC.residual(T, c["match"]), KC.residual(To, c["match"])
            print("    residual of the hand-worked pairs %.6g / %.6g" % (res_d, res_o))
            assert res_d <= res_o + 1e-12
    lum = check_lum(dev, ora)
    if c["name"] != "generic-plane":
        assert lum or not c["exact"], "the f32 transforms of an exact case differ"
    if c["lum"] is not None:
        assert dev["singular"] == 1


@pytest.mark.gpu
def test_degenerate_edges_do_not_disturb_their_batch(groups):
    """Every case alone and all the cases of one store in one call, twice: the same bits, the traces included."""
    for key, (kfs, edges) in groups.sets.items():
        together = [kfs.store.register_edges(edges, trace=TRACE) for _ in range(2)]
        names = [n for n in NAMES if groups.where[n][0] == key]
        print("\nstore %s: %d edges in one call" % (dict(key), len(edges)))
        for e, name in enumerate(names):
            alone = groups.alone(name)[0]
            for other in (together[0][e], together[1][e]):
                assert same_result(alone, other), name
                assert np.array_equal(alone["pairs_trace"], other["pairs_trace"]), name


# ------------------------------------------------------------------ the LDS staging boundary and a really mixed batch
SHIFT = np.array([0.25, -0.125, 0.25])


@pytest.fixture(scope="module")
def lattices():
    """targets of 6 144 (= kLdsPoints), 6 145 and 64 points, each followed by its copy moved by a dyadic shift"""
    kfs = Keyframes()
    for n in (6144, 6145, 64):
        p = KC.counted_lattice(n)
        kfs.add(KC.exact_copy(p, np.eye(3), SHIFT), n)
        kfs.add(p, n)
    return kfs


@pytest.mark.gpu
def test_targets_on_both_sides_of_the_lds_boundary_in_one_batch(lattices):
    """tgt.n == lds_points, lds_points + 1 and far below, in one call (the dynamic LDS is sized by one edge and used by
    another, the 6 145-point target is read through L2 beside them), through L2 altogether, and each alone (with only the
    6 145-point target no target fits: no dynamic LDS at all).  Results, not paths: all the same bits, and the restatement's."""
    store = lattices.store
    edges = [(0, 1, np.eye(4)), (2, 3, np.eye(4)), (4, 5, np.eye(4))]
    assert [store.info(f)["n_points"] for f, _, _ in edges] == [6144, 6145, 64]
    runs = {}
    for lds in (1, 0):
        store.set_params(target_in_lds=lds)
        runs["batch", lds] = store.register_edges(edges, trace=TRACE)
        runs["reversed", lds] = store.register_edges(edges[::-1], trace=TRACE)[::-1]
        runs["alone", lds] = [store.register_edges([e], trace=TRACE)[0] for e in edges]
    store.set_params(target_in_lds=1)
    want = KC.T_of(np.eye(3), SHIFT)
    for e, (frm, to, init) in enumerate(edges):
        ref = runs["batch", 1][e]
        for k, r in runs.items():
            assert same_result(ref, r[e]) and np.array_equal(ref["pairs_trace"], r[e]["pairs_trace"]), (k, e)
        ora = lattices.oracle_edge(frm, to, init)
        n = store.info(frm)["n_points"]
        print("\ntarget of %d points: %d iterations, state %d, pairs %s, |dT| %.3g, |T - hand-worked| %.3g" %
              (n, ref["iterations"], ref["state"], ref["pairs_trace"][:3].tolist(), np.abs(ref["transform64"] - ora["transform64"]).max(),
               np.abs(ref["transform64"] - want).max()))
        check_discrete(ref, ora)
        assert (ref["iterations"], ref["state"], ref["pairs"]) == (2, api.KF_TRANSFORM, n) and ora["margin"] > MARGIN_TOL
        assert np.abs(ref["transform64"] - ora["transform64"]).max() < SOLVE_TOL and np.abs(ref["transform64"] - want).max() < SOLVE_TOL
        assert check_lum(ref, ora) and ref["singular"] == 1


# ------------------------------------------------------------------ the search where the lattice ends, and crowded cells
PLACEMENTS = KC.placements(api.kf_default_params())
BAD_QUERIES = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.inf]], np.float32)


@pytest.fixture(scope="module")
def boxes():
    kfs = Keyframes()
    for centre in PLACEMENTS.values():
        kfs.add(KC.box_cloud(centre))
    return kfs


def check_search(kfs, kid, q, strict):
    f = kfs.filtered[kid]
    gi, gd = kfs.store.nearest(kid, q, strict=strict)
    bi, bd = K.brute_force(f, q, kfs.store.params.gate, strict)
    oi, od = kfs.ora[kid].nearest(q, strict=strict)
    assert np.array_equal(oi, bi) and np.array_equal(od.view(np.uint32), bd.view(np.uint32))
    assert np.array_equal(gi, bi)
    assert np.array_equal(gd.view(np.uint32), bd.view(np.uint32))
    return int((bi >= 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_gated_search_equals_brute_force_where_the_lattice_ends(boxes, name, strict):
    """cell_coord's clamp at +-2^20 cells, nearest27 without its pruning for a clamped coordinate, the neighbours outside
    [0, 2^21) skipped, and the cell that every clamped coordinate shares"""
    kid = list(PLACEMENTS).index(name)
    centre, f, info = PLACEMENTS[name], boxes.filtered[kid], boxes.store.info(kid)
    q = KC.box_queries(f, centre)
    kept = check_search(boxes, kid, q, strict)
    print("\n%s: %s, kept %d of %d" % (name, info, kept, len(q)))
    assert kept >= len(q) // 4
    assert (info["n_cells"], info["max_cell_points"]) == boxes.ora[kid].stats()
    if name == "origin":     # both signs of every coordinate, queries in cells -1 and 0
        assert all((f[:, k] < 0).any() and (f[:, k] > 0).any() for k in range(3))
        assert all(((q[:, k] > -0.75) & (q[:, k] < 0)).any() and ((q[:, k] >= 0) & (q[:, k] < 0.75)).any() for k in range(3))
    if name == "corner":
        assert info["max_cell_points"] >= 500
    if name == "beyond":
        assert info["max_cell_points"] == info["n_points"]
    bad = BAD_QUERIES + np.where(np.isfinite(BAD_QUERIES), np.float32(centre), 0).astype(np.float32)
    gi, gd = boxes.store.nearest(kid, bad, strict=strict)
    assert (gi == -1).all() and (gd == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_gated_search_in_one_crowded_cell(strict):
    """2 000 points in one lattice cell: the serial count of kf_table_kernel, the long run scanned by every query"""
    kfs = Keyframes(leaf_size=KC.ONE_CELL_LEAF)
    kid = kfs.add(KC.one_cell_cloud(), 2000)
    info = kfs.store.info(kid)
    assert (info["n_cells"], info["max_cell_points"]) == (1, 2000)
    q = KC.box_queries(kfs.filtered[kid], (0.375, 0.375, 0.15625), n=5000, side=1.0, sigma=0.4)
    kept = check_search(kfs, kid, q, strict)
    print("\none cell: %s, kept %d of %d" % (info, kept, len(q)))
    assert kept >= len(q) // 4
    gi, gd = kfs.store.nearest(kid, BAD_QUERIES, strict=strict)
    assert (gi == -1).all() and (gd == 0).all()


@pytest.mark.gpu
def test_an_edge_at_the_corner_of_the_lattice():
    """Three iterations with the stop rules off between a cloud about (+B, -B, +B) and its copy a dyadic shift away:
    move_f64 and the centroids at 7.9e5 m, an eighth of the target in each octant of the clamp.  2 048 pairs of multiples of
    1/16: the sums are exact, so CHAIN_TOL is not eaten by 7.9e5 m times the reassociation of H (between two random clouds
    there, permuting the source moves the restatement's own transform by 1e-9 to 5e-9)."""
    kfs = Keyframes(max_iterations=3, transformation_epsilon=-1.0, fitness_epsilon=-1.0)
    p = KC.corner_lattice(kfs.store.params)
    frm, to = kfs.add(KC.exact_copy(p, np.eye(3), SHIFT), 2048), kfs.add(p, 2048)
    info = kfs.store.info(frm)
    assert info["max_cell_points"] >= 2048 // 8     # the octant beyond all three clamps is one cell
    dev = kfs.store.register_edges([(frm, to, np.eye(4))], trace=TRACE)[0]
    ora = kfs.oracle_edge(frm, to, np.eye(4))
    dT = np.abs(dev["transform64"] - ora["transform64"]).max()
    print("\ncorner edge: %s; pairs %s / %s, |dT| %.3g, |T - hand-worked| %.3g" % (info, dev["pairs_trace"][:4].tolist(),
          ora["pairs_trace"][:4].tolist(), dT, np.abs(dev["transform64"] - KC.T_of(np.eye(3), SHIFT)).max()))
    check_discrete(dev, ora)
    assert dev["pairs_trace"][:4].tolist() == [2048, 2048, 2048, -1] and (dev["iterations"], dev["state"]) == (3, api.KF_ITERATIONS)
    assert dT < CHAIN_TOL
    assert np.abs(dev["transform64"][:3, :3] - np.eye(3)).max() < SOLVE_TOL     # the shift itself carries 7.9e5 m of R's rounding
    assert check_lum(dev, ora)
