"""The restatement (tests/cpp/kf_edge_oracle.cpp) on the hand-worked edges of tests/kf_edge_cases.py: every case reaches
the branch it was built for -- rank and orientation of the first iteration's H, stop state, iterations, pairs, the way LUM
falls back -- and the closed-form transform where there is one.  This is what keeps tests/test_gpu_kf_edge_branches.py
honest: a case that no longer reaches its branch fails here, on the reference alone.  Also the restatement's gated search
against brute force where the lattice ends and in a crowded cell.  No GPU needed."""
import numpy as np
import pytest

import kf_edge_cases as KC
import kf_edge_oracle as K
import oracle_lib as O
from slam_amd import api

SOLVE_TOL = KC.SOLVE_TOL
MARGIN_TOL = 1e-9            # as tests/test_gpu_kf_edge.py
CASES = KC.cases()
STATE_NAMES = {api.KF_ITERATIONS: "ITERATIONS", api.KF_TRANSFORM: "TRANSFORM", api.KF_ABS_MSE: "ABS_MSE", api.KF_REL_MSE: "REL_MSE",
               api.KF_NO_CORRESPONDENCES: "NO_CORRESPONDENCES"}


def filtered(xyz, leaf):
    f = O.voxel_downsample(np.hstack([xyz, np.zeros((len(xyz), 1), np.float32)]), leaf=(leaf, leaf, leaf))[0]
    return np.ascontiguousarray(f[:, :3])


def moved_f64(T, p):
    """the source under the total transform as the contract moves it: in double, left to right, rounded to f32 once"""
    T, p = np.asarray(T, np.float64), p.astype(np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def rows(a):
    return [tuple(float(v) for v in r) for r in np.asarray(a)[:, :3]]


def walk(c):
    """One case through the restatement: what it reached, as a dict; every expectation of the case asserted."""
    leaf = c["store"].get("leaf_size", 0.5)
    params = K.default_params(leaf_size=leaf, **c["icp"])
    src, tgt = filtered(c["src"], leaf), filtered(c["tgt"], leaf)
    if c["n_src"] is not None:   # the filter keeps every point, as it is
        assert (len(src), len(tgt)) == (c["n_src"], c["n_tgt"])
        assert sorted(rows(src)) == sorted(rows(c["src"])) and sorted(rows(tgt)) == sorted(rows(c["tgt"]))
    kf = K.OracleKeyframe(tgt, params)
    # the first iteration's pairs, and the branch of the solver they take
    m = moved_f64(c["init"], src)
    idx, d2 = kf.nearest(m, strict=False)
    keep = idx >= 0
    P, Q = m[keep], tgt[idx[keep]]
    if c["first"] is not None:
        assert keep.sum() == c["first"]
    if c["match"] is not None and c["exact"]:   # the pairing is the hand-worked one
        want = dict(zip(rows(c["match"][0]), rows(c["match"][1])))
        assert {s: q for s, q in zip(rows(src[keep]), rows(Q))} == want
    rank = sign = None
    if keep.sum() >= 3:
        R, t, rank = K.solve(P, Q)
        sign = KC.solver_sign(KC.cross_covariance(P, Q), rank)
        assert np.abs(R @ R.T - np.eye(3)).max() < SOLVE_TOL and abs(np.linalg.det(R) - 1) < SOLVE_TOL
        if c["exact"] or c["rank"] is not None:
            assert (rank, sign) == (c["rank"], c["sign"])
    else:
        assert c["rank"] is None
    r = K.register_edge(kf, src, c["init"], params=params, trace=32)
    T = r["transform64"]
    print("%-15s rank %s sign %s: %s after %d iterations, pairs %s, margin %.3g; LUM n %d ss %.3g singular %d" %
          (c["name"], rank, sign, STATE_NAMES[r["state"]], r["iterations"], r["pairs_trace"][:r["iterations"] + 1].tolist(), r["margin"],
           r["num_corr"], float(r["ss"]), r["singular"]))
    assert r["state"] == c["state"] and r["converged"] == (c["state"] != api.KF_NO_CORRESPONDENCES)
    if c["iterations"] is not None:
        assert r["iterations"] == c["iterations"]
    assert r["margin"] > MARGIN_TOL          # no stop test is close: the device must decide every one the same way
    if c["pairs"] is not None:
        assert r["pairs"] == c["pairs"] and r["num_corr"] == c["num_corr"]
        assert r["pairs_trace"][0] == c["first"]
    if r["state"] == api.KF_NO_CORRESPONDENCES:
        assert r["iterations"] == 0 and r["pairs"] < 3 and r["pairs_trace"][1] == -1
        assert np.array_equal(T, np.asarray(c["init"], np.float64), equal_nan=True)     # init returned as it came
    if c["singular"] is not None:
        assert r["singular"] == c["singular"]
    if r["singular"]:
        assert np.array_equal(r["information"], np.eye(6))
    ss = float(r["ss"])
    if c["lum"] == "ss":
        assert r["num_corr"] > 0 and ss < 1e-13
    elif c["lum"] == "nonfinite":
        assert r["num_corr"] > 0 and not np.isfinite(ss)
    elif c["lum"] == "nopairs":
        assert r["num_corr"] == 0 and ss == 0.0
    if c["mse"] is not None:
        assert r["mse"] == c["mse"]
    if r["iterations"] > 0:     # the product of the steps (the f32 init of a generic yaw is orthonormal to 1e-8 only)
        Rt = T[:3, :3] @ np.linalg.inv(np.asarray(c["init"], np.float64)[:3, :3])
        assert np.abs(Rt @ Rt.T - np.eye(3)).max() < SOLVE_TOL and abs(np.linalg.det(Rt) - 1) < SOLVE_TOL
    if c["T"] is not None and c["exact"]:
        if c["image"]:    # the pairs pin the image of the source, not the roll about the line
            got = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            want = src.astype(np.float64) @ c["T"][:3, :3].T + c["T"][:3, 3]
            assert np.abs(got - want).max() < SOLVE_TOL
        else:
            assert np.array_equal(T, c["T"], equal_nan=True) or np.abs(T - c["T"]).max() < SOLVE_TOL
    if c["match"] is not None and r["iterations"] > 0:
        res = KC.residual(T, c["match"])
        if c["T"] is not None:     # no worse than the hand-worked transform
            assert res <= KC.residual(c["T"], c["match"]) + (SOLVE_TOL if c["exact"] else 1e-9)
        if c["exact"] and c["T"] is not None and c["state"] != api.KF_ITERATIONS:   # the last iteration's pairs, in place
            assert abs(r["mse"] - res) < SOLVE_TOL
    return dict(rank=rank, sign=sign, state=r["state"], iterations=r["iterations"], pairs=r["pairs"], lum=c["lum"] if r["singular"] else None,
                num_corr=r["num_corr"], R=T[:3, :3])


@pytest.fixture(scope="module")
def reached():
    return {}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_reaches_its_branch(c, reached):
    reached[c["name"]] = walk(c)


def test_mirrored_slabs_get_a_proper_rotation_close_to_the_identity():
    """det H < 0 on 64 pairs: the fixed sign keeps R proper (a reflection would fit exactly, and is refused)"""
    for c in CASES[:2]:
        got = walk(c)
        # a slab 16 m wide and a quarter of a metre thick: the best proper rotation is a small one
        assert got["sign"] == -1 and np.linalg.det(got["R"]) > 0 and np.abs(got["R"] - np.eye(3)).max() < 0.1


def test_the_cases_cover_every_branch(reached):
    """rank 3 and 2 with both orientations, rank 1 and 0, the five stop states, 0 to 3 pairs, and LUM falling back by ss ~ 0,
    by a non-finite D and by having no pairs"""
    for c in CASES:
        if c["name"] not in reached:
            reached[c["name"]] = walk(c)
    exact = [reached[c["name"]] for c in CASES if c["exact"] or c["rank"] is not None]
    assert {(r["rank"], r["sign"]) for r in exact if r["rank"] is not None} >= {(3, 1), (3, -1), (2, 1), (2, -1), (1, 1), (0, 1)}
    assert {r["state"] for r in exact} == set(STATE_NAMES)
    assert {r["pairs"] for r in exact} >= {0, 1, 2, 3}
    assert {r["lum"] for r in exact} >= {"ss", "nonfinite", "nopairs", None}
    one = reached["one-pair"]
    assert (one["num_corr"], one["lum"]) == (1, "nonfinite")
    line = reached["line"]
    assert (line["num_corr"], line["lum"]) == (16, "nonfinite")     # a really singular MM with pairs present


# ------------------------------------------------------------------ the search where the lattice ends, and a crowded cell
PLACEMENTS = KC.placements(K.default_params())


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_restatement_search_equals_brute_force_where_the_lattice_ends(name):
    centre = PLACEMENTS[name]
    f = filtered(KC.box_cloud(centre), 0.5)
    kf = K.OracleKeyframe(f)
    q = KC.box_queries(f, centre)
    cells, max_cell = kf.stats()
    for strict in (False, True):
        oi, od = kf.nearest(q, strict=strict)
        bi, bd = K.brute_force(f, q, 0.75, strict)
        assert np.array_equal(oi, bi) and np.array_equal(od.view(np.uint32), bd.view(np.uint32))
    print("%s: %d points, %d cells, largest %d, kept %d of %d" % (name, len(f), cells, max_cell, (bi >= 0).sum(), len(q)))
    assert (bi >= 0).sum() >= len(q) // 4
    if name == "corner":
        assert max_cell >= 500
    if name == "beyond":
        assert cells == 1 and max_cell == len(f)


def test_restatement_search_in_one_crowded_cell():
    p = KC.one_cell_cloud()
    f = filtered(p, KC.ONE_CELL_LEAF)
    assert len(f) == len(p) == 2000 and sorted(rows(f)) == sorted(rows(p))
    kf = K.OracleKeyframe(f, K.default_params(leaf_size=KC.ONE_CELL_LEAF))
    assert kf.stats() == (1, 2000)
    q = KC.box_queries(f, (0.375, 0.375, 0.15625), n=5000, side=1.0, sigma=0.4)
    for strict in (False, True):
        oi, od = kf.nearest(q, strict=strict)
        bi, bd = K.brute_force(f, q, 0.75, strict)
        assert np.array_equal(oi, bi) and np.array_equal(od.view(np.uint32), bd.view(np.uint32))
    print("one cell: kept %d of %d" % ((bi >= 0).sum(), len(q)))
    assert (bi >= 0).sum() >= len(q) // 4
    bad = np.array([[np.nan, 0.3, 0.15], [0.3, np.inf, 0.15], [0.3, 0.3, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    oi, od = kf.nearest(bad)
    assert (oi == -1).all() and (od == 0).all()


def test_counted_lattices_keep_every_point():
    for n in (64, 6144, 6145):
        p = KC.counted_lattice(n)
        f = filtered(p, 0.5)
        assert len(f) == n and sorted(rows(f)) == sorted(rows(p))
    p = KC.corner_lattice(K.default_params())
    assert len(filtered(p, 0.5)) == 2048
