"""The map localiser restated, without a device (docs/VOXEL_MAP.md section 11.3): tests/map_localizer_cases.py's
OracleLocalizer on cases A (a fan of eight from 9.7 m and 2.78 rad off, four levels) and B (one start nearby, three levels).
What the cases claim is asserted here, so that the device tests that share them stand on checked ground; the bounds guard the
inputs, not the device."""
import math
import os

import numpy as np
import pytest

import map_localizer_cases as ML
import vmap_oracle as V
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    """cases A and B once: name -> (the localiser's answer, the truth, per start the error of its level-0 f32 transform)"""
    parts, cloud, truth = ML.scene()
    out = {}
    for name, case in (("A", ML.CASE_A), ("B", ML.CASE_B)):
        loc = ML.OracleLocalizer(parts, case["levels"])
        r = loc.localize(cloud, ML.starts_of(case, truth), api.MapLocalizer.MAX_SCORE)
        err = [None if x is None else V.pose_error(x["transform"], truth) for x in r["last"][0]]
        out[name] = (r, truth, err)
    return out


def recovered(err):
    return err is not None and err[0] * 1e3 <= 2 * ML.RECORDED_MM and err[1] * 1e3 <= 2 * ML.RECORDED_MRAD


def test_case_a_the_fan_finds_the_truth(runs):
    r, truth, err = runs["A"]
    for i, (x, e) in enumerate(zip(r["last"][0], err)):
        print("start %d: iterations %s state %d converged %d fitness_pairs %d fitness %.6g; %.3f mm %.4f mrad from the truth" %
              (i, [lv[i]["iterations"] if lv[i] else None for lv in r["last"]][::-1], x["state"], x["converged"], x["fitness_pairs"], x["fitness"],
               e[0] * 1e3, e[1] * 1e3))
    assert len(r["last"]) == 4 and len(r["last"][0]) == 8 and r["n_source"] > 3000
    assert r["found"] and recovered(err[r["index"]])
    won = [i for i in range(8) if recovered(err[i])]
    lost = [i for i in range(8) if not recovered(err[i])]
    assert len(won) >= 1 and len(lost) >= 1 and r["index"] == won[0]
    assert all(r["last"][0][i]["fitness"] > api.MapLocalizer.MAX_SCORE for i in lost if r["last"][0][i] is not None)
    assert any(r["last"][0][i] is not None and r["last"][0][i]["fitness"] > api.MapLocalizer.MAX_SCORE for i in lost)
    assert all(r["last"][0][i]["fitness"] <= api.MapLocalizer.MAX_SCORE and r["last"][0][i]["converged"] for i in won)
    assert all(r["last"][0][i]["fitness_pairs"] >= ML.MIN_PAIR_SHARE * r["n_source"] for i in won)
    # no start of this fan begins within a leaf of the truth: level 0 alone could not have been entered
    yaw_truth = math.atan2(truth[1, 0], truth[0, 0])
    for s in ML.starts_of(ML.CASE_A, truth):
        d = math.hypot(float(s[0, 3]) - truth[0, 3], float(s[1, 3]) - truth[1, 3])
        assert d > 9.0 and abs(math.remainder(math.atan2(float(s[1, 0]), float(s[0, 0])) - yaw_truth, 2 * math.pi)) > 0.3


def test_case_b_one_start_nearby(runs):
    r, truth, err = runs["B"]
    assert len(r["last"]) == 3 and len(r["last"][0]) == 1
    assert r["found"] and r["index"] == 0 and recovered(err[0])
    assert all(lv[0]["converged"] for lv in r["last"])


def test_max_score_is_the_geometric_mean_of_the_two_populations(runs):
    """the default of both twins: the geometric mean of the largest winning and the smallest losing level-0 fitness over the
    two cases, rounded to one digit (docs/VOXEL_MAP.md section 11.3 records the two numbers)"""
    win, lose = [], []
    for r, truth, err in runs.values():
        for x, e in zip(r["last"][0], err):
            if x is not None:
                (win if recovered(e) else lose).append(x["fitness"])
    print("largest winning fitness %.6g, smallest losing %.6g, geometric mean %.4g" % (max(win), min(lose), math.sqrt(max(win) * min(lose))))
    assert float("%.1g" % math.sqrt(max(win) * min(lose))) == api.MapLocalizer.MAX_SCORE == 0.03
    assert max(win) < api.MapLocalizer.MAX_SCORE / 3 and min(lose) > 3 * api.MapLocalizer.MAX_SCORE
    hdr = open(os.path.join(ROOT, "include", "slam_amd", "global_match.hpp")).read()
    assert "MAX_SCORE = 0.03;" in hdr and "GATE_RATIO = 2.0;" in hdr and "N_YAW = 8;" in hdr and "MIN_PAIR_SHARE = 0.5;" in hdr
    assert (api.MapLocalizer.GATE_RATIO, api.MapLocalizer.N_YAW, api.MapLocalizer.MIN_PAIR_SHARE) == (ML.GATE_RATIO, ML.N_YAW, ML.MIN_PAIR_SHARE)


def test_the_winner_rule():
    def res(pairs, fitness, converged=1, state=api.KF_TRANSFORM):
        return dict(fitness_pairs=pairs, fitness=fitness, converged=converged, state=state)
    n = 1000
    assert ML.pick([res(600, 0.01), res(700, 0.02), res(700, 0.001)], n, 0.03) == 1          # most pairs, then the lowest index
    assert ML.pick([res(499, 0.01), res(500, 0.03)], n, 0.03) == 1                          # both bounds are kept
    assert ML.pick([res(900, 0.031), res(900, 0.01, converged=0), None, res(900, float("nan"))], n, 0.03) == -1
    assert ML.pick([res(900, 0.0, state=api.KF_DEGENERATE), res(2, 0.0, state=api.KF_NO_CORRESPONDENCES)], n, 0.03) == -1
    assert ML.pick([], n, 0.03) == -1


def test_the_yaw_fan_of_the_adapter_is_the_restated_one():
    for x, y, yaw, n in ((1.5, -2.25, 0.3, 8), (-9.7, 0.3, 2.78, 8), (0.0, 0.0, -3.0, 5), (3.0, 4.0, 6.0, 1)):
        a, b = api.MapLocalizer.yaw_fan(x, y, yaw, n), ML.yaw_fan(x, y, yaw, n)
        assert len(a) == len(b) == n
        for p, q in zip(a, b):
            assert p.dtype == np.float32 and p.tobytes() == q.tobytes()
        assert a[0].tobytes() == api.GlobalMatcher.planar(np.float32(x), np.float32(y), np.float32(yaw)).tobytes()
    fan = api.MapLocalizer.yaw_fan(0, 0, 0.0, 4)
    assert np.allclose([abs(math.atan2(float(m[1, 0]), float(m[0, 0]))) for m in fan], [0, math.pi / 2, math.pi, math.pi / 2], atol=1e-6)
    assert float(fan[1][1, 0]) > 0 > float(fan[3][1, 0])
