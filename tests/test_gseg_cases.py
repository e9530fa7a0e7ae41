"""The oracle (oracle/gseg_oracle.c) on the hand-built clouds of tests/gseg_cases.py: every case reaches the branch it is
named for -- seed count, rounds, the model size entering each round, candidates left, points dropped -- and every decision
it takes is at least MARGIN_TOL from its threshold.  The second is a condition on the inputs, not a measurement: device
and oracle agree on the GP values to 1e-9, so a case 1 000 times clear of every threshold cannot have a label flipped by
rounding, and tests/test_gpu_gseg_branches.py may compare labels, states and rounds exactly.  No GPU needed."""
import numpy as np
import pytest

import gseg_cases as G
import oracle_lib as O

CASES = G.cases()
NAMES = [c["name"] for c in CASES]
NL = G.NL


def trace_of(c, **kw):
    return O.gseg_segment_trace(c["xyz"], O.gseg_params(**c["params"]), **kw)


def sorted_signal_bins(c, t, sec):
    """the sector's signal bins as (height, bin, range of the prototype), sorted as :229 sorts them -- from the cloud alone"""
    xyz, out = c["xyz"], []
    for b in range(NL):
        idx = np.flatnonzero(t["bin_of"] == sec * NL + b)
        if len(idx) > 5:
            i = idx[np.argmin(xyz[idx, 2], axis=0)]          # (the first of the lowest)
            out.append((float(xyz[i, 2]), b, float(np.float32(np.hypot(float(xyz[i, 0]), float(xyz[i, 1]))))))
    return sorted(out)


def longest_run(bin_of):
    edges = np.flatnonzero(np.diff(bin_of) != 0)
    return int(np.diff(np.concatenate([[-1], edges, [len(bin_of) - 1]])).max())


def check_expectations(c, t):
    """what the case's `expect` asks of the oracle's trace; returns a line describing what was reached"""
    e, sec = c["expect"], c["sector"]
    st = t["state"].reshape(G.NA, NL)
    lab = np.bincount(t["labels"], minlength=4)
    known = {"seeds", "rounds", "min_rounds", "model", "left", "min_left", "over64", "over64_distinct", "max_entering",
             "last_round_adds", "ground", "dropped", "bins_state1", "occupied_sectors", "seeds_not_a_prefix", "longest_run",
             "same_as"}
    assert set(e) <= known, set(e) - known
    line = "labels %s" % lab.tolist()
    if sec is not None:
        entering = t["round_model"][sec]
        model, left = int((st[sec] == 1).sum()), int((st[sec] == 2).sum())
        line = "sector %d: seeds %d, rounds %d, model %d, left %d, entering %s; " % (sec, t["seeds"][sec], t["rounds"][sec], model, left,
                                                                                    entering) + line
        assert (st[np.arange(G.NA) != sec] == 0).all() and t["rounds"].sum() == t["rounds"][sec]          # the case lives there alone
        assert len(entering) == t["rounds"][sec] and (not entering or entering[0] == t["seeds"][sec])
        assert all(a <= b for a, b in zip(entering, entering[1:])) and (not entering or entering[-1] <= model)
        over = [m for m in entering if m > 64]
        for key, got in (("seeds", t["seeds"][sec]), ("rounds", t["rounds"][sec]), ("model", model), ("left", left)):
            if key in e:
                assert got == e[key], (key, got, e[key])
        if "min_rounds" in e:
            assert t["rounds"][sec] >= e["min_rounds"]
        if "min_left" in e:
            assert left >= e["min_left"]
        if "over64" in e:          # the serial solve runs in that many rounds at least
            assert len(over) >= e["over64"], entering
        if "over64_distinct" in e:
            assert len(set(over)) >= e["over64_distinct"], entering
        if "max_entering" in e:          # ... or in none
            assert max(entering) <= e["max_entering"], entering
        if "last_round_adds" in e:          # the loop ends because a round adds nothing, with candidates left
            assert model - entering[-1] == e["last_round_adds"] and left > 0
        if t["seeds"][sec] < 2:          # "model too small": no round, no candidate verdict
            assert t["rounds"][sec] == 0 and left == 0
        if e.get("seeds_not_a_prefix"):
            p = O.gseg_params(**c["params"])
            sig = sorted_signal_bins(c, t, sec)
            ok = [r < p.max_seed_range and abs(h) < p.max_seed_height for h, b, r in sig]
            taken = np.flatnonzero(ok)[:p.num_seedpoints]
            assert len(taken) == t["seeds"][sec] and not all(ok[:taken[-1] + 1])          # a failing entry in front of a seed
            assert not ok[0] and sum(not o for o in ok[:taken[-1]]) >= 3
    if "ground" in e:
        assert lab[O.GSEG_GROUND] == e["ground"], lab
    if "dropped" in e:
        assert lab[O.GSEG_DROPPED] == e["dropped"], lab
    if "bins_state1" in e:
        assert sorted(np.flatnonzero(t["state"] == 1).tolist()) == sorted(e["bins_state1"])
    if "occupied_sectors" in e:
        assert np.flatnonzero((st > 0).any(1)).tolist() == e["occupied_sectors"]
        assert len(e["occupied_sectors"]) < G.NA and (t["seeds"][~(st > 0).any(1)] == 0).all()
    if "longest_run" in e:
        assert longest_run(t["bin_of"]) == e["longest_run"] and e["longest_run"] >= 200
    return line


@pytest.fixture(scope="module")
def traces():
    return {c["name"]: trace_of(c) for c in CASES}


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_branch_clear_of_every_threshold(traces, name):
    c, t = CASES[NAMES.index(name)], traces[name]
    line = check_expectations(c, t)
    margin = min(t["margins"].values())
    print("\n%-22s n %d; %s\n    margins %s" % (name, len(c["xyz"]), line, {k: float("%.3g" % v) for k, v in t["margins"].items()}))
    assert margin >= G.MARGIN_TOL, t["margins"]
    assert c["value_tol"] == G.VALUE_TOL          # (a case that needs more says so, with its figures, in gseg_cases.py)
    # both entry points are one body
    lab, bins, state, value, iters = O.gseg_segment(c["xyz"], O.gseg_params(**c["params"]))
    assert np.array_equal(lab, t["labels"]) and np.array_equal(bins, t["bin_of"]) and np.array_equal(state, t["state"])
    assert np.array_equal(value, t["value"]) and iters == t["iterations"] == t["rounds"].sum()
    # the oracle's own rounding: the solve in long double decides everything the same way, and moves the values by this much
    ld = trace_of(c, long_double=True)
    assert np.array_equal(ld["labels"], t["labels"]) and np.array_equal(ld["state"], t["state"]) and np.array_equal(ld["rounds"], t["rounds"])
    m = t["state"] > 0
    own = float(np.abs(ld["value"] - t["value"])[m].max()) if m.any() else 0.0
    print("    |oracle - long double oracle| of value: %.3g" % own)
    assert own < c["value_tol"] / 100          # two decades under the bound the device is held to


def test_variants_are_their_originals(traces):
    """a permuted or strided cloud is the same cloud: the same state, values and rounds, the labels permuted with the points"""
    seen = 0
    for c in CASES:
        if "same_as" in c["expect"]:
            a, b = traces[c["name"]], traces[c["expect"]["same_as"]]
            assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["rounds"], b["rounds"])
            assert np.array_equal(a["value"], b["value"])
            assert np.array_equal(np.bincount(a["labels"], minlength=4), np.bincount(b["labels"], minlength=4))
            seen += 1
    assert seen >= 3


def test_the_cases_cover_every_branch(traces):
    """over all cases: the serial solve (a model over 64 bins entering a round) in several rounds, candidates left after a
    round that added nothing, many rounds of growth, every size of a too-small model, sectors without a signal bin, a run of
    one bin across wavefronts, ragged last blocks, and all four labels"""
    entering = [m for t in traces.values() for r in t["round_model"] for m in r]
    assert sum(m > 64 for m in entering) >= 10 and any(m <= 64 for m in entering)
    assert max(t["rounds"].max() for t in traces.values()) >= 25
    assert sum(int((t["state"] == 2).sum()) for t in traces.values()) >= 100
    seeds = {int(s) for t in traces.values() for s in t["seeds"]}
    assert {0, 1, 10, 186} <= seeds
    assert {len(c["xyz"]) for c in CASES} >= {1, 63, 65, 257, 8191}
    assert any(len(c["xyz"]) % 256 for c in CASES)
    assert any(c["xyz"].shape[1] == 8 for c in CASES)
    assert set(np.concatenate([t["labels"] for t in traces.values()]).tolist()) == {0, 1, 2, 3}
    assert {c["params"].get("num_seedpoints") for c in CASES} >= {0, 1, 200, None}


def test_octant_directions_land_where_libm_puts_them(traces):
    """atan2 of an exact axis or diagonal is an exact multiple of 45 degrees in libm: sectors 0, 9, .. 63, and 360.0 - tiny
    rounds to 360.0, which the clamp sends to sector 71"""
    c, t = CASES[NAMES.index("octants")], traces["octants"]
    sectors = t["bin_of"].reshape(-1, G.K)[:, 0] // NL
    assert sectors.tolist() == [0, 9, 18, 27, 36, 45, 54, 63, 71]
    assert (t["bin_of"].reshape(-1, G.K) == t["bin_of"].reshape(-1, G.K)[:, :1]).all()
    assert (c["xyz"][-G.K:, 1] < 0).all()


def test_signed_zero_tie_keeps_the_first_point(traces):
    c, t = CASES[NAMES.index("height_ties")], traces["height_ties"]
    first = 9 * G.K
    b = t["bin_of"][first]
    assert b == 20 * NL + 12 and t["bin_of"][first + 4] == b and t["state"][b] == 1
    assert not np.signbit(t["value"][b])          # the model holds the +0.0f point's height ...
    # ... and its range: with the other point's range the candidates' GP means move by far more than the bound
    swapped = c["xyz"].copy()
    swapped[[first, first + 4]] = swapped[[first + 4, first]]
    swapped[[first, first + 4], 2] = swapped[[first + 4, first], 2]          # (+0.0f still first, at the other range)
    other = O.gseg_segment_trace(swapped, O.gseg_params(**c["params"]))
    cand = np.flatnonzero(t["state"] == 2)
    assert len(cand) == 4 and np.array_equal(other["state"], t["state"])
    moved = np.abs(other["value"][cand] - t["value"][cand]).max()
    print("\nthe candidates' GP mean with bin 12 at its other point's range: moved by %.3g" % moved)
    assert moved > 1e3 * c["value_tol"]
