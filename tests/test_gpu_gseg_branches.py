"""slam_gseg_* (slam_amd/csrc/gseg.hip) against the oracle on the branches benign clouds never take: the hand-built clouds
of tests/gseg_cases.py -- a model over 64 bins (the serial solve), candidates that stay out (the state-2 verdict), dozens of
rounds of growth, models of one bin and of none, num_seedpoints 0 / 1 / 200, seeds that are no prefix of the sorted list,
bit-equal heights and a signed-zero tie, the exact octant directions, empty sectors, shuffled, strided and ragged clouds, a
run of one bin across wavefronts.  tests/test_gseg_cases.py shows on the CPU that the oracle reaches every branch named
here, at least 1e-6 clear of every threshold: labels, states and per-sector rounds are compared exactly, the GP values to
the 1e-9 of tests/test_gseg.py.  All cases of one parameter set share one handle, large clouds in front of small and empty
ones.  Then split_dev's rows and slam_gseg_classify_ga_counted_dev."""
import ctypes as C
import signal

import numpy as np
import pytest

import gseg_cases as G
import oracle_lib as O
from slam_amd import api

TEST_SECONDS = 120
CASES = G.cases()
NAMES = [c["name"] for c in CASES]
EMPTY = np.zeros((0, 3), np.float32)


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
    return tuple(sorted(c["params"].items()))


def run(seg, xyz):
    lab = seg.segment(xyz)
    st, val, it = seg.read_model()
    return dict(labels=lab, state=st, value=val, iters=it)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("labels", "state", "iters")) and \
        np.array_equal(a["value"][a["state"] > 0], b["value"][b["state"] > 0])


class Shared:
    """One handle per parameter set; its cases from the largest cloud to the smallest, then an empty cloud, then the
    largest and the smallest once more."""

    def __init__(self):
        self.sets, self.first, self.again, self.after_empty = {}, {}, {}, {}
        for c in CASES:
            self.sets.setdefault(param_key(c), []).append(c)
        for key, cs in self.sets.items():
            cs.sort(key=lambda c: -len(c["xyz"]))
            seg = api.GroundSegmentation(**G.api_params(dict(key)))
            for c in cs:
                self.first[c["name"]] = run(seg, c["xyz"])
            self.after_empty[key] = run(seg, EMPTY)
            for c in (cs[0], cs[-1]):
                self.again[c["name"]] = run(seg, c["xyz"])
            seg.close()


@pytest.fixture(scope="module")
def shared():
    return Shared()


@pytest.fixture(scope="module")
def oracle():
    return {c["name"]: O.gseg_segment_trace(c["xyz"], O.gseg_params(**c["params"])) for c in CASES}


def describe(st, it):
    secs = np.flatnonzero((st.reshape(G.NA, G.NL) > 0).any(1))
    return "sectors %s%s, state 1 / 2 in %d / %d bins, rounds %s" % (
        secs[:12].tolist(), " ..." if len(secs) > 12 else "", (st == 1).sum(), (st == 2).sum(), it[secs][:12].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_follows_the_oracle(shared, oracle, name):
    c, dev, ora = CASES[NAMES.index(name)], shared.first[name], oracle[name]
    m = ora["state"] > 0
    both = m & (dev["state"] > 0)
    dv = float(np.abs(dev["value"] - ora["value"])[both].max()) if both.any() else 0.0
    print("\n%-22s device: %s\n%-22s oracle: %s\n    labels %s / %s, |value - oracle| %.3g over %d bins, margin %.3g" % (
        name, describe(dev["state"], dev["iters"]), "", describe(ora["state"], ora["rounds"]),
        np.bincount(dev["labels"], minlength=4).tolist(), np.bincount(ora["labels"], minlength=4).tolist(), dv, both.sum(),
        min(ora["margins"].values())))
    assert min(ora["margins"].values()) >= G.MARGIN_TOL          # (tests/test_gseg_cases.py holds the oracle to the whole case)
    assert np.array_equal(dev["state"], ora["state"])
    assert np.array_equal(dev["iters"], ora["rounds"])          # all 72 sectors, not their sum
    assert dv < c["value_tol"]
    assert np.array_equal(dev["labels"], ora["labels"])


@pytest.mark.gpu
def test_shared_handle_gives_what_a_fresh_one_gives(shared):
    """The label kernel clears the bin counts and prototypes for the next call: every result of the shared handles, after
    larger clouds, and after an empty one, is bit for bit a fresh handle's; after the empty cloud the model is empty."""
    for key, cs in shared.sets.items():
        sizes = [len(c["xyz"]) for c in cs]
        print("\nhandle %s: clouds of %s points, then 0, %d, %d" % (dict(key), sizes, sizes[0], sizes[-1]))
        for c in cs:
            seg = api.GroundSegmentation(**G.api_params(dict(key)))
            fresh = run(seg, c["xyz"])
            seg.close()
            assert same_bits(shared.first[c["name"]], fresh), c["name"]
            if c["name"] in shared.again:
                assert same_bits(shared.again[c["name"]], fresh), c["name"]
        e = shared.after_empty[key]
        assert len(e["labels"]) == 0 and (e["state"] == 0).all() and (e["iters"] == 0).all()
    default = [len(c["xyz"]) for c in shared.sets[()]]
    assert default[0] > G.NA * G.NL > default[1] and default[-1] == 1          # a launch sized by the cloud, then by the bins


@pytest.mark.gpu
def test_empty_cloud_on_the_device_path_clears_the_model():
    seg = api.GroundSegmentation()
    c = CASES[NAMES.index("big_model")]
    assert (run(seg, c["xyz"])["state"] > 0).sum() == 180
    seg.segment_dev(api.DeviceArray((1, 3), np.float32), 0, 3, api.DeviceArray((1,), np.uint8))
    st, val, it = seg.read_model()
    assert (st == 0).all() and (it == 0).all()
    assert (run(seg, c["xyz"])["state"] > 0).sum() == 180
    seg.close()


def rows(a):
    return sorted(map(tuple, np.asarray(a).tolist()))


@pytest.mark.gpu
def test_split_rows_are_the_labelled_points(oracle):
    """slam_gseg_split_dev: the ground and obstacle outputs as sets of rows (x, y, z, 0) against the label masks, cloud after
    cloud through the same buffers"""
    seg = {}
    for name in ("big_model", "ramp", "ramp_big", "long_run_stride8", "empty_sectors", "synth_n8191", "synth_n257", "one_seed_plus",
                 "no_seed_far", "big_model_n1"):
        c = CASES[NAMES.index(name)]
        key = param_key(c)
        if key not in seg:
            seg[key] = api.GroundSegmentation(**G.api_params(c["params"]))
        xyz = c["xyz"]
        n, stride = xyz.shape
        d_xyz, d_lab = api.DeviceArray.from_host(xyz), api.DeviceArray((n,), np.uint8)
        d_gnd = api.DeviceArray.from_host(np.full((n, 4), -77.0, np.float32))
        d_obs = api.DeviceArray.from_host(np.full((n, 4), -77.0, np.float32))
        d_cnt = api.DeviceArray.from_host(np.array([-1, -1], np.int32))
        seg[key].segment_dev(d_xyz, n, stride, d_lab)
        seg[key].split_dev(d_xyz, n, stride, d_lab, d_gnd, d_obs, d_cnt)
        api.synchronize()
        lab, (n_gnd, n_obs), gnd, obs = d_lab.download(), d_cnt.download(), d_gnd.download(), d_obs.download()
        print("\n%-18s %d points: %d ground, %d obstacle" % (name, n, n_gnd, n_obs))
        assert np.array_equal(lab, oracle[name]["labels"])
        for got, k, which in ((gnd, n_gnd, api.GSEG_GROUND), (obs, n_obs, api.GSEG_OBSTACLE)):
            want = np.zeros((int((lab == which).sum()), 4), np.float32)
            want[:, :3] = xyz[lab == which, :3]
            assert k == len(want)
            assert rows(got[:k].view(np.uint32)) == rows(want.view(np.uint32))          # bit for bit, -0.0f included
            assert (got[k:] == -77.0).all()          # nothing written past the count
    for s in seg.values():
        s.close()


# ------------------------------------------------------------------ slam_gseg_classify_ga_counted_dev
SENTINEL = 77


def classify_counted(seg, d_xyz, count, capacity, stride, d_flags):
    d_n = api.DeviceArray.from_host(np.array([count], np.int32))
    d_flags.upload(np.full(capacity, SENTINEL, np.uint8))
    api.check(api.lib().slam_gseg_classify_ga_counted_dev(seg.h, d_xyz.ptr, d_n.ptr, int(capacity), int(stride), d_flags.ptr, None))
    api.synchronize()
    return d_flags.download()


def lattice_columns(parity, side=24, origin=(-40.0, 12.0)):
    """the centres of the 0.5 m cells of every second column of a side x side block, three points each"""
    i, j = np.meshgrid(np.arange(parity, side, 2), np.arange(side), indexing="ij")
    xy = np.stack([origin[0] + 0.5 * i.ravel() + 0.25, origin[1] + 0.5 * j.ravel() + 0.25], 1)
    pts = np.concatenate([xy + d for d in ((0, 0), (0.125, -0.125), (-0.0625, 0.0625))])
    return np.concatenate([pts, np.zeros((len(pts), 1))], 1).astype(np.float32)


@pytest.mark.gpu
def test_counted_ga_classification_matches_oracle():
    rs = np.random.RandomState(3)
    blob = (rs.rand(3000, 3) * [30, 30, 1] - [15, 15, 0]).astype(np.float32)
    wide = (rs.rand(1000, 3) * [700, 700, 1] - [350, 350, 0]).astype(np.float32)          # the edge ring and beyond
    pts = np.concatenate([blob, wide])[rs.permutation(4000)]
    cap = len(pts)
    seg = api.GroundSegmentation()
    d_xyz, d_flags = api.DeviceArray.from_host(pts), api.DeviceArray((cap,), np.uint8)
    for count in (1000, 257, 1, cap):          # fewer points than the launch was sized for: the rest is not touched
        f = classify_counted(seg, d_xyz, count, cap, 3, d_flags)
        ref = O.classify_ga(pts[:count])
        assert np.array_equal(f[:count], ref) and (f[count:] == SENTINEL).all(), count
        assert {0, 1, 255} >= set(ref.tolist()) and (count < cap or len(set(ref.tolist())) == 3)
    # a call without points marks nothing and answers nothing; the next one is a call like any other
    f = classify_counted(seg, d_xyz, 0, cap, 3, d_flags)
    assert (f == SENTINEL).all()
    f = classify_counted(seg, d_xyz, cap, cap, 3, d_flags)
    assert np.array_equal(f, O.classify_ga(pts))
    seg.close()


@pytest.mark.gpu
def test_counted_ga_classification_forgets_the_call_before():
    """A, B, A on one handle, A and B the even and the odd columns of one block of cells: alone, every cell of either has
    six empty neighbours (GA); with the other's cells still counted, the inner ones have none."""
    A, B = lattice_columns(0), lattice_columns(1)
    ref_a, ref_b, ref_ab = O.classify_ga(A), O.classify_ga(B), O.classify_ga(np.concatenate([A, B]))
    assert (ref_a == 1).all() and (ref_b == 1).all() and (ref_ab == 0).sum() > len(A)          # what a stale lattice would say
    seg = api.GroundSegmentation()
    cap = len(A) + 100
    pad = np.zeros((100, 3), np.float32)
    d_a, d_b = api.DeviceArray.from_host(np.concatenate([A, pad])), api.DeviceArray.from_host(np.concatenate([B, pad]))
    d_flags = api.DeviceArray((cap,), np.uint8)
    for d, n, ref in ((d_a, len(A), ref_a), (d_b, len(B), ref_b), (d_a, len(A), ref_a)):
        f = classify_counted(seg, d, n, cap, 3, d_flags)
        assert np.array_equal(f[:n], ref) and (f[n:] == SENTINEL).all()
    # ... and the uncounted entry point shares the lattice and the epoch
    assert np.array_equal(seg.classify_ga(B), ref_b) and np.array_equal(seg.classify_ga(np.concatenate([A, B])), ref_ab)
    f = classify_counted(seg, d_a, len(A), cap, 3, d_flags)
    assert np.array_equal(f[:len(A)], ref_a)
    seg.close()
