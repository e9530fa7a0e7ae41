"""The streaming mapper's sliding-window ICP target (slam_amd/csrc/mapper.hip: window_points_kernel, thin_*_kernel,
begin_rebuild / adopt_build, and the index build's device-count and small-LDS paths in icp_build.hip) read back after
every push and held BIT FOR BIT to the numpy restatement tests/mapper_target_cases.py, worked from the poses the mapper
itself returned.  No comparison here has a tolerance: the window's points are unfused f64 sums of values the test holds
exactly, and the index stores their f32 conversion (docs/MAPPER_TARGET.md)."""
import signal

import numpy as np
import pytest

import mapper_target_cases as T
from slam_amd import api, synth

pytestmark = pytest.mark.gpu
TEST_SECONDS = 120
ICP = dict(max_iter=5)


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


@pytest.fixture(scope="module")
def prior():
    return synth.make_map(T.PRIOR_POINTS)


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32)).view(np.uint32).reshape(-1, 2)


def assert_same_points(got, want, what):
    """count, points and order, bit for bit (want: f64, converted as the build converts: one rounding to f32)"""
    g, w = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 2), f32_bits(want)
    assert len(g) == len(w), "%s: %d points, the restatement has %d" % (what, len(g), len(w))
    bad = np.flatnonzero((g != w).any(1))
    assert bad.size == 0, "%s: %d of %d points differ, first at %d: %r against %r" % (what, bad.size, len(g), bad[0], got[bad[0]], want[bad[0]])


def run_case(params, chunks, prior, pipelined):
    """Pushes the chunks one by one; after every push the target in force is read back and compared.  Returns one record per
    push (what was read, and the restatement's account of the rebuild that made it)."""
    m_ga, m_nga = prior
    size, res = params["grid_size"], params["resolution"]
    mp = api.Mapper(m_ga, m_nga, grid=dict(rolling=0, min_cluster_points=20, max_range=0.45 * size * res), icp=ICP,
                    grid_size_x=size, grid_size_y=size, resolution=res, window_chunks=params["window_chunks"],
                    rebuild_every=params["rebuild_every"], target_points=params["target_points"], keep_prior=params["keep_prior"],
                    thin_res=params["thin_res"], strict_window=1, pipelined=pipelined,
                    max_scans=max(c.n_scans for c in chunks), max_points=max(c.n_points for c in chunks))
    sched = T.Schedule(params["window_chunks"], params["rebuild_every"])
    want, info, rebuilds, entries, log, host = (m_ga, m_nga), None, 0, [], [], None
    try:
        for k, c in enumerate(chunks):
            reads = sched.push(k)
            if reads is not None:
                assert reads == list(range(len(entries)))[-params["window_chunks"]:]
                made = T.target(m_ga, m_nga, entries, params)
                if made is not None:                      # fewer than five points: the previous target stays in force
                    want, info, rebuilds, host = made[:2], made[2], rebuilds + 1, None
            R, t = mp.wait(mp.push(c))
            assert np.isfinite(R).all() and np.isfinite(t).all()
            ga, nga = mp.target_model()
            assert_same_points(ga, want[0], "push %d, class GA" % k)
            assert_same_points(nga, want[1], "push %d, class NGA" % k)
            assert mp.stats()["rebuilds"] == rebuilds, (k, mp.stats(), rebuilds)                 # (a)
            if host is None:                                                                    # (b) the host build of the same points
                h = api.Icp(want[0], want[1], build_on_host=1, pair_scans=-1, **ICP)
                assert not h.build_info()[0]
                host = (h.index_info(), h.index_blob(0), h.index_blob(1))
                h.close()
            got_info = mp.target_index_info()
            assert got_info.pop("built_on_device") and got_info.pop("build_host_ms") is not None    # the mapper's targets: device builds
            blobs = mp.target_index_blobs()
            assert got_info == host[0], (k, got_info, host[0])
            for which in (0, 1):
                x, y = blobs[which], host[1 + which]
                assert x.shape == y.shape, "push %d: blob %d has %d bytes, the host build %d" % (k, which, x.size, y.size)
                diff = np.flatnonzero(x != y)
                assert diff.size == 0, "push %d: blob %d differs at %d bytes, first at offset %d of %d" % (k, which, diff.size, diff[0], x.size)
            n_ga, n_nga = T.class_totals(c)
            sg = T.stride_for(n_ga, params["thin_res"], params["target_points"], params["window_chunks"])
            sn = T.stride_for(n_nga, params["thin_res"], params["target_points"], params["window_chunks"])
            entries.append(T.window_points(c, R, t, sg, sn))
            log.append(dict(k=k, ga=ga, nga=nga, blobs=blobs, index=got_info, rebuilt=reads is not None and made is not None, info=info,
                            rebuilds=rebuilds, strides=(sg, sn), totals=(n_ga, n_nga), R=R, t=t))
        mp.finish()
    finally:
        mp.close()
    return log


def check_edges(case, log, prior):
    """what the case is there for, named: the count, the block, the stride, kept against cap, the segments"""
    name, infos = case.name, [r["info"] for r in log if r["rebuilt"]]
    line = "%s:" % name
    if name == "strides 1, 2, 3 around per_chunk":
        pc = T.per_chunk_of(case.params["target_points"], 2)
        seen = {(r["totals"][1] - pc, r["strides"][1]) for r in log}
        assert {(-1, 1), (0, 1), (1, 2)} <= seen and {r["strides"][0] for r in log} == {1, 2, 3}
        line += " per_chunk %d, NGA count - per_chunk and stride %s" % (pc, sorted(seen))
    elif name.startswith("empty scans"):
        assert all(r["totals"] == (81, 102) and r["strides"] == (1, 2) for r in log)      # 81 GA kept, every second of 102 NGA
        assert [i["window"] for i in infos] == [(81, 51), (162, 102), (162, 102)]
        assert len(log[-1]["ga"]) == (len(prior[0]) if case.params["keep_prior"] else 0) + 2 * 81
        assert len(log[-1]["nga"]) == (len(prior[1]) if case.params["keep_prior"] else 0) + 2 * 51
        line += " GA %d, NGA %d points in the last target" % (len(log[-1]["ga"]), len(log[-1]["nga"]))
    elif name == "class totals 255, 256, 257, 513":
        for cls in (0, 1):
            assert {i["window"][cls] for i in infos} >= {255, 256, 257, 513}
        assert {i["nga"]["blocks"] for i in infos} >= {1, 2, 3}
        line += " window totals %s" % [i["window"] for i in infos]
    elif name == "more than 65 536 points":
        i = infos[-1]
        assert i["window"][1] > 65536 and i["nga"]["blocks"] > 256 + 4 and i["window"][0] == 0
        line += " %d points, %d blocks, kept %d of cap %d, stride %d" % (i["window"][1], i["nga"]["blocks"], i["nga"]["kept"], i["nga"]["cap"], i["nga"]["stride"])
    elif name == "eight segments and the ring's wrap":
        assert max(i["segments"] for i in infos) == (8, 8) and sum(i["segments"] == (8, 8) for i in infos) == 5 and len(log) == 13
        line += " segments per rebuild %s" % [i["segments"][0] for i in infos]
    elif name == "the extent cuts the room":
        half = 0.5 * case.params["grid_size"] * case.params["resolution"]      # counted from the mapper's own poses
        q = np.concatenate([np.concatenate(T.registered(c, r["R"], r["t"])) for c, r in zip(case.chunks(), log)])
        inside = ((q >= -half) & (q < half)).all(1)
        assert log[-1]["rebuilds"] == 3 and infos[-1]["nga"]["kept"] > 0 and 0 < inside.sum() < len(q)
        line += " %d of %d registered points outside +-%.1f m, NGA kept %s" % ((~inside).sum(), len(q), half, [i["nga"]["kept"] for i in infos])
    elif name == "six rebuilds in a row":
        assert log[-1]["rebuilds"] == 6 and all(r["rebuilt"] for r in log[1:])
        line += " kept per rebuild %s" % [(i["ga"]["kept"], i["nga"]["kept"]) for i in infos]
    elif name == "no GA point in the window":
        assert all(i["ga"]["kept"] == 0 and i["window"][0] == 0 for i in infos) and len(log[-1]["ga"]) == len(prior[0]) > 0
        assert len(log[-1]["nga"]) > len(prior[1])
        line += " GA stays at the prior's %d points" % len(prior[0])
    elif name.startswith("fewer than five points"):
        assert [r["rebuilds"] for r in log] == [0, 0, 1] and [r["rebuilt"] for r in log] == [False, False, True]
        assert len(log[1]["ga"]) == len(prior[0]) and len(log[1]["nga"]) == len(prior[1])       # four points: the prior stayed
        assert len(log[2]["ga"]) + len(log[2]["nga"]) <= 30
        line += " a 4-point window left the prior in force; then %d + %d points" % (len(log[2]["ga"]), len(log[2]["nga"]))
    elif name == "a rebuild every third chunk":
        assert [r["k"] for r in log if r["rebuilt"]] == [3, 6, 9] and log[-1]["rebuilds"] == 3
        assert all(log[k]["ga"].shape == log[3 * (k // 3)]["ga"].shape for k in range(3, 10))
        line += " rebuilds at pushes 3, 6, 9"
    else:
        raise AssertionError("no edge named for %s" % name)
    print(line)


@pytest.mark.parametrize("pipelined", [1, 0])
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_target_is_the_restatement(case, pipelined, prior):
    check_edges(case, run_case(case.params, case.chunks(), prior, pipelined), prior)


def test_the_cap_edge(prior):
    """kept == cap keeps every winner, kept == cap + 1 every second: the stride is worked out on the device from a total the
    host never sees.  Chunk 0 is registered against the prior alone, so its window -- and K, the cells its NGA points
    occupy -- is the same whatever target_points says."""
    chunks = T.cap_edge_chunks()
    params = dict(T.Case("", "", None, thin_res=0.1).params)
    first = run_case(dict(params, target_points=100000), chunks, prior, 1)
    K = first[1]["info"]["nga"]["kept"]
    assert first[1]["info"]["nga"]["stride"] == 1 and len(first[1]["nga"]) == len(prior[1]) + K and K >= 66
    at_cap = run_case(dict(params, target_points=2 * K), chunks, prior, 1)
    above = run_case(dict(params, target_points=2 * (K - 1)), chunks, prior, 1)
    for run in (at_cap, above):
        assert np.array_equal(run[0]["R"], first[0]["R"]) and np.array_equal(run[0]["t"], first[0]["t"])
    a, b = at_cap[1]["info"]["nga"], above[1]["info"]["nga"]
    assert (a["kept"], a["cap"], a["stride"]) == (K, K, 1) and len(at_cap[1]["nga"]) == len(prior[1]) + K
    assert (b["kept"], b["cap"], b["stride"]) == (K, K - 1, 2) and len(above[1]["nga"]) == len(prior[1]) + (K + 1) // 2
    print("cap edge: K = %d winners; cap K: stride 1, %d points; cap K - 1: stride 2, %d points" % (K, K, (K + 1) // 2))


def test_the_same_bits_twice(prior):
    """one thinned case twice pipelined and once stage after stage: every target's read-back, its index and its lists identical"""
    case = T.case(T.SAME_BITS_CASE)
    runs = [run_case(case.params, case.chunks(), prior, p) for p in (1, 1, 0)]
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            assert np.array_equal(a["ga"].view(np.uint32), b["ga"].view(np.uint32)) and np.array_equal(a["nga"].view(np.uint32), b["nga"].view(np.uint32))
            assert a["index"] == b["index"] and np.array_equal(a["blobs"][0], b["blobs"][0]) and np.array_equal(a["blobs"][1], b["blobs"][1])
            assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])


def test_read_model_of_a_plain_handle_and_its_capacity(prior):
    """slam_icp_read_model on handles built both ways, 16- and 32-bit index entries, a short capacity, and point-to-line's one class"""
    import ctypes as C
    m_ga, m_nga = prior
    for kw in ({}, {"build_on_host": 1}, {"force_global": 1}):
        icp = api.Icp(m_ga, m_nga, **kw)
        assert_same_points(icp.read_model(0), m_ga, "GA %r" % kw)
        assert_same_points(icp.read_model(1), m_nga, "NGA %r" % kw)
        n, buf = C.c_int(0), np.full((len(m_nga), 2), 7.0, np.float32)
        rc = api.lib().slam_icp_read_model(icp.h, 1, buf.ctypes.data_as(C.c_void_p), len(m_nga) - 1, C.byref(n))
        assert rc == api.E_NOMEM and n.value == len(m_nga) and (buf == 7.0).all()      # the count, and nothing written
        icp.close()
    p2l = api.Icp(m_ga, m_nga, mode=api.ICP_P2L)
    assert len(p2l.read_model(0)) == 0
    assert_same_points(p2l.read_model(1), np.concatenate([m_ga, m_nga]), "point-to-line: one class, GA then NGA")
    p2l.close()
