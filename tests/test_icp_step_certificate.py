"""The step certificate (tests/icp_step_certificate.py) held to account without a GPU: it accepts the oracle's own brute-force
traces with deviation 0 and rejects every mutation a subtly wrong kernel would produce -- a neighbour swapped for the runner-up,
a gate that drops or admits one point, n_corr off by one, a step skipped, a chain cut short, a tie given to the higher index --
on every input the GPU tests use (tests/icp_step_cases.py), with the row recomputed by the long-double restatement of the step
and the rest of the chain continued correctly from it.  Per input the smallest effect of a swapped neighbour is printed and must
be at least 100 step tolerances: the bound is what does the work (with the chain-end tolerance of 1e-4 the same mutations pass)."""
import numpy as np
import pytest

import icp_step_cases as K
import icp_step_certificate as C
import oracle_lib as O

SWAPS_PER_STEP = 20
MARGIN = 100.0            # smallest swapped-neighbour effect / step tolerance
CASE_MODES = [(name, mode) for name in K.CASE_NAMES for mode in K.by_name(name).modes]

_traces = {}


def world(name, mode):
    """case, oracle model, and the oracle's own brute-force trace of the case (computed once, never changed: tests copy it)"""
    if (name, mode) not in _traces:
        case = K.by_name(name)
        _traces[name, mode] = (case, case.model(mode)) + C.oracle_trace(case.model(mode), case.batch, case.max_iter, case.min_delta,
                                                                        case.indist, K.OMODE[mode])
    return _traces[name, mode]


def cert(case, model, mode, trace, result, **kw):
    return C.certify(model, case.batch, trace, result, case.max_iter, case.min_delta, case.indist, K.OMODE[mode], **kw)


def steps_of(case, result, trace, mode, first=0):
    """(scan, step) of every executed step that moves the pose by more than 100 tolerances (a converged step is no step to speak
    of: skipping it changes nothing a tolerance could see)"""
    for s in range(case.batch.n_scans):
        for k in range(first, int(result["iters"][s])):
            if abs(trace[s, k, 6]) > MARGIN * C.STEP_TOL[K.OMODE[mode]]:
                yield s, k


def mutated_row(case, model, mode, trace, result, s, k, c):
    """the trace with row k of scan s recomputed from the (mutated) correspondences c and every later row continued by the oracle"""
    tr, res = trace.copy(), result.copy()
    Rk, tk = C.pose_before(case.batch, trace, s, k)
    tr[s, k] = C.restated_step(c, Rk, tk)
    C.continue_chain(model, case.batch, tr, res, s, k, case.max_iter, case.min_delta, case.indist, K.OMODE[mode])
    return tr, res


def correspondences(case, model, mode, trace, s, k):
    ga, nga = case.batch.scan(s)
    Rk, tk = C.pose_before(case.batch, trace, s, k)
    return C.Correspondences(model, ga, nga, Rk, tk, case.indist, K.OMODE[mode]), Rk, tk


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_accepts_the_oracles_own_trace_and_the_restatement_agrees(name, mode):
    case, model, trace, result, Rs, ts, corrs = world(name, mode)
    assert cert(case, model, mode, trace, result, R=Rs, t=ts) == 0.0
    worst = 0.0
    for s in range(case.batch.n_scans):
        for k in range(int(result["iters"][s])):
            c, Rk, tk = correspondences(case, model, mode, trace, s, k)
            assert np.array_equal(np.where(c.inlier, c.idx, -1), corrs[s][k]), (s, k)      # the same pairs as the oracle's step
            row = C.restated_step(c, Rk, tk)
            assert row[7] == trace[s, k, 7]
            worst = max(worst, np.abs(row[:7] - trace[s, k, :7]).max())
    print("%s %s: long-double restatement against the oracle's step %.3g" % (name, mode, worst))
    assert worst < 1e-13


def test_the_cases_reach_what_they_are_for():
    # outliers: the gate rejects some points and keeps some, in every step of every scan
    case, model, trace, result, _, _, _ = world("outliers", "p2p")
    for s in range(case.batch.n_scans):
        n = case.batch.scan_off[s + 1] - case.batch.scan_off[s]
        assert result["iters"][s] == case.max_iter and ((0 < trace[s, :, 7]) & (trace[s, :, 7] < n)).all(), s
    # ties: after the first step some query has two exactly equidistant neighbours of different index
    case, model, trace, result, _, _, _ = world("ties", "p2p")
    for s in range(case.batch.n_scans):
        for k in range(1, case.max_iter):
            c, _, _ = correspondences(case, model, "p2p", trace, s, k)
            tied = np.flatnonzero((c.dis == c.dis2) & (c.idx != c.idx2))
            assert set(range(K.N_TIE_QUERIES)) <= set(tied.tolist()) and (c.idx[tied] < c.idx2[tied]).all(), (s, k)
    # ... and the point-to-line step leaves none after its first, which is why that case is point-to-point only
    lmodel = case.model("p2l")
    ltrace = C.oracle_trace(lmodel, case.batch, case.max_iter, -1.0, case.indist, O.MODE_P2L)[0]
    left = 0
    for k in range(1, case.max_iter):
        c, _, _ = correspondences(case, lmodel, "p2l", ltrace, 0, k)
        left += int(((c.dis == c.dis2) & (c.idx != c.idx2)).sum())
    print("ties, point-to-line: %d exact ties after the first step" % left)
    assert left == 0
    # ragged: the scan of three points is left alone, every other runs; both empty classes are there
    case, model, trace, result, Rs, ts, _ = world("ragged", "p2p")
    sizes = np.diff(case.batch.scan_off)
    assert sizes.tolist() == K.RAGGED_SIZES and len(sizes) % 2 == 1
    assert [int(result["iters"][s]) for s in range(len(sizes))] == [0 if n < 5 else case.max_iter for n in sizes]
    assert (case.batch.scan_nga == 0).any() and (case.batch.scan_nga == sizes).any()
    # small_class: class GA's queries pair with nothing
    case, model, trace, result, _, _, _ = world("small_class", "p2p")
    assert len(case.m_ga) == 3 and (case.batch.scan_nga > 0).all()
    for s in range(case.batch.n_scans):
        assert (trace[s, :, 7] == case.batch.scan_off[s + 1] - case.batch.scan_off[s] - case.batch.scan_nga[s]).all()
    # early exit: scans stop before max_iter and the two scans of a pair stop apart
    for md in (1e-2, 1e-4):
        for mode in ("p2p", "p2l"):
            case, model, trace, result, _, _, _ = world("early_%g" % md, mode)
            it = result["iters"]
            assert (it < case.max_iter).any() and (it[0] != it[1] or it[2] != it[3]), (md, mode, it)
    # no two model points of a case nearer than about a millimetre
    for name in ("room", "ties"):
        case = K.by_name(name)
        for m in (case.m_ga, case.m_nga):
            f = m.astype(np.float32)
            d2 = ((f[:, None] - f[None]) ** 2).sum(-1) + np.eye(len(f))
            assert np.sqrt(d2.min()) > 1e-3, name


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_rejects_a_swapped_neighbour_at_every_step(name, mode):
    """One inlier's neighbour swapped for its second nearest, 20 random inliers per step: the smallest change of the row is at
    least 100 tolerances, and the certificate rejects that smallest one AT that step."""
    case, model, trace, result, _, _, _ = world(name, mode)
    rs = np.random.RandomState(31)
    smallest, n_steps = np.inf, 0
    for s, k in steps_of(case, result, trace, mode):
        c, Rk, tk = correspondences(case, model, mode, trace, s, k)
        pool = np.flatnonzero(c.inlier & (c.idx2 >= 0))
        best = None
        for j in rs.choice(pool, min(SWAPS_PER_STEP, len(pool)), replace=False):
            keep = c.idx[j]
            c.idx[j] = c.idx2[j]
            effect = np.abs(C.restated_step(c, Rk, tk)[:7] - trace[s, k, :7]).max()
            c.idx[j] = keep
            if best is None or effect < best[0]:
                best = (effect, j)
        smallest = min(smallest, best[0])
        c.idx[best[1]] = c.idx2[best[1]]
        tr, res = mutated_row(case, model, mode, trace, result, s, k, c)
        with pytest.raises(C.CertificateError) as e:
            cert(case, model, mode, tr, res, scans=[s])
        assert e.value.step == k and e.value.what in ("pose", "delta"), str(e.value)
        n_steps += 1
    tol = C.STEP_TOL[K.OMODE[mode]]
    print("%s %s: smallest effect of a swapped neighbour over %d steps %.3g = %.0f tolerances of %g" % (name, mode, n_steps, smallest, smallest / tol, tol))
    assert n_steps > 0 and smallest >= MARGIN * tol


def test_the_chain_end_tolerance_would_not_see_a_swapped_neighbour():
    """the same mutation held to POS_TOL = 1e-4 (what the chain-end checks of the suite ask) passes: the tight bound does the work"""
    case, model, trace, result, _, _, _ = world("room", "p2p")
    rs = np.random.RandomState(32)
    passed = tried = 0
    for s, k in steps_of(case, result, trace, "p2p"):
        c, Rk, tk = correspondences(case, model, "p2p", trace, s, k)
        j = rs.choice(np.flatnonzero(c.inlier))
        c.idx[j] = c.idx2[j]
        tr, res = mutated_row(case, model, "p2p", trace, result, s, k, c)
        tried += 1
        try:
            cert(case, model, "p2p", tr, res, scans=[s], tol=1e-4)
            passed += 1
        except C.CertificateError:
            pass
        with pytest.raises(C.CertificateError):
            cert(case, model, "p2p", tr, res, scans=[s])
    print("room p2p: %d of %d swapped neighbours pass a tolerance of 1e-4; none passes %g" % (passed, tried, C.STEP_TOL[O.MODE_P2P]))
    assert passed > tried // 2


def test_rejects_a_gate_that_drops_or_admits_one_point():
    """outliers, point-to-point (the point-to-line step has no gate): the inlier nearest the gate dropped, the outlier nearest
    the gate admitted (n_corr tells), and both at once -- n_corr is right and the pose must tell"""
    case, model, trace, result, _, _, _ = world("outliers", "p2p")
    n = 0
    for s, k in steps_of(case, result, trace, "p2p"):
        c, Rk, tk = correspondences(case, model, "p2p", trace, s, k)
        searched = c.idx >= 0
        inside = np.flatnonzero(searched & c.inlier)
        outside = np.flatnonzero(searched & ~c.inlier)
        drop, admit = inside[np.argmax(c.dis[inside])], outside[np.argmin(c.dis[outside])]
        for flips, what in (([drop], ("n_corr",)), ([admit], ("n_corr",)), ([drop, admit], ("pose", "delta"))):
            c.inlier[flips] ^= True
            tr, res = mutated_row(case, model, "p2p", trace, result, s, k, c)
            c.inlier[flips] ^= True
            with pytest.raises(C.CertificateError) as e:
                cert(case, model, "p2p", tr, res, scans=[s])
            assert e.value.step == k and e.value.what in what, str(e.value)
            n += 1
    assert n >= 3 * case.batch.n_scans * case.max_iter // 2


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_rejects_wrong_counts_skipped_steps_and_short_chains(name, mode):
    case, model, trace, result, _, _, _ = world(name, mode)
    n = 0
    for s, k in steps_of(case, result, trace, mode):
        # n_corr off by one, the pose unchanged
        for off in (1, -1):
            tr = trace.copy()
            tr[s, k, 7] += off
            res = result.copy()
            if k + 1 == res["iters"][s]:
                res["n_corr"][s] += off
            with pytest.raises(C.CertificateError) as e:
                cert(case, model, mode, tr, res, scans=[s])
            assert (e.value.step, e.value.what) == (k, "n_corr")
        # a row repeated: step k skipped, the chain continued from there
        if k > 0:
            tr, res = trace.copy(), result.copy()
            tr[s, k] = tr[s, k - 1]
            C.continue_chain(model, case.batch, tr, res, s, k, case.max_iter, case.min_delta, case.indist, K.OMODE[mode])
            with pytest.raises(C.CertificateError) as e:
                cert(case, model, mode, tr, res, scans=[s])
            assert e.value.step == k and e.value.what in ("pose", "delta", "n_corr"), str(e.value)
        n += 1
    for s in range(case.batch.n_scans):
        it = int(result["iters"][s])
        if it < 2:
            continue
        # iters one short, the rows as they were
        res = result.copy()
        res["iters"][s] = it - 1
        with pytest.raises(C.CertificateError) as e:
            cert(case, model, mode, trace, res, scans=[s])
        assert e.value.what in ("iters", "result", "unwritten"), str(e.value)
        # the chain stops early although delta >= min_delta: consistent in itself, one step missing
        tr, res = trace.copy(), result.copy()
        tr[s, it - 1] = np.nan
        res[s] = (it - 1, tr[s, it - 2, 7], tr[s, it - 2, 6])
        with pytest.raises(C.CertificateError) as e:
            cert(case, model, mode, tr, res, scans=[s])
        assert e.value.what == "iters", str(e.value)
        # the result is not the last row
        res = result.copy()
        res["delta"][s] = trace[s, it - 2, 6]
        with pytest.raises(C.CertificateError) as e:
            cert(case, model, mode, trace, res, scans=[s])
        assert e.value.what == "result"
    assert n > 0
    # a scan of fewer than five points: no step, no row, the pose untouched
    for s in np.flatnonzero(np.diff(case.batch.scan_off) < 5):
        _, _, _, _, Rs, ts, _ = world(name, mode)
        res = result.copy()
        res["iters"][s] = 1
        with pytest.raises(C.CertificateError):
            cert(case, model, mode, trace, res, scans=[s])
        tr = trace.copy()
        tr[s, 0] = 0.0
        with pytest.raises(C.CertificateError):
            cert(case, model, mode, tr, result, scans=[s])
        moved = ts.copy()
        moved[s, 0] += 1e-12
        with pytest.raises(C.CertificateError):
            cert(case, model, mode, trace, result, scans=[s], R=Rs, t=moved)


def test_rejects_a_tie_given_to_the_higher_index():
    case, model, trace, result, _, _, _ = world("ties", "p2p")
    n, smallest = 0, np.inf
    for s in range(case.batch.n_scans):
        for k in range(1, case.max_iter):
            c, Rk, tk = correspondences(case, model, "p2p", trace, s, k)
            for j in range(K.N_TIE_QUERIES):
                assert c.dis[j] == c.dis2[j] and c.idx[j] < c.idx2[j]
                keep = c.idx[j]
                c.idx[j] = c.idx2[j]
                tr, res = mutated_row(case, model, "p2p", trace, result, s, k, c)
                c.idx[j] = keep
                smallest = min(smallest, np.abs(tr[s, k, :7] - trace[s, k, :7]).max())
                with pytest.raises(C.CertificateError) as e:
                    cert(case, model, "p2p", tr, res, scans=[s])
                assert e.value.step == k and e.value.what in ("pose", "delta"), str(e.value)
                n += 1
    print("ties p2p: smallest effect of a tie given to the higher index %.3g over %d mutations" % (smallest, n))
    assert n == case.batch.n_scans * (case.max_iter - 1) * K.N_TIE_QUERIES and smallest >= MARGIN * C.STEP_TOL[O.MODE_P2P]
