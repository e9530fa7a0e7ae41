"""Every executed step of every form of the registration kernels against ONE brute-force step of the oracle from the device's
own previous pose (tests/icp_step_certificate.py): equal n_corr, the pose and delta within the step tolerance, the iteration rule
from the device's own deltas, untouched rows still NaN -- and two runs of every fit bit for bit the same.  What only a fit's final
pose could show before -- the seeded ring search and its one-pass disks, the halo-list sweeps with their cooperative round and
exact pass, the pair form, the spread form's search from the last neighbour, the staged tiles -- is held to the neighbour here:
tests/test_icp_step_certificate.py shows on the CPU that ONE wrong neighbour in ONE step of these inputs moves a row by at least
100 tolerances.  The inputs are tests/icp_step_cases.py; the numbers measured are in docs/ICP_STEP_CERTIFICATE.md."""
import numpy as np
import pytest

import icp_step_cases as K
import icp_step_certificate as C
from slam_amd import api

pytestmark = pytest.mark.gpu

SPREAD = 16               # batches of up to this many scans in the spread form (every case has fewer)
ONE_PER_WG = dict(spread_scans=-1, pair_scans=-1)
# what slam_icp_params selects (icp.hip launch_fit, icp_single.hip).  The hand-over of the default schedule waits for the guard
# (far_div) and, point-to-point, for ten ring iterations: the forms that are to hand over inside these short fits say far_div = 1.
FORMS = {
    "fused": ONE_PER_WG,                                                       # the default schedule, one scan per workgroup
    "ring1": dict(spread_scans=-1, lanes_per_point=1),                         # the ring search for every iteration
    "ring2": dict(spread_scans=-1, lanes_per_point=2),
    "ring4": dict(spread_scans=-1, lanes_per_point=4),
    "ring8": dict(spread_scans=-1, lanes_per_point=8),
    "ring16": dict(spread_scans=-1, lanes_per_point=16),
    "ring32": dict(spread_scans=-1, lanes_per_point=32),
    "ring64": dict(spread_scans=-1, lanes_per_point=64),
    "ring_per_pass": dict(spread_scans=-1, lanes_per_point=-1),
    "lists": dict(spread_scans=-1, lanes_per_point=-2),                        # the list sweeps for every iteration
    "split": dict(split_launch=1, first_iterations=2, far_div=1, **ONE_PER_WG),   # the two forms as two launches
    "first1": dict(first_iterations=1, far_div=1, **ONE_PER_WG),               # ring search, then lists, in one launch
    "first2": dict(first_iterations=2, far_div=1, **ONE_PER_WG),
    "pair1": dict(spread_scans=-1, pair_scans=1),                              # two scans per workgroup
    "pair2": dict(spread_scans=-1, pair_scans=2),
    "pair2_first1": dict(spread_scans=-1, pair_scans=2, first_iterations=1, far_div=1),   # ... handing over inside the fit
    "global": dict(force_global=1, **ONE_PER_WG),                              # the index in HBM / L2
    "wave_tiles": dict(spread_scans=-1, force_global=1, lanes_per_point=2, wave_tiles=1),   # ... staged per wavefront
    "spread": dict(spread_scans=SPREAD),                                       # many workgroups per scan
    "spread_tile1": dict(spread_scans=SPREAD, force_global=1, spread_tile=1),
    "spread_tile2": dict(spread_scans=SPREAD, force_global=1, spread_tile=2),
    "spread_no_tile": dict(spread_scans=SPREAD, force_global=1, spread_tile=-1),
    "spread_handed_over": dict(spread_scans=SPREAD, spread_wait_us=-1),        # redone by the one-workgroup form
}
CASE_MODES = [(name, mode) for name in K.CASE_NAMES for mode in K.by_name(name).modes]

measured = {}             # (form, mode) -> largest |device - oracle| over the cases, printed when the module is done


def fit(icp, case):
    """one fit with a result and a trace buffer of the test's own, the trace filled with NaN"""
    b = case.batch
    S = b.n_scans
    d = [api.DeviceArray.from_host(a, dt) for a, dt in ((b.pts, np.float64), (b.scan_off, np.int32), (b.scan_nga, np.int32),
                                                        (b.R, np.float64), (b.t, np.float64))]
    d_res = api.DeviceArray((S,), api.RESULT_DTYPE)
    d_res.zero()
    d_tr = api.DeviceArray.from_host(np.full((S, case.max_iter, 8), np.nan), np.float64)
    icp.fit_batch_dev(d[0], d[1], d[2], S, d[3], d[4], case.indist, d_res, d_tr)
    api.synchronize()
    return d[3].download(), d[4].download(), d_res.download(), d_tr.download()


@pytest.mark.parametrize("name,mode", CASE_MODES)
@pytest.mark.parametrize("form", list(FORMS))
def test_every_step_of_every_form(form, name, mode):
    case = K.by_name(name)
    assert case.batch.n_scans <= SPREAD and 4 <= case.max_iter <= 12
    kw = dict(FORMS[form], max_iter=case.max_iter, min_delta=case.min_delta)
    if mode == "p2l":
        kw.update(mode=api.ICP_P2L, normals_k=10)
        if kw.get("split_launch"):
            # the point-to-line solver has the one-launch schedule only: the request is refused, not ignored
            with pytest.raises(api.SlamError) as e:
                api.Icp(case.m_ga, case.m_nga, **kw)
            assert e.value.code == api.E_UNSUPPORTED
            return
    icp = api.Icp(case.m_ga, case.m_nga, **kw)
    info = icp.index_info()
    assert info["in_lds"] == (not kw.get("force_global"))
    if "first_iterations" in kw:
        assert info["two_forms"] and info["first_iterations"] == kw["first_iterations"]
    R, t, res, trace = fit(icp, case)
    R2, t2, res2, trace2 = fit(icp, case)
    icp.close()
    assert np.array_equal(R, R2) and np.array_equal(t, t2) and np.array_equal(res, res2)            # reproducible to the bit
    assert np.array_equal(trace, trace2, equal_nan=True)
    model, omode = case.model(mode), K.OMODE[mode]
    args = (model, case.batch, trace, res, case.max_iter, case.min_delta, case.indist, omode)
    worst = C.certify(*args, R=R, t=t, tol=np.inf)       # the counts and the iteration rule; the figure before it is held to the bound
    print("%s %s %s: largest |device - oracle| of a step %.3g (tolerance %g)" % (form, name, mode, worst, C.STEP_TOL[omode]))
    measured[form, mode] = max(measured.get((form, mode), 0.0), worst)
    C.certify(*args, R=R, t=t)


@pytest.mark.parametrize("mode", ["p2p", "p2l"])
def test_the_room_reaches_the_seeded_search(mode):
    """proved on the host from the oracle's poses: seed disks beyond 3 x 3 cells read in one pass, rows clipped by their chord,
    levels entered without a candidate and probed (ring_restatement.py)"""
    from test_gpu_icp_ring_prune import reach_counts_fit
    case = K.room()
    kw = dict(mode=api.ICP_P2L, normals_k=10) if mode == "p2l" else {}
    icp = api.Icp(case.m_ga, case.m_nga, max_iter=case.max_iter, min_delta=-1.0, **ONE_PER_WG, **kw)
    info = icp.index_info()
    icp.close()
    un, se = reach_counts_fit(info, case.m_ga, case.m_nga, case.model(mode), case.batch, mode == "p2l")
    print("unseeded", un, "seeded", se)
    assert se.get("big", 0) > 0 and se.get("onepass", 0) > 0 and se.get("clipped", 0) > 0, se
    assert un.get("probed", 0) > 0 and un.get("clipped", 0) > 0, un


def test_the_outliers_stay_beyond_the_lists():
    """the list forms' far queries: at every pose of the oracle's chain some queries of the outlier scans lie beyond the lists'
    certified radius -- they go to the cooperative round"""
    case = K.outliers()
    icp = api.Icp(case.m_ga, case.m_nga, max_iter=case.max_iter, min_delta=-1.0, first_iterations=1, far_div=1, **ONE_PER_WG)
    info = icp.index_info()
    icp.close()
    assert info["two_forms"]
    model = case.model("p2p")
    trace = C.oracle_trace(model, case.batch, case.max_iter, -1.0, case.indist, K.OMODE["p2p"])[0]
    for s in (0, 2):
        ga, nga = case.batch.scan(s)
        for k in range(1, case.max_iter):
            Rk, tk = C.pose_before(case.batch, trace, s, k)
            c = C.Correspondences(model, ga, nga, Rk, tk, case.indist, K.OMODE["p2p"])
            far = int((np.sqrt(c.dis) > info["list_certified_radius"]).sum())
            assert far > 0, (s, k)


@pytest.fixture(scope="module", autouse=True)
def report_the_measured_maxima():
    """after the module: per form and solver the largest deviation of a step over all cases (docs/ICP_STEP_CERTIFICATE.md)"""
    yield
    for mode in ("p2p", "p2l"):
        rows = {f: v for (f, m), v in measured.items() if m == mode}
        for f in FORMS:
            if f in rows:
                print("\nmeasured %s %-20s %.3g" % (mode, f, rows[f]), end="")
        if rows:
            print("\nmeasured %s maximum %.3g, tolerance %g" % (mode, max(rows.values()), C.STEP_TOL[K.OMODE[mode]]))
