"""The raycast held to the oracle's sequential integer Bresenham at every edge it has: the cases of tests/grid_raycast_cases.py
(shown to reach their edges in tests/test_grid_raycast_cases.py) through the tiled, the merging tiled and the global-atomics
form.  Counts and total_updates() are integers and compared as such; after every call the reported dirty rows must cover every
storage row that holds a count, and on a grid that was never rolled be exactly the lowest and the highest such row.  The clip
itself, at sizes no device test reaches in seconds: tests/test_grid_clip.py.  docs/GRID_RAYCAST.md has the table of edges."""
import numpy as np
import pytest

import grid_raycast_cases as RC
import oracle_lib as O
from slam_amd import api

pytestmark = pytest.mark.gpu

IMPLS = [api.RAYCAST_TILED, api.RAYCAST_TILED_MERGE, api.RAYCAST_GLOBAL]
IMPL_IDS = ["tiled", "tiled_merge", "global"]


_last = {}     # the case in work and the oracle's planes for it: built once, shared by the three forms (which run back to back)


def reference(key, build):
    """-> case, oracle hits, misses, updates; `build`: () -> case, called once per key"""
    if _last.get("key") != key:
        _last.clear()
        case = build()
        g = O.grid_params(case.size_x, case.size_y, case.res, case.kwargs.get("max_range", 75.0), 1.0, 0.3, 0, case.kwargs["rolling"])
        _last.update(key=key, value=(case,) + tuple(O.grid_raycast(g, case.origin, case.end)))
    return _last["value"]


def compare(g, impl, want_h, want_m, want_n, rolled=False):
    api.synchronize()
    h, m = g.read_counts()
    for name, got, want in (("hits", h, want_h), ("misses", m, want_m)):
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            some = [(int(c % g.size_x), int(c // g.size_x), int(got[c]), int(want[c])) for c in bad[:12]]
            raise AssertionError("%s differ in %d cells; (x, y, device, oracle): %s" % (name, len(bad), some))
    assert g.total_updates() == want_n
    rows = np.flatnonzero(((want_h != 0) | (want_m != 0)).reshape(g.size_y, g.size_x).any(axis=1))
    lo, hi = g.dirty_rows()
    if rows.size == 0:
        assert (lo, hi) == (0, -1)
        return
    srows = (rows + g.info()["origin_y"]) % g.size_y
    assert lo <= srows.min() and hi >= srows.max(), ((lo, hi), (srows.min(), srows.max()))
    if not rolled and impl != api.RAYCAST_GLOBAL:
        assert (lo, hi) == (srows.min(), srows.max())


@pytest.mark.parametrize("impl", IMPLS, ids=IMPL_IDS)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_bit_exact(name, impl):
    case, want_h, want_m, want_n = reference(name, RC.CASES[name])
    g = api.Grid(case.size_x, case.size_y, case.res, raycast_impl=impl, **case.kwargs)
    g.raycast(case.origin, case.end)
    compare(g, impl, want_h, want_m, want_n)
    if name.startswith("counter_carry-wg1") and impl != api.RAYCAST_GLOBAL:
        # one workgroup took all 1100 blocks of the one tile: the packed counters forced a write-back after 1023
        assert g.raycast_stats()["tile_write_backs"] >= 2
    g.close()


_prior = []


def prior_reference():
    if not _prior:
        prior = RC.ragged_prior()
        g = O.grid_params(prior.size_x, prior.size_y, prior.res, prior.kwargs["max_range"], 1.0, 0.3, 0, prior.kwargs["rolling"])
        _prior.extend((prior,) + tuple(O.grid_raycast(g, prior.origin, prior.end)))
    return _prior


@pytest.mark.parametrize("impl", IMPLS, ids=IMPL_IDS)
@pytest.mark.parametrize("n", RC.RAGGED_N)
def test_ragged_counts_after_a_larger_call(n, impl):
    """n beams on a handle that has just raycast 5 000 others: the scratch holds live stale beams behind n"""
    case, want_h, want_m, want_n = reference(("ragged", n), lambda: RC.ragged_counts(n))
    prior, ph, pm, pn = prior_reference()
    g = api.Grid(case.size_x, case.size_y, case.res, raycast_impl=impl, **case.kwargs)
    g.raycast(prior.origin, prior.end)
    compare(g, impl, ph, pm, pn)
    g.raycast(case.origin, case.end)
    compare(g, impl, ph + want_h, pm + want_m, pn + want_n)
    g.close()


@pytest.mark.parametrize("impl", IMPLS, ids=IMPL_IDS)
def test_scans_on_a_rolled_window(impl):
    """slam_grid_raycast_scans_dev after two moves that are no whole numbers of cells: the seam lies inside a tile and in the
    middle of the scans; one scan is empty, one point NaN"""
    case, want_h, want_m, want_n = reference("scans_rolling", lambda: RC.scans_rolling(O.transform_points))
    s = RC.scans_rolling_inputs()
    g = api.Grid(case.size_x, case.size_y, case.res, raycast_impl=impl, **case.kwargs)
    for pose in s.poses:
        g.set_pose(*pose)
    assert (g.size_x - g.info()["origin_x"]) % RC.TILE and (g.size_y - g.info()["origin_y"]) % RC.TILE
    d = [api.DeviceArray.from_host(a, dt) for a, dt in ((s.pts, np.float64), (s.scan_off, np.int32), (s.R, np.float64), (s.t, np.float64))]
    g.raycast_scans_dev(d[0], d[1], len(s.scan_off) - 1, len(s.pts), d[2], d[3])
    compare(g, impl, want_h, want_m, want_n, rolled=True)
    g.close()
