"""The scan-context restatement (tests/cpp/sc_oracle.cpp) on its own: against plain numpy on random and edge clouds, the
symmetries of the search, its tables against numpy's libm, and the mutations -- every decision of the contract, restated
wrongly, changes at least one case of tests/sc_cases.py.  No GPU."""
import numpy as np
import pytest

import sc_cases as K
import sc_oracle as SO


def ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("name", sorted(K.PARAM_SETS))
def test_tables_agree_with_libm_within_one_ulp(name):
    p = K.PARAM_SETS[name]
    e, c, s = SO.tables(p)
    k = np.arange(p.n_sectors // 4)
    assert ulps(c, np.cos(2.0 * np.pi * k / p.n_sectors)).max() <= 1 and ulps(s, np.sin(2.0 * np.pi * k / p.n_sectors)).max() <= 1
    edge = (np.arange(p.n_rings) + 1) * (p.max_range / p.n_rings)
    assert np.array_equal(e, edge * edge)
    assert np.array_equal(edge.astype(np.float32).astype(np.float64), edge)   # f32 coordinates reach the ring edges exactly
    assert c[0] == 1.0 and s[0] == 0.0 and np.all(np.diff(e) > 0)


@pytest.mark.parametrize("name", sorted(K.PARAM_SETS))
def test_descriptor_equals_numpy_brute_force(name):
    p = K.PARAM_SETS[name]
    tabs = SO.tables(p)
    clouds = K.descriptor_clouds(p, tabs) + [("random_%d" % k, K.random_cloud(40 + k, 777, p)) for k in range(3)]
    for cname, cloud in clouds:
        d = SO.descriptor(cloud, p, tabs)
        assert np.array_equal(d, K.numpy_descriptor(cloud, p, tabs)), cname
        rs = np.random.RandomState(5)                    # any order of the points, the same cells
        assert np.array_equal(d, SO.descriptor(cloud[rs.permutation(len(cloud))], p, tabs)), cname


def test_hand_worked_cells():
    p = SO.Params()                                      # rings of 4 m, 64 sectors, bins of 2 cm from -2 m
    d = SO.descriptor([[4.0, 0.0, 0.0], [0.0, 0.0, -2.0], [-1.0, 0.0, 10.0], [0.0, -79.0, -5.0], [80.0, 0.0, 0.0]], p)
    want = np.zeros((20, 64), np.uint8)
    want[1, 0] = 101                                     # on the edge of ring 0: ring 1; z = 0 is bin 100
    want[0, 0] = 1                                       # the origin, at z_min: bin 0 is code 1
    want[0, 32] = 255                                    # the negative x axis opens the third quadrant; above the top bin
    want[19, 48] = 1                                     # the negative y axis opens the fourth; below z_min clamps to bin 0
    assert np.array_equal(d, want)                       # and 80 m is beyond the last ring


def test_edge_clouds_hold_exact_ring_edges_and_sector_ties():
    """what the mutations below rest on, said directly: the 'exact' edge cloud has points with r2 == edge2[k] and, where a
    boundary lies on the diagonal, points whose two rounded products are equal"""
    for p in K.PARAM_SETS.values():
        e, c, s = SO.tables(p)
        a = K.edge_cloud(p, (e, c, s), "exact").astype(np.float64)
        a = a[np.isfinite(a).all(axis=1)]
        r2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        assert np.isin(e, r2).all()
        per = p.n_sectors // 4
        if per % 2 == 0:
            k = per // 2
            ties = (a[:, 1] * c[k] == a[:, 0] * s[k]) & (a[:, 0] > 0) & (a[:, 1] > 0)
            assert ties.any()


def test_search_equals_numpy_and_is_symmetric():
    p = SO.Params(n_rings=6, n_sectors=20, max_range=30.0)
    tabs = SO.tables(p)
    descs = [SO.descriptor(K.random_cloud(60 + k, 150, p), p, tabs) for k in range(8)]
    for sets in K.match_sets(p).values():
        descs += [SO.descriptor(c, p, tabs) for c in sets[:3]]
    for i, a in enumerate(descs):
        for j, b in enumerate(descs):
            ab, ba = SO.match(a, b), SO.match(b, a)
            assert ab == K.numpy_match(a, b), (i, j)
            assert ab[0] == ba[0]                        # D_min(a, b) == D_min(b, a)
            assert (ab[2], ab[3]) == (ba[3], ba[2])
            d = K.numpy_distances(a, b)
            if (d == d.min()).sum() == 1:                # the minimum at one shift only: the shifts are opposite, the overlap the same
                assert (ab[1] + ba[1]) % p.n_sectors == 0 and ab[4] == ba[4], (i, j)


def test_rolled_descriptor_is_found_at_its_shift():
    p = SO.Params(n_sectors=60)
    a = SO.descriptor(K.random_cloud(70, 900, p), p)
    for s in (0, 1, 7, 59):
        m = SO.match(np.roll(a, s, axis=1), a)           # the candidate rolled by +s lies on the query
        assert m[:2] == (0, s) and m[2] == m[3] == m[4]
        assert SO.match(a, np.roll(a, s, axis=1))[:2] == (0, (-s) % 60)


def test_tie_takes_the_lowest_shift():
    p = SO.Params()
    a, b = [SO.descriptor(c, p) for c in K.match_sets(p)["tie"]]
    d = K.numpy_distances(a, b)
    assert sorted(np.flatnonzero(d == d.min())) == [3, p.n_sectors - 2]
    assert SO.match(a, b)[:2] == (int(d.min()), 3)


def cases_differ(mutation):
    """the names of the cases that the mutated restatement changes"""
    hit = []
    for pname, p in sorted(K.PARAM_SETS.items()):
        tabs = SO.tables(p)
        for cname, cloud in K.descriptor_clouds(p, tabs):
            if not np.array_equal(SO.descriptor(cloud, p, tabs), SO.descriptor(cloud, p, tabs, mutation)):
                hit.append("%s/%s" % (pname, cname))
        for sname, clouds in sorted(K.match_sets(p).items()):
            if sname == "seventy":
                clouds = clouds[:4]
            d = [SO.descriptor(c, p, tabs) for c in clouds]
            dm = [SO.descriptor(c, p, tabs, mutation) for c in clouds]
            if any(SO.match(d[i], d[j]) != SO.match(dm[i], dm[j], mutation) for i in range(len(d)) for j in range(len(d)) if i != j):
                hit.append("%s/match_%s" % (pname, sname))
    return hit


@pytest.mark.parametrize("name", sorted(SO.MUTATIONS))
def test_every_mutation_changes_a_case(name):
    hit = cases_differ(SO.MUTATIONS[name])
    print(name, hit)
    assert hit, "no case of sc_cases.py reaches the decision that '%s' restates wrongly" % name
    want = {"ring_strict": "edges_exact", "sector_strict": "edges_exact", "quadrant_turn": "edges_", "tie_highest": "match_tie",
            "roll_direction": "match_rolled", "h_no_plus_one": "edges_"}[name]
    assert any(want in h for h in hit), hit
