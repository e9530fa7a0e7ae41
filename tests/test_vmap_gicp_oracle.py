"""The restatement of the voxel map's moments, plane distributions and Generalized ICP against them
(tests/cpp/vmap_gicp_oracle.cpp) against hand-worked values of docs/VOXEL_MAP.md section 9, Python's integers and its own
mutations (truncation for floor in e, '<=' for '<' at the gate, non-plane voxels paired, the lowest-key tie rule dropped),
each caught by a test named here.  Then what the library answers without a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import kf_gicp_oracle as KG
import vmap_gicp_cases as G
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api

I6 = np.array([1.0, 0, 0, 1.0, 0, 1.0])


def voxel(d, key):
    """the fields of the voxel with this key"""
    i = int(np.flatnonzero(d["key"] == np.uint64(key))[0])
    return {k: v[i] for k, v in d.items()}


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize("leaf", G.LEAVES)
def test_hand_worked_moments(leaf):
    m = VG.OracleDistMap(leaf)
    p, key, e, M = G.negative_point(leaf)
    c, ckey = G.corner_point(leaf)
    assert m.integrate(np.concatenate([p, c])) == 0
    d = m.read()
    v = voxel(d, key)
    assert v["count"] == 1 and tuple(int(x) for x in v["E"]) == e and tuple(int(x) for x in v["M"]) == M
    assert e == (G.L_of(leaf) // 32, 3 * G.L_of(leaf) // 64, G.L_of(leaf) // 64)
    v = voxel(d, ckey)
    assert v["count"] == 1 and not v["E"].any() and not v["M"].any()
    assert tuple(v["centroid"]) == (G.F(leaf), G.F(-leaf), G.F(0))


def test_floor_not_truncation_in_e():
    leaf, p, key, e = G.negative_d_point()
    m = VG.OracleDistMap(leaf)
    m.integrate(p)
    v = voxel(m.read(), key)
    assert tuple(int(x) for x in v["E"]) == e and tuple(int(x) for x in v["M"]) == (1, 1, 1, 1, 1, 1)
    assert G.python_moments(p, leaf) == ([-1, -1, -1], [1] * 6)


def test_mutation_truncated_e_is_caught():
    leaf, p, key, e = G.negative_d_point()
    m = VG.OracleDistMap(leaf, mutation=VG.MUT_TRUNCATE_E)
    m.integrate(p)
    v = voxel(m.read(), key)
    assert tuple(int(x) for x in v["E"]) == (0, 0, 0) != e


@pytest.mark.parametrize("leaf", G.LEAVES + (0.30,))
def test_moments_against_python_integers(leaf):
    """2 000 points in one voxel (cell 2 on every axis at each leaf)"""
    pts = ((K_one_voxel() - 0.5) * (leaf / 0.25) * 0.999 + 2.0 * leaf + 0.0005 * leaf).astype(np.float32)
    m = VG.OracleDistMap(leaf)
    assert m.integrate(pts) == 0
    d = m.read()
    assert len(d["key"]) == 1 and d["count"][0] == 2000 and d["key"][0] == G.key_of(2, 2, 2)
    E, M = G.python_moments(pts, leaf)
    assert [int(x) for x in d["E"][0]] == E and [int(x) for x in d["M"][0]] == M


def K_one_voxel():
    import vmap_cases as K
    return K.one_voxel(2000).astype(np.float64)


def test_any_order_of_points_and_clouds_gives_the_same_bits():
    maps = []
    for order in G.ORDERS:
        m = VG.OracleDistMap(1.0)
        for k in order:
            cloud, (R, t) = G.FOUR_CLOUDS[k]
            m.integrate(cloud, R, t)
        maps.append(m.read())
    m = VG.OracleDistMap(1.0)
    rng = np.random.default_rng(5)
    for k in range(4):
        cloud, (R, t) = G.FOUR_CLOUDS[k]
        m.integrate(cloud[rng.permutation(len(cloud))], R, t)
    maps.append(m.read())
    assert maps[0]["flag"].sum() > 0 and len(maps[0]["key"]) > 100
    for other in maps[1:]:
        for f in maps[0]:
            assert VG.same_bits(maps[0][f], other[f]), f


def test_sums_and_keys_are_the_plain_maps():
    """a map with distributions holds the sums, counts and keys of tests/cpp/vmap_oracle.cpp"""
    a, b = VG.OracleDistMap(0.25), V.OracleMap(0.25)
    for cloud, (R, t) in G.FOUR_CLOUDS:
        assert a.integrate(cloud, R, t) == b.integrate(cloud, R, t)
    d, (xyz4, count, key, sums) = a.read(), b.extract()
    assert VG.same_bits(d["key"], key) and VG.same_bits(d["count"], count) and VG.same_bits(d["sums"], sums)
    assert VG.same_bits(d["centroid"], np.ascontiguousarray(xyz4[:, :3]))


def test_enable_refusals():
    with pytest.raises(ValueError):
        VG.OracleDistMap(8.5)
    VG.OracleDistMap(8.0)
    m = VG.OracleDistMap(1.0)
    m.integrate(np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        m.enable()
    m.clear()
    m.enable(min_points=4)


# ------------------------------------------------------------------ distributions
@pytest.mark.parametrize("leaf", G.LEAVES)
def test_hand_worked_distributions(leaf):
    m = VG.OracleDistMap(leaf, min_points=4)
    (sq, ksq), (ln, kln), (bl, kbl) = G.square(leaf), G.line(leaf), G.blob(leaf)
    few, kfew = G.too_few(leaf, min_points=4, cell=(10, 0, 0))
    m.integrate(np.concatenate([sq, ln, bl, few]))
    d = m.read()
    v = voxel(d, ksq)
    assert v["flag"] == 1 and tuple(v["normal"]) == (0.0, 0.0, 1.0)
    assert tuple(v["cov6"]) == (1.0, 0.0, 0.0, 1.0, 0.0, G.EPS)                     # diag(1, 1, eps) to the bit
    assert tuple(v["eig"]) == (leaf * leaf / 16, leaf * leaf / 16, 0.0)
    assert tuple(v["centroid"]) == tuple(np.float32([4.5 * leaf, 0.5 * leaf, 0.5 * leaf]))
    v = voxel(d, kln)
    assert v["flag"] == 0 and v["count"] == 6 and v["eig"][0] > 0 and v["eig"][1] == 0 and not v["cov6"].any() and not v["normal"].any()
    v = voxel(d, kbl)
    # per axis e = c +- o twice and c four times with c = L / 32, o = L / 64: M / 6 is not exact, so the contract's own
    # operations in doubles; leaf^2 / 48 up to that rounding
    c, o = G.L_of(leaf) // 32, G.L_of(leaf) // 64
    lam = (float(6 * c * c + 2 * o * o) / 6.0 - float(c) * float(c)) * 2.0 ** -32
    assert v["flag"] == 0 and v["count"] == 6 and v["eig"][0] == v["eig"][1] == v["eig"][2] == lam
    assert lam == pytest.approx(leaf * leaf / 48, rel=1e-9)
    v = voxel(d, kfew)
    assert v["flag"] == 0 and v["count"] == 3 and v["eig"][2] == 0
    # the same voxel with one point more is a plane voxel: the count alone kept it out
    m2 = VG.OracleDistMap(leaf, min_points=4)
    m2.integrate(G.too_few(leaf, min_points=5, cell=(10, 0, 0))[0])
    assert voxel(m2.read(), kfew)["flag"] == 1


def test_default_min_points_is_six():
    m = VG.OracleDistMap(1.0)
    m.integrate(np.concatenate([G.too_few(1.0, 6)[0], G.too_few(1.0, 7, cell=(12, 0, 0))[0]]))
    d = m.read()
    assert voxel(d, G.too_few(1.0, 6)[1])["flag"] == 0 and voxel(d, G.key_of(12, 0, 0))["flag"] == 1


def test_carved_rule_is_part_of_the_plane_rule_when_asked():
    sq, key = G.square(1.0)
    for num, den, miss, want in ((0, 0, 5, 1), (1, 1, 5, 0), (1, 1, 2, 1), (1, 1, 3, 0)):
        m = VG.OracleDistMap(1.0, min_points=4, max_miss_num=num, max_miss_den=den)
        m.integrate(sq)
        m.set_carve([2], [miss], [key])          # seen 2: kept iff miss den <= 2 num
        assert voxel(m.read(), key)["flag"] == want, (num, den, miss)


def test_plane_covariance_agrees_with_the_stores():
    """on a tilted plane the voxel's C' is the store's plane_covariance of the same raw covariance, bit for bit"""
    rng = np.random.default_rng(2)
    uv = rng.uniform(0.1, 0.9, (40, 2))
    pts = np.stack([uv[:, 0], uv[:, 1], 0.3 + 0.2 * uv[:, 0] + 0.1 * uv[:, 1]], axis=1).astype(np.float32)
    m = VG.OracleDistMap(1.0)
    m.integrate(pts)
    v = voxel(m.read(), G.key_of(0, 0, 0))
    E, M, n = v["E"].astype(np.float64), v["M"].astype(np.float64), 40.0
    mu, s = E / n, M / n
    raw = np.array([(s[0] - mu[0] * mu[0]), (s[1] - mu[0] * mu[1]), (s[2] - mu[0] * mu[2]), (s[3] - mu[1] * mu[1]), (s[4] - mu[1] * mu[2]),
                    (s[5] - mu[2] * mu[2])]) * 2.0 ** -32
    assert v["flag"] == 1 and VG.same_bits(v["cov6"], KG.plane_covariance(raw, G.EPS))
    want = np.array([0.2, 0.1, -1.0]) / np.linalg.norm([0.2, 0.1, -1.0])
    assert abs(abs(v["normal"] @ want) - 1.0) < 1e-6          # quantisation to 2^-16 m tilts it by less


# ------------------------------------------------------------------ the pairs
def two_patches():
    """cell (0, 0, 0): a patch perpendicular to x through the centre; cell (1, 0, 0): one perpendicular to z; both centroids are
    the cell centres exactly"""
    m = dict(a=G.plane_patch((0, 0, 0), 0, n=4), b=G.plane_patch((1, 0, 0), 2, n=4))
    return m


def pairs_map(mutation=VG.MUT_NONE, with_line=False):
    m = VG.OracleDistMap(1.0, mutation=mutation)
    p = two_patches()
    m.integrate(np.concatenate([p["a"], p["b"]] + ([G.line(1.0, cell=(0, 3, 0))[0]] if with_line else [])))
    return m


def run(m, src, **kw):
    src = np.array(src, np.float32)
    return m.register(src, np.tile(I6, (len(src), 1)), np.eye(4), trace=4, **kw)


def test_patch_centroids_are_exact():
    d = pairs_map().read()
    assert [tuple(c) for c in d["centroid"]] == [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5)] and list(d["flag"]) == [1, 1]
    assert tuple(d["normal"][0]) == (1.0, 0.0, 0.0) and tuple(d["normal"][1]) == (0.0, 0.0, 1.0)


GATE_SRC = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 0.5, 0.75), (2.0, 0.5, 0.5)]     # the last: 0.5 from b's centroid, a's is 1.5 away


def test_the_gate_is_strict():
    r = run(pairs_map(), GATE_SRC, gate=0.5, max_iterations=1)
    assert r["pairs_trace"][0] == 3           # d^2 = 0.25 = gate^2: dropped
    assert run(pairs_map(), GATE_SRC, gate=float(np.nextafter(0.5, 1)), max_iterations=1)["pairs_trace"][0] == 4


def test_mutation_closed_gate_is_caught():
    assert run(pairs_map(VG.MUT_CLOSED_GATE), GATE_SRC, gate=0.5, max_iterations=1)["pairs_trace"][0] == 4


LINE_SRC = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 0.5, 0.75), (0.5, 3.5, 0.5)]     # the last: only the line's voxel is near


def test_only_plane_voxels_are_paired():
    m = pairs_map(with_line=True)
    assert list(m.read()["flag"]) == [1, 1, 0]
    assert run(m, LINE_SRC, max_iterations=1)["pairs_trace"][0] == 3


def test_mutation_pair_all_is_caught():
    assert run(pairs_map(VG.MUT_PAIR_ALL, with_line=True), LINE_SRC, max_iterations=1)["pairs_trace"][0] == 4


TIE_SRC = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (1.0, 0.5, 0.5)]      # the last: 0.5 from either centroid, an exact tie in f32
# the first iteration's cost from identity: the two points on centroids add nothing; the third has r = (-+0.5, 0, 0), and
# with Cp = I the pair's M is (C'q + I)^-1: 1 / (1 + eps) along a's normal x, 1 / 2 along x in b's plane
TIE_COST_LOWEST = 0.25 / (1.0 + G.EPS) / 3.0
TIE_COST_HIGHEST = 0.25 / 2.0 / 3.0


def test_an_exact_tie_goes_to_the_lowest_key():
    r = run(pairs_map(), TIE_SRC, max_iterations=1)
    assert r["pairs_trace"][0] == 3 and r["cost"] == pytest.approx(TIE_COST_LOWEST, rel=1e-12)


def test_mutation_no_tie_rule_is_caught():
    r = run(pairs_map(VG.MUT_NO_TIE_RULE), TIE_SRC, max_iterations=1)
    assert r["cost"] == pytest.approx(TIE_COST_HIGHEST, rel=1e-12) and abs(r["cost"] - TIE_COST_LOWEST) > 0.01


def test_fewer_than_three_pairs_and_no_plane_voxel():
    r = run(pairs_map(), TIE_SRC[:2])
    assert (r["state"], r["converged"], r["iterations"], r["pairs"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 2)
    assert np.array_equal(r["transform"], np.eye(4, dtype=np.float32))
    m = VG.OracleDistMap(1.0)
    m.integrate(G.line(1.0)[0])
    r = run(m, [(6.5, 0.5, 0.5)] * 5)
    assert (r["state"], r["pairs"], r["fitness_pairs"], r["fitness"]) == (api.KF_NO_CORRESPONDENCES, 0, 0, 0.0)


# ------------------------------------------------------------------ the registration
def test_registration_recovers_an_exact_copy():
    """Cloud 0 of the builder's sequence is the map (leaf 1.0) and, filtered at 0.30 with the store's covariances, the source,
    started 0.3 m and 0.05 rad off.  The truth is the identity.  Bound: the prototype's error against the truth for a map
    of one cloud at leaf 1.0 (1.46 mm, 0.201 mrad), which had a sensor 0.75 m away on top; a copy has no such change."""
    cloud = V.builder_clouds([0])[0][0]
    m = VG.OracleDistMap(1.0)
    m.integrate(cloud)
    import kf_edge_oracle as KE
    src = KG.OracleCloud(V.cpu_filter(0.30)(cloud), KE.default_params(leaf_size=0.30, gate=2.0), KG.default_gicp())
    c, s = np.cos(0.05), np.sin(0.05)
    init = np.array([[c, -s, 0, 0.25], [s, c, 0, -0.15], [0, 0, 1, 0.05], [0, 0, 0, 1.0]])
    r = m.register(src.xyz, src.cov, init)
    dp, da = V.pose_error(r["transform64"], np.eye(4))
    print("exact copy: %d iterations, state %d, pairs %s of %d, %.4f mm %.5f mrad from the identity, fitness %.3g" %
          (r["iterations"], r["state"], r["pairs_trace"][:r["iterations"]], len(src.xyz), dp * 1e3, da * 1e3, r["fitness"]))
    assert r["converged"] and r["state"] == api.KF_TRANSFORM and r["pairs"] >= len(src.xyz) // 2
    assert dp <= 1.46e-3 and da <= 0.201e-3


# ------------------------------------------------------------------ the library without a device
def test_struct_mirrors():
    assert VG.layout() == VG.mirror_layout()
    for f, want in (("min_points", 6), ("flat_ratio", 4.0), ("line_ratio", 0.01), ("epsilon", 1e-3), ("max_miss_num", 0), ("max_miss_den", 0)):
        assert getattr(api.vmap_default_dist_params(), f) == getattr(VG.default_dist(), f) == want
    for f, want in (("gate", 2.0), ("max_iterations", 100), ("transformation_epsilon", 1e-6), ("rotation_epsilon", 2e-3)):
        assert getattr(api.vmap_default_gicp_params(), f) == getattr(VG.default_gicp(), f) == want


def test_entry_points_without_a_device_and_argument_errors():
    """Well-formed arguments: SLAM_E_NO_DEVICE on a machine without a device (no handle can exist there); with a device a NULL
    map is SLAM_E_INVALID.  Broken arguments are SLAM_E_INVALID on both, before the device is asked for."""
    L = api.lib()
    want = api.E_NO_DEVICE if api.device_count() == 0 else api.E_INVALID
    n, out = C.c_int(-5), np.zeros(64, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    req, res = (api.VmapGicpReq * 1)(), (api.VmapGicpResult * 1)()
    tr = np.zeros(8, np.int32)
    assert L.slam_vmap_enable_distributions(None, None) == want
    assert L.slam_vmap_compute_distributions(None, None) == want
    assert L.slam_vmap_read_moments(None, p(out), p(out), p(out), 4, C.byref(n)) == want
    assert L.slam_vmap_read_distributions(None, None, None, None, None, None, p(out), 4, C.byref(n)) == want
    assert L.slam_vmap_register_gicp(None, None, req, 1, None, res, None) == want
    assert L.slam_vmap_register_gicp_traced(None, None, req, 1, None, res, p(tr), 8, None) == want
    # broken arguments, whatever the machine
    assert L.slam_vmap_enable_distributions(None, C.byref(api.vmap_default_dist_params(epsilon=0.0))) == api.E_INVALID
    assert L.slam_vmap_enable_distributions(None, C.byref(api.vmap_default_dist_params(min_points=0))) == api.E_INVALID
    assert L.slam_vmap_read_moments(None, None, None, None, -1, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_read_moments(None, None, None, None, 0, None) == api.E_INVALID
    assert L.slam_vmap_read_distributions(None, None, None, None, None, None, None, -1, C.byref(n)) == api.E_INVALID
    assert L.slam_vmap_register_gicp(None, None, req, -1, None, res, None) == api.E_INVALID
    assert b"slam_vmap_register_gicp" in L.slam_last_error()
    assert L.slam_vmap_register_gicp(None, None, None, 1, None, res, None) == api.E_INVALID
    assert L.slam_vmap_register_gicp(None, None, req, 1, None, None, None) == api.E_INVALID
    for bad in (dict(gate=0.0), dict(gate=-1.0), dict(max_iterations=0)):
        gp = api.vmap_default_gicp_params(**bad)
        assert L.slam_vmap_register_gicp(None, None, req, 1, C.byref(gp), res, None) == api.E_INVALID, bad
    assert L.slam_vmap_register_gicp_traced(None, None, req, 1, None, res, p(tr), 0, None) == api.E_INVALID
