"""slam_vmap_coarsen without a device (docs/VOXEL_MAP.md section 11.1): the Python restatement tests/vmap_coarsen_cases.py
(a dict of Python ints, written from the contract) against maps that tests/cpp/vmap_oracle.cpp and vmap_gicp_oracle.cpp build
directly at the coarser leaf, bit for bit; hand-worked parents; the refusals; the mutations of the restatement, each caught by a
named test; and the library's entry point as far as it goes without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import vmap_carve_oracle as VC
import vmap_coarsen_cases as CC
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api, build
from test_cabi_cpu import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENT_FIELDS = ("key", "count", "sums", "E", "M")
PLAIN_FIELDS = ("key", "count", "sums")


def direct(leaf, clouds):
    """the records of a map with moments that integrated `clouds` ((points, (R, t)) or bare points) at `leaf`"""
    om = VG.OracleDistMap(leaf)
    for c in clouds:
        pts, (R, t) = c if isinstance(c, tuple) else (c, (None, None))
        assert om.integrate(pts, R, t) == 0
    return om.read()


def direct_plain(leaf, clouds):
    om = V.OracleMap(leaf)
    for pts, (R, t) in clouds:
        assert om.integrate(pts, R, t) == 0
    _, count, key, sums = om.extract()
    return dict(key=key, count=count, sums=sums)


# ------------------------------------------------------------------ the restatement against maps built at the coarser leaf
@pytest.mark.parametrize("fine,coarse", CC.LEAF_PAIRS)
def test_four_clouds_coarsened_equal_the_map_built_at_the_coarser_leaf(fine, coarse):
    got = CC.coarsened(fine, coarse, direct(fine, CC.FOUR_CLOUDS), True)
    want = direct(coarse, CC.FOUR_CLOUDS)
    assert CC.same_records(got, want, MOMENT_FIELDS)
    assert len(want["key"]) > 20 and int(want["count"].max()) > 10           # a guard of the inputs: parents of many children
    # and without the moments: the plain accumulators alone
    assert CC.same_records(CC.coarsened(fine, coarse, direct_plain(fine, CC.FOUR_CLOUDS), False), direct_plain(coarse, CC.FOUR_CLOUDS), PLAIN_FIELDS)


def test_leaf_030_to_060_holds_plain():
    fine, coarse = CC.PLAIN_ONLY
    assert CC.shift_of(fine, coarse) == 1 and not CC.moments_split(fine)
    got = CC.coarsened(fine, coarse, direct_plain(fine, CC.FOUR_CLOUDS), False)
    assert CC.same_records(got, direct_plain(coarse, CC.FOUR_CLOUDS), PLAIN_FIELDS)


def test_hand_worked_parent_with_eight_children():
    pts, cells, parent, E, M = CC.eight_children(1.0)
    fine = direct(1.0, [pts])
    assert sorted(int(k) for k in fine["key"]) == sorted(CC.key_of(*c) for c in cells) and list(fine["count"]) == [1] * 8
    assert fine["E"].tolist() == [[16384, 32768, 49152]] * 8                  # e = (1/4, 1/2, 3/4) of 65 536 in every child
    got = CC.coarsened(1.0, 2.0, fine, True)
    assert [int(k) for k in got["key"]] == [parent] and list(got["count"]) == [8]
    assert got["E"].tolist() == [E] == [[393216, 524288, 655360]]
    assert got["M"].tolist() == [M] and M[0] == 27917287424
    assert CC.same_records(got, direct(2.0, [pts]), MOMENT_FIELDS)


@pytest.mark.parametrize("j", (1, 2, 3))
def test_cells_around_zero_floor(j):
    pts = CC.around_zero(0.25)
    fine = direct(0.25, [pts])
    assert sorted({CC.cells_of(k)[0] for k in fine["key"]}) == list(range(-9, 9))
    got = CC.coarsened(0.25, 0.25 * 2 ** j, fine, True)
    assert CC.same_records(got, direct(0.25 * 2 ** j, [pts]), MOMENT_FIELDS)
    parents = sorted({CC.cells_of(k)[0] for k in got["key"]})
    assert parents == sorted({c >> j for c in range(-9, 9)}) and -1 in parents and all(CC.cells_of(k)[1] == -1 for k in got["key"])


def test_a_point_on_a_parent_corner():
    pts = CC.parent_corner(0.25)
    got = CC.coarsened(0.25, 0.5, direct(0.25, [pts]), True)
    assert CC.same_records(got, direct(0.5, [pts]), MOMENT_FIELDS)
    assert [int(k) for k in got["key"]] == [CC.key_of(1, -1, 0)] and list(got["count"]) == [2]
    alone = CC.coarsened(0.25, 0.5, direct(0.25, [pts[:1]]), True)
    assert not alone["E"].any() and not alone["M"].any()                      # o = 0 and e = 0 on every axis


def test_shift_two_equals_shift_one_twice():
    fine = direct(0.25, CC.FOUR_CLOUDS)
    once = CC.coarsened(0.25, 1.0, fine, True)
    twice = CC.coarsened(0.5, 1.0, CC.coarsened(0.25, 0.5, fine, True), True)
    assert CC.same_records(once, twice, MOMENT_FIELDS)


def test_a_partition_equals_the_whole_in_three_orders():
    parts = [direct(0.25, [c]) for c in CC.FOUR_CLOUDS]
    want = direct(1.0, CC.FOUR_CLOUDS)
    for order in CC.ORDERS:
        got = CC.coarsened(0.25, 1.0, [parts[k] for k in order], True)
        assert CC.same_records(got, want, MOMENT_FIELDS)
    m = CC.CoarseMap(1.0, True)
    for p in parts:
        m.coarsen(0.25, p)
    assert (m.n_voxels, m.n_points) == (len(want["key"]), sum(len(c[0]) for c in CC.FOUR_CLOUDS))


def test_refusals():
    rec = direct(0.25, [CC.parent_corner()])
    for fine, coarse in ((0.25, 0.25), (0.5, 0.25), (0.25, 0.75), (0.25, 128.0), (0.25, float(np.nextafter(0.5, 1.0)))):
        with pytest.raises(ValueError):
            CC.CoarseMap(coarse, True).coarsen(fine, rec)
    assert CC.shift_of(0.25, 64.0) == 8 and CC.shift_of(0.25, 128.0) is None
    with pytest.raises(ValueError):
        CC.CoarseMap(0.5, True).coarsen(0.25, rec, src_moments=False)
    with pytest.raises(ValueError):
        CC.CoarseMap(0.5, False).coarsen(0.25, rec, src_moments=True)
    # leaf 0.7 with moments: L = 734 003 is no multiple of 16 and floor(d / 16) does not split; plain it is legal
    assert CC.shift_of(0.7, 1.4) == 1 and not CC.moments_split(0.7)
    with pytest.raises(ValueError):
        CC.CoarseMap(1.4, True).coarsen(0.7, rec)
    CC.CoarseMap(1.4, False).coarsen(0.7, rec)
    assert CC.moments_split(0.375) and CC.moments_split(2.0 ** -16) and not CC.moments_split(0.30)


def test_leaf_07_moments_really_do_not_split():
    """why the refusal: at leaf 0.7 the re-centred moments of section 11.1 are not the coarser map's"""
    pts = CC.FOUR_CLOUDS[0][0]
    m = CC.CoarseMap(1.4, True)
    m.coarsen(0.7, direct(0.7, [pts]), unchecked=True)
    r, want = m.records(), direct(1.4, [pts])
    assert int(round(0.7 * 2.0 ** 20)) % 16 == 3
    assert CC.same_records(r, want, PLAIN_FIELDS) and not CC.same_records(r, want, ("E", "M"))


# ------------------------------------------------------------------ mutations of the restatement
def test_mutation_truncation_is_caught():
    """test_cells_around_zero_floor's expectation"""
    pts = CC.around_zero(0.25)
    got = CC.coarsened(0.25, 0.5, direct(0.25, [pts]), True, CC.MUT_TRUNCATE)
    assert not CC.same_records(got, direct(0.5, [pts]), PLAIN_FIELDS)


def test_mutation_dropped_cross_term_is_caught():
    """test_hand_worked_parent_with_eight_children's expectation"""
    pts, cells, parent, E, M = CC.eight_children(1.0)
    got = CC.coarsened(1.0, 2.0, direct(1.0, [pts]), True, CC.MUT_NO_CROSS)
    assert got["E"].tolist() == [E] and got["M"].tolist() != [M]


def test_mutation_full_L_is_caught():
    """test_hand_worked_parent_with_eight_children's expectation"""
    pts, cells, parent, E, M = CC.eight_children(1.0)
    got = CC.coarsened(1.0, 2.0, direct(1.0, [pts]), True, CC.MUT_FULL_L)
    assert got["E"].tolist() != [E] and got["M"].tolist() != [M]


def carved_pair(leaf=0.25):
    """one scan with endpoints in two children of one parent, integrated and carved at `leaf` and at 2 leaf"""
    pts = np.array([(4.25 * leaf, 0.5 * leaf, 0.5 * leaf), (5.25 * leaf, 0.5 * leaf, 0.5 * leaf)], np.float32)
    out = []
    for lf in (leaf, 2 * leaf):
        m = VC.CarveOracleMap(lf)
        m.integrate(pts)
        m.carve(pts)
        seen, miss, key = m.read_carve()
        _, count, key2, sums = m.extract()
        out.append(dict(key=key, count=count, sums=sums, seen=seen, miss=miss))
    return out


def test_carve_planes_are_not_derived():
    fine, coarse = carved_pair()
    assert list(fine["seen"]) == [1, 1] and list(coarse["seen"]) == [1] and [int(k) for k in coarse["key"]] == [CC.key_of(2, 0, 0)]
    got = CC.coarsened(0.25, 0.5, fine, False)
    assert CC.same_records(got, coarse, PLAIN_FIELDS) and list(got["seen"]) == [0] and list(got["miss"]) == [0]


def test_mutation_added_carve_planes_is_caught():
    """test_carve_planes_are_not_derived's example: one scan seen in two children is one scan of the parent, not two"""
    fine, coarse = carved_pair()
    got = CC.coarsened(0.25, 0.5, fine, False, CC.MUT_ADD_CARVE)
    assert list(got["seen"]) == [2] and list(coarse["seen"]) == [1]


# ------------------------------------------------------------------ the library, as far as it goes without a device
@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def test_the_symbol_is_declared_exported_and_bound(L):
    assert "slam_vmap_coarsen" in header_functions() and "slam_vmap_coarsen" in api.EXPORTS
    assert hasattr(L, "slam_vmap_coarsen") and L.slam_vmap_coarsen.argtypes is not None and len(L.slam_vmap_coarsen.argtypes) == 3
    assert callable(api.VoxelMap.coarsen)


def test_argument_errors_need_no_device(L):
    word = np.zeros(64, np.uint64)
    p = word.ctypes.data_as(C.c_void_p)
    assert L.slam_vmap_coarsen(p, p, None) == api.E_INVALID                   # dst == src, before anything is looked at
    assert b"slam_vmap_coarsen" in L.slam_last_error()


@pytest.mark.skipif(api.device_count() != 0, reason="a GPU is present")
def test_well_formed_arguments_answer_no_device(L):
    assert L.slam_vmap_coarsen(None, None, None) == api.E_NO_DEVICE
    a, b = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    assert L.slam_vmap_coarsen(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), None) == api.E_NO_DEVICE
