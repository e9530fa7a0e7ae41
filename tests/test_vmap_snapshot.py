"""Snapshots and merging of the voxel map without a device (docs/VOXEL_MAP.md section 10): the new entry points are declared,
exported and bound and refuse bad arguments before they ask for a device; slam_vmap_load parses and validates a file on the
host (files written by the Python restatement tests/vmap_snapshot_cases.py); the restatement itself; and the parser alone
(slam_amd/csrc/vmap_file.hpp) as a program of its own under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vmap_cases as K
import vmap_oracle as V
import vmap_snapshot_cases as S
from slam_amd import api, build
from test_cabi_cpu import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("slam_vmap_layout", "slam_vmap_absorb_dev", "slam_vmap_absorb", "slam_vmap_merge", "slam_vmap_save", "slam_vmap_load")


@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def no_gpu():
    return api.device_count() == 0


def test_new_symbols_are_declared_exported_and_bound(L):
    names = header_functions()
    for n in NEW:
        assert n in names and n in api.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None, n
    assert api.E_IO == -10
    txt = open(os.path.join(ROOT, "include", "slam_mi355x.h")).read()
    assert "#define SLAM_E_IO" in txt and "-10" in txt.split("#define SLAM_E_IO")[1].splitlines()[0]
    for f in ("layout", "absorb", "absorb_dev", "merge", "save", "load"):
        assert callable(getattr(api.VoxelMap, f)), f
    assert callable(api.GlobalMapBuilder.save) and callable(api.GlobalMapBuilder.resume)


def test_argument_errors_need_no_device(L):
    one = np.ones(4, np.uint64)
    p = one.ctypes.data_as(C.c_void_p)
    rej = C.c_int64(-7)
    for f, stream in ((L.slam_vmap_absorb_dev, (None,)), (L.slam_vmap_absorb, ())):
        assert f(None, p, p, p, None, None, None, None, -1, C.byref(rej), *stream) == api.E_INVALID          # n < 0
        assert f(None, None, p, p, None, None, None, None, 1, C.byref(rej), *stream) == api.E_INVALID        # no keys
        assert f(None, p, None, p, None, None, None, None, 1, C.byref(rej), *stream) == api.E_INVALID        # no counts
        assert f(None, p, p, None, None, None, None, None, 1, C.byref(rej), *stream) == api.E_INVALID        # no sums
        assert f(None, p, p, p, p, None, None, None, 1, C.byref(rej), *stream) == api.E_INVALID              # seen without miss
        assert f(None, p, p, p, None, None, None, p, 1, C.byref(rej), *stream) == api.E_INVALID              # M without E
        assert b"slam_vmap_absorb" in L.slam_last_error() and rej.value == -7
    h = C.c_void_p()
    assert L.slam_vmap_save(None, None) == api.E_INVALID and L.slam_vmap_save(None, b"") == api.E_INVALID
    assert L.slam_vmap_load(None, C.byref(h)) == api.E_INVALID and L.slam_vmap_load(b"x", None) == api.E_INVALID
    assert h.value is None


@pytest.mark.skipif(not no_gpu(), reason="a GPU is present")
def test_well_formed_arguments_answer_no_device(L, tmp_path):
    one = np.ones(6, np.uint64)
    p = one.ctypes.data_as(C.c_void_p)
    rej = C.c_int64()
    assert L.slam_vmap_layout(None, None, None, None, None) == api.E_NO_DEVICE
    assert L.slam_vmap_absorb_dev(None, p, p, p, None, None, None, None, 1, C.byref(rej), None) == api.E_NO_DEVICE
    assert L.slam_vmap_absorb(None, p, p, p, p, p, p, p, 1, C.byref(rej)) == api.E_NO_DEVICE
    assert L.slam_vmap_absorb(None, None, None, None, None, None, None, None, 0, None) == api.E_NO_DEVICE
    assert L.slam_vmap_merge(None, None, None, None) == api.E_NO_DEVICE
    assert L.slam_vmap_save(None, str(tmp_path / "m.vmap").encode()) == api.E_NO_DEVICE
    assert not (tmp_path / "m.vmap").exists()
    with pytest.raises(api.SlamError) as e:
        api.VoxelMap.load(str(tmp_path / "absent.vmap"))
    assert e.value.code == api.E_IO


def load_code(L, path):
    h = C.c_void_p()
    rc = L.slam_vmap_load(os.fsencode(str(path)), C.byref(h))
    if rc == api.SLAM_OK:           # a machine with a device: the file loaded
        L.slam_vmap_destroy(h)
    return rc


def good_files():
    rec = S.small_records()
    empty = {k: v[:0] for k, v in rec.items()}
    return {"good_both": S.write_file(1.0, rec, carved=True, dist=S.DEFAULT_DIST), "good_plain": S.write_file(0.3, rec),
            "good_carved": S.write_file(0.3, rec, carved=True), "good_moments": S.write_file(8.0, rec, dist=S.DEFAULT_DIST),
            "good_empty": S.write_file(0.25, empty), "good_even": S.write_file(0.3, {k: v[:4] for k, v in rec.items()})}


def test_load_validates_on_the_host(L, tmp_path):
    """a good file gets past the parser (what answers then is the device question), each malformed one is SLAM_E_INVALID, a
    missing one SLAM_E_IO with the system's message"""
    past_the_parser = api.E_NO_DEVICE if no_gpu() else api.SLAM_OK
    for name, b in good_files().items():
        assert S.valid(b), name
        (tmp_path / name).write_bytes(b)
        assert load_code(L, tmp_path / name) == past_the_parser, (name, L.slam_last_error())
    good, bad = S.malformed_files()
    assert S.valid(good) and len(bad) == 16
    for name, b in bad.items():
        assert not S.valid(b), name
        (tmp_path / name).write_bytes(b)
        assert load_code(L, tmp_path / name) == api.E_INVALID, name
        assert b"slam_vmap_load" in L.slam_last_error()
    assert load_code(L, tmp_path / "no_such_file") == api.E_IO
    assert b"No such file" in L.slam_last_error()


# ------------------------------------------------------------------ the restatement itself
def four_cloud_records(which=range(4)):
    """the sums, counts and keys of the four-cloud case, one record set per cloud, by tests/cpp/vmap_oracle.cpp"""
    out = []
    for k in which:
        om = V.OracleMap(K.LEAF)
        c, (R, t) = K.FOUR_CLOUDS[k]
        om.integrate(c, R, t)
        _, count, key, sums = om.extract()
        out.append(dict(key=key, count=count, sums=sums))
    return out


def same_records(a, b):
    return all(a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes() for f in a)


def test_absorb_of_a_partition_equals_the_whole():
    recs = four_cloud_records()
    whole = V.OracleMap(K.LEAF)
    for c, (R, t) in K.FOUR_CLOUDS:
        whole.integrate(c, R, t)
    _, count, key, sums = whole.extract()
    for order in K.ORDERS:
        m = S.RefMap()
        for k in order:
            assert m.absorb(**recs[k]) == 0
        got = m.records()
        assert got["key"].tobytes() == key.tobytes() and got["count"].tobytes() == count.tobytes() and got["sums"].tobytes() == sums.tobytes()
        assert (m.n_voxels, m.n_points) == (whole.n_voxels, whole.n_points)
    # two maps of two clouds each, then one into the other, either way
    a, b = S.RefMap(), S.RefMap()
    a.absorb(**recs[0]), a.absorb(**recs[1]), b.absorb(**recs[2]), b.absorb(**recs[3])
    ra, rb = a.records(), b.records()
    ab, ba = S.RefMap(), S.RefMap()
    for m, first, second in ((ab, ra, rb), (ba, rb, ra)):
        m.absorb(first["key"], first["count"], first["sums"])
        m.absorb(second["key"], second["count"], second["sums"])
    assert same_records(ab.records(), ba.records()) and ab.records()["sums"].tobytes() == sums.tobytes()
    assert len(set(ra["key"]) & set(rb["key"])) > 0          # the halves share voxels: the adds are exercised


def test_repeats_add_and_invalid_records_are_rejected_one_by_one():
    k = S.key_of(2, -3, 4)
    m = S.RefMap(moments=True)
    n = 300
    assert m.absorb([k] * n, [2] * n, [[1, -2, 3]] * n, E3=[[1, 1, -1]] * n, M6=[[1, 2, 3, 4, 5, 6]] * n) == 0
    r = m.records()
    assert (m.n_voxels, m.n_points, int(r["count"][0])) == (1, 600, 600)
    assert r["sums"].tolist() == [[300, -600, 900]] and r["E"].tolist() == [[300, 300, -300]] and r["M"].tolist() == [[300 * v for v in range(1, 7)]]
    bad = {"all ones": (S.ALL_ONES, 1), "bit 63": (k | 1 << 63, 1), "x field": (k | S.FIELD, 1), "y field": (k | S.FIELD << 21, 1),
           "z field": (k | S.FIELD << 42, 1), "zero count": (k, 0)}
    for name, (key, count) in bad.items():
        m = S.RefMap()
        assert m.absorb([k, key, k + 1], [1, count, 1], [[1, 1, 1]] * 3) == 1, name
        assert (m.n_voxels, m.n_points) == (2, 2), name
    assert S.key_valid(S.key_of(2 ** 20 - 2, 0, 0)) and not S.key_valid(S.key_of(2 ** 20 - 1, 0, 0))
    with pytest.raises(ValueError):
        S.RefMap().absorb([k], [1], [[0, 0, 0]], E3=[[0, 0, 0]], M6=[[0] * 6])
    with pytest.raises(ValueError):
        S.RefMap(moments=True).absorb([k], [1], [[0, 0, 0]])
    with pytest.raises(ValueError):
        S.RefMap().absorb([k], [1], [[0, 0, 0]], seen=[1])
    # seen and miss into a map never carved make it carved; records without them add nothing to the planes
    m = S.RefMap()
    m.absorb([k], [1], [[0, 0, 0]], seen=[2], miss=[1])
    m.absorb([k], [1], [[0, 0, 0]])
    r = m.records()
    assert m.carved and (int(r["seen"][0]), int(r["miss"][0]), int(r["count"][0])) == (2, 1, 2)


def test_the_carve_planes_add_and_what_that_sum_is():
    X, Y, joint, a, b = S.carve_example()
    for first, second in ((a, b), (b, a)):
        m = S.RefMap()
        m.absorb(**first), m.absorb(**second)
        r = m.records()
        got = {int(k): (int(s), int(ms)) for k, s, ms in zip(r["key"], r["seen"], r["miss"])}
        assert got == {X: (1, 0), Y: (1, 0)}
        assert got[Y] == joint[Y] and got[X] != joint[X]      # equal where every map held the voxel at its carve, short of it elsewhere


def test_writer_and_reader_round_trip():
    rec = S.small_records()
    for name, b in good_files().items():
        f = S.read_file(b)
        n = f["n"]
        assert len(b) == 96 + S.payload_bytes(n, f["flags"]), name
        assert f["key"].tobytes() == rec["key"][:n].astype("<u8").tobytes() and f["n_points"] == int(rec["count"][:n].sum())
        again = S.write_file(f["leaf"], f, carved=bool(f["flags"] & S.CARVE), dist=f.get("dist"))
        assert again == b, name
    assert len(good_files()["good_empty"]) == 96
    assert S.payload_bytes(5, 3) == 40 + 24 + 120 + 40 + 360


# ------------------------------------------------------------------ the parser alone, under the host sanitizers
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vmap_file_check") / "vmap_file_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                           "-I", os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "vmap_file_check.cpp"), "-o", exe])
    return exe


def verdicts(checker, directory):
    """name -> 'ok' / 'invalid' from one run of the program; a sanitizer report fails the run"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")      # out-of-bounds reads are what a parser risks
    r = subprocess.run([checker, str(directory)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    return {ln.split()[0]: ln.split()[1] for ln in r.stdout.splitlines()}


def test_parser_alone_agrees_with_the_python_reader(checker, tmp_path):
    files = dict(good_files())
    good, bad = S.malformed_files()
    files.update(bad)
    for name, b in files.items():
        (tmp_path / name).write_bytes(b)
    got = verdicts(checker, tmp_path)
    assert got == {name: "ok" if S.valid(b) else "invalid" for name, b in files.items()}
    assert sum(v == "ok" for v in got.values()) == 6 and sum(v == "invalid" for v in got.values()) == 16


def test_parser_alone_on_every_truncation(checker, tmp_path):
    good = good_files()["good_both"]
    assert S.read_file(good)["n"] == 5 and S.read_file(good)["flags"] == 3
    for n in range(len(good) + 1):
        (tmp_path / ("cut_%04d" % n)).write_bytes(good[:n])
    got = verdicts(checker, tmp_path)
    want = {"cut_%04d" % n: "ok" if S.valid(good[:n]) else "invalid" for n in range(len(good) + 1)}
    assert got == want and [k for k, v in got.items() if v == "ok"] == ["cut_%04d" % len(good)]
