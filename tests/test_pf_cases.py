"""CPU checks of the particle filter (docs/PARTICLE_FILTER.md): the numpy restatement of tests/pf_cases.py against the published
Philox vectors and against itself (two forms of the resampling rule, the rule's properties), the three host-made tables through the
C-ABI, every refusal that must not need a device, pf_tables.hpp alone under the host sanitizers, and the accuracy condition -- the
filter against dead reckoning of a biased odometry over twenty scans of the synthetic loop -- on the restatement alone."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import pf_cases as F
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["slam_pf_default_params", "slam_pf_angle_table", "slam_pf_gauss_table", "slam_pf_weight_table", "slam_pf_create", "slam_pf_destroy",
       "slam_pf_set_tables", "slam_pf_set_particles", "slam_pf_read_particles", "slam_pf_read_weights", "slam_pf_read_state",
       "slam_pf_random_words_dev", "slam_pf_predict_dev", "slam_pf_predict", "slam_pf_init_gaussian", "slam_pf_update_dev", "slam_pf_update",
       "slam_pf_resample_indices_dev"]


@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    for counter, key, out in F.PHILOX_VECTORS:
        assert F.philox(np.array(counter), key).tolist() == list(out)
    many = F.philox(np.array([v[0] for v in F.PHILOX_VECTORS[:1]] * 3), (0, 0))          # vectorised over counters
    assert many.shape == (3, 4) and (many == many[0]).all()
    w = F.words(0x299f31d0a4093822, [0x243f6a88], 0x85a308d3, 0x13198a2e)                # the key's halves, the counter's order
    assert w[0].tolist() == list(F.philox(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, 0]), (0xa4093822, 0x299f31d0)))


# ------------------------------------------------------------------------------------------------------------ resampling
def sample_of(n):
    if n <= 300:
        return None
    return np.unique(np.concatenate([np.arange(3), np.arange(n - 3, n), np.random.RandomState(n).randint(0, n, 24)]))


@pytest.mark.parametrize("name", sorted(F.resample_cases()))
def test_the_two_resampling_forms_agree(name):
    """the search in the prefix sums against the rule read off its definition: every output of the cases up to 300 weights, both
    ends and a random sample of the larger ones"""
    w = F.resample_cases()[name]
    js = sample_of(len(w))
    for r in F.offsets_of(w):
        a = F.resample_search(w, r)
        assert np.array_equal(a if js is None else a[js], F.resample_direct(w, r, js)), (name, r)


@pytest.mark.parametrize("name", sorted(F.resample_cases()))
def test_properties_of_the_resampling_rule(name):
    w = F.clamp_weights(F.resample_cases()[name])
    n, W = len(w), int(w.sum())
    for r in F.offsets_of(w):
        src = F.resample_search(w, r)
        assert (np.diff(src) >= 0).all() and src.min() >= 0 and src.max() < n
        if W == 0:
            assert np.array_equal(src, np.arange(n))
            continue
        count = np.bincount(src, minlength=n)
        assert (w[count > 0] > 0).all()                                                   # no particle without weight survives
        lo, hi = (n * w) // W, -((-n * w) // W)                                           # floor and ceiling of n w_i / W
        assert (count >= lo).all() and (count <= hi).all(), name                          # within 1 of n w_i / W
        if name.startswith("equal") or name.startswith("full"):
            assert np.array_equal(src, np.arange(n))                                      # equal weights: the identity
        if name.startswith("one_"):
            assert (src == int(np.flatnonzero(w)[0])).all()                               # one weight: n copies of it


def test_offsets_wrap_at_the_sum():
    w = F.resample_cases()["random_257"]
    W = int(w.sum())
    assert np.array_equal(F.resample_search(w, W), F.resample_search(w, 0)) and np.array_equal(F.resample_search(w, W + 1), F.resample_search(w, 1))
    assert not np.array_equal(F.resample_search(w, W - 1), F.resample_search(w, 0))


# ------------------------------------------------------------------------------------------------------------ the tables
def test_the_entry_points_are_declared_and_exported(L):
    for n in NEW:
        assert n in api.EXPORTS and hasattr(L, n), n
    assert sorted(n for n in api.EXPORTS if n.startswith("slam_pf_")) == sorted(NEW)
    for m in ("tables", "set_tables", "set_particles", "particles", "weights", "state", "random_words", "init_gaussian", "predict",
              "predict_dev", "update", "update_dev", "resample_indices"):
        assert callable(getattr(api.ParticleFilter, m)), m
    assert callable(api.GridMatcher.particle_filter) and issubclass(api.ParticleFilter, api._Handle)
    p = api.pf_default_params()
    assert (p.n_particles, p.n_angles, p.gauss_bits, p.weight_len, p.weight_shift, p.resample_num, p.resample_den, p.weight_scale, p.seed) == \
        tuple(F.DEFAULTS[k] for k in ("n_particles", "n_angles", "gauss_bits", "weight_len", "weight_shift", "resample_num", "resample_den",
                                      "weight_scale", "seed"))
    assert [f for f, _ in api.PfState._fields_] == ["t", "n", "resampled", "degenerate", "best", "refused", "n_resamples", "A_max", "W", "S2",
                                                    "MX", "MY", "MC", "MS", "x", "y", "theta"]
    assert C.sizeof(api.PfState) == 136
    assert C.sizeof(api.PfMotion) == 48 and api.PfMotion.dk.offset == 40
    assert api.PF_MOTION_DTYPE.itemsize == 48 and api.PF_MOTION_DTYPE.fields["dk"][1] == 40
    assert api.PF_MOTION_DTYPE.names == ("dx", "dy", "sx", "sy", "sk", "dk")


@pytest.mark.parametrize("A", (64, 4096, 65536))
def test_angle_table(L, A):
    cs = api.pf_angle_table(A).reshape(A, 2)
    q = A // 4
    assert cs[0].tolist() == [1.0, 0.0] and cs[q].tolist() == [0.0, 1.0] and cs[2 * q].tolist() == [-1.0, 0.0] and cs[3 * q].tolist() == [0.0, -1.0]
    th = 2.0 * np.pi * np.arange(A) / A
    assert np.abs(cs[:, 0] - np.cos(th)).max() < 4e-16 and np.abs(cs[:, 1] - np.sin(th)).max() < 4e-16


@pytest.mark.parametrize("b", (4, 12, 16))
def test_gauss_table(L, b):
    G = api.pf_gauss_table(b)
    N = 1 << b
    assert len(G) == N and np.array_equal(G, -G[::-1]) and (np.diff(G) > 0).all()         # antisymmetric exactly, rising
    p = (np.arange(N) + 0.5) / N
    phi = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in G])
    err = float(np.abs(phi - p).max())
    print("b = %d: max |Phi(G[i]) - (i + 1/2) / 2^b| = %.3g" % (b, err))
    assert err <= 1e-12
    assert abs(G.std() - 1.0) < (0.15 if b == 4 else 0.01)                                # a unit Gaussian, up to the tails the table cuts


def test_weight_table(L):
    for scale, shift, n in ((1024.0, 4, 1024), (1.0, 0, 2), (1e300, 14, 65536), (5e-324, 0, 7), (37.5, 3, 999)):
        w = api.pf_weight_table(scale, shift, n)
        assert w[0] == 65536 and w.max() == 65536 and (np.diff(w.astype(np.int64)) <= 0).all()
        with np.errstate(all="ignore"):
            want = np.rint(65536.0 * np.exp(-(np.arange(n, dtype=np.int64) << shift).astype(np.float64) / scale))
        assert np.abs(w.astype(np.int64) - want.astype(np.int64)).max() <= 1              # (numpy's exp may differ in the last place)
    w = api.pf_weight_table(1024.0, 4, 1024)
    assert w[1] == int(np.rint(65536.0 * math.exp(-16.0 / 1024.0))) and w[-1] == 0


def refused(L, f, word, *args):
    rc = f(*args)
    msg = L.slam_last_error().decode()
    assert rc == api.E_INVALID and word in msg, (args, rc, msg)


def test_the_table_makers_refuse_before_they_write(L):
    buf = np.full(1 << 17, 7.0)
    for A in (0, -64, 32, 63, 65, 96, 1 << 17, 2 ** 31 - 1):
        refused(L, L.slam_pf_angle_table, "slam_pf_angle_table", A, vp(buf), 2 * A if 0 < A < (1 << 16) else 128)
    for n in (127, 129, 0, -1):
        refused(L, L.slam_pf_angle_table, "2 n_angles", 64, vp(buf), n)
    refused(L, L.slam_pf_angle_table, "null", 64, None, 128)
    for b in (3, 17, 0, -1, 32, 64):
        refused(L, L.slam_pf_gauss_table, "gauss_bits", b, vp(buf), 16)
    for n in (15, 17, 0):
        refused(L, L.slam_pf_gauss_table, "2^gauss_bits", 4, vp(buf), n)
    refused(L, L.slam_pf_gauss_table, "null", 4, None, 16)
    w = np.full(70000, 7, np.uint32)
    for scale in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):                  # a quotient that would be NaN or would not decay
        refused(L, L.slam_pf_weight_table, "weight_scale", scale, 4, 16, vp(w))
    for shift in (-1, 15, 32):
        refused(L, L.slam_pf_weight_table, "weight_shift", 1024.0, shift, 16, vp(w))
    for n in (1, 0, -3, 65537):
        refused(L, L.slam_pf_weight_table, "weight_len", 1024.0, 4, n, vp(w))
    refused(L, L.slam_pf_weight_table, "null", 1024.0, 4, 16, None)
    assert (buf == 7.0).all() and (w == 7).all()


# --------------------------------------------------------------------------------------- refusals that must not need a device
BAD_PARAMS = [(dict(n_particles=0), "n_particles"), (dict(n_particles=-1), "n_particles"), (dict(n_particles=(1 << 18) + 1), "n_particles"),
              (dict(n_angles=32), "n_angles"), (dict(n_angles=4095), "n_angles"), (dict(n_angles=1 << 17), "n_angles"), (dict(n_angles=0), "n_angles"),
              (dict(gauss_bits=3), "gauss_bits"), (dict(gauss_bits=17), "gauss_bits"), (dict(weight_len=1), "weight_len"),
              (dict(weight_len=65537), "weight_len"), (dict(weight_shift=-1), "weight_shift"), (dict(weight_shift=15), "weight_shift"),
              (dict(weight_scale=0.0), "weight_scale"), (dict(weight_scale=float("nan")), "weight_scale"),
              (dict(weight_scale=float("inf")), "weight_scale"), (dict(weight_scale=-2.0), "weight_scale"),
              (dict(resample_num=-1), "resample_num"), (dict(resample_num=65536), "resample_num"), (dict(resample_den=0), "resample_num"),
              (dict(resample_den=65536), "resample_num")]


@pytest.mark.parametrize("kw,word", BAD_PARAMS)
def test_create_refuses_before_it_touches_a_device(L, kw, word):
    h = C.c_void_p(5)
    p = api.pf_default_params(**kw)
    refused(L, L.slam_pf_create, word, C.byref(p), C.byref(h))
    assert not h.value                                                                    # the out pointer is nulled, no handle leaks
    refused(L, L.slam_pf_create, "null out", C.byref(p), None)


BAD_MOTIONS = [((0.0, 0.0, float("nan"), 0.0, 0.0, 0), "sigma"), ((0.0, 0.0, 0.0, float("inf"), 0.0, 0), "sigma"),
               ((0.0, 0.0, 0.0, 0.0, float("nan"), 0), "sigma"), ((0.0, 0.0, -0.1, 0.0, 0.0, 0), "negative"),
               ((0.0, 0.0, 0.0, 0.0, -1.0, 0), "negative"), ((0.0, 0.0, 0.0, 0.0, 2.0 ** 20, 0), "sk at or beyond"),
               ((0.0, 0.0, 0.0, 0.0, 1.0, 1 << 20), "dk"), ((0.0, 0.0, 0.0, 0.0, 1.0, -(1 << 20)), "dk"),
               ((float("nan"), 0.0, 0.0, 0.0, 0.0, 0), "increment"), ((0.0, float("-inf"), 0.0, 0.0, 0.0, 0), "increment")]


@pytest.mark.parametrize("m,word", BAD_MOTIONS)
def test_motion_arguments_are_refused_before_a_device_is_touched(L, m, word):
    """slam_pf_predict reads the motion before anything else: a non-null handle that is never dereferenced is enough to show that the
    refusal comes first (no filter can exist on a machine without a device)"""
    assert not F.motion_ok(m)
    fake = (C.c_char * 4096)()                                                            # never read: the motion is checked first
    refused(L, L.slam_pf_predict, word, C.addressof(fake), C.byref(api.PfMotion(*m)))
    ref = F.Filter(np.zeros(128), np.zeros(16), np.array([65536, 0]), n_particles=3, n_angles=64, gauss_bits=4, weight_len=2)
    ref.predict(m)
    assert (ref.t, ref.refused) == (0, 1)                                                 # the restatement counts and skips it


def test_null_handles_are_refused(L):
    one, fake = np.zeros(4), (C.c_char * 4096)()                                          # fake: a handle that is never read
    refused(L, L.slam_pf_create, "null out", None, None)                                  # (null params are the defaults)
    refused(L, L.slam_pf_predict, "slam_pf_predict", None, C.byref(api.PfMotion()))
    refused(L, L.slam_pf_predict, "null motion", C.addressof(fake), None)
    refused(L, L.slam_pf_predict_dev, "slam_pf_predict_dev", None, None, None)
    refused(L, L.slam_pf_update, "slam_pf_update", None, None, vp(one), 2, 0, 0.0, 0.0)
    refused(L, L.slam_pf_update_dev, "slam_pf_update_dev", None, None, vp(one), 2, 0, 0.0, 0.0, None)
    refused(L, L.slam_pf_read_state, "slam_pf_read_state", None, C.byref(api.PfState()))
    refused(L, L.slam_pf_read_state, "slam_pf_read_state", C.addressof(fake), None)
    refused(L, L.slam_pf_set_particles, "slam_pf_set_particles", None, vp(one), vp(one), vp(one), 1)
    refused(L, L.slam_pf_read_particles, "slam_pf_read_particles", None, None, None, None)
    refused(L, L.slam_pf_read_weights, "slam_pf_read_weights", None, None, None)
    refused(L, L.slam_pf_set_tables, "slam_pf_set_tables", None, None, 0, None, 0, None, 0)
    refused(L, L.slam_pf_init_gaussian, "slam_pf_init_gaussian", None, 0.0, 0.0, 0, 0.0, 0.0, 0.0)
    refused(L, L.slam_pf_random_words_dev, "slam_pf_random_words_dev", None, 0, 1, 0, 0, None)
    refused(L, L.slam_pf_resample_indices_dev, "slam_pf_resample_indices_dev", None, None, 1, 0, None, None)
    L.slam_pf_destroy(None)
    L.slam_pf_default_params(None)


@pytest.mark.skipif(api.device_count() != 0, reason="a GPU is present")
def test_create_fails_loudly_without_a_device(L):
    with pytest.raises(api.SlamError) as e:
        api.ParticleFilter(16)
    assert e.value.code == api.E_NO_DEVICE


# --------------------------------------------------------------------------- the table header alone, under the host sanitizers
def test_table_header_alone_under_the_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "slam_amd", "csrc", "pf_tables.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cmath", "cstdint"]        # no HIP, no library
    exe = str(tmp_path / "pf_tables_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pf_tables_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "ok"


# ------------------------------------------------------------------------------------------------- the accuracy condition
@pytest.mark.parametrize("seed", F.LOOP["seeds"])
def test_the_filter_beats_dead_reckoning_over_twenty_scans(L, seed):
    """1 024 particles in the 500 x 500 grid at 0.1 m, started around the true pose; the odometry is the true increment with its dx
    10 % too long and two heading steps too many per scan (LOOP in tests/pf_cases.py).  The estimate is nearer to the truth than dead
    reckoning of that odometry at the last step and at 15 of the 20 steps or more.  No absolute figure is asserted."""
    plane = F.loop_plane()
    half = F.LOOP["size"] // 2
    tab = (-half, -half, plane)
    f = F.Filter(api.pf_angle_table(4096), api.pf_gauss_table(12), api.pf_weight_table(1024.0, 4, 1024), seed=seed)
    errs = F.run_loop(f, (tab, tab))
    wins = sum(a < b for a, b in errs)
    print("seed %d: filter / dead reckoning at the last step %.4f / %.4f m, nearer at %d of 20 steps, worst filter error %.4f m, %d resamples"
          % (seed, errs[-1][0], errs[-1][1], wins, max(e[0] for e in errs), f.n_resamples))
    assert len(errs) == 20 and errs[-1][0] < errs[-1][1] and wins >= 15
