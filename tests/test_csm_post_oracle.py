"""The posterior's restatement (tests/csm_post_oracle.py, docs/CSM.md section 6) on its own: cases worked by hand, the
property the pruned enumeration rests on, the two scenes, the ctypes mirrors of the new structures and the overflow guard.
No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import csm_cases as K
import csm_oracle as CO
import csm_post_cases as PC
import csm_post_oracle as PO
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WTAB = PO.weight_table(8.0)


def post_of(om, ga, nga, R0, t0, wtab=WTAB, **kw):
    vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
    P = om.params
    return vol, cnt, PO.posterior(vol, cnt, len(ga) + len(nga), wtab, P.resolution, P.theta_step, bounds=om.bounds(ga, nga, R0, t0), **kw)


def test_weight_table_ends():
    assert WTAB[0] == 65536 and WTAB[256] == int(np.rint(65536.0 * np.exp(-8.0))) == 22
    assert np.all(np.diff(WTAB.astype(np.int64)) <= 0)
    assert np.all(PO.weight_table(0.0) == 65536)
    assert PO.weight_table(64.0)[256] == 0


def test_uniform_by_hand():
    # a scan wholly outside the tables: every score is 0, every deficit 0, every weight wtab[0]
    box = K.box_model()
    om = CO.OracleMatcher(box[0], box[1])
    om.set_window(8, 8, 0, 0.01)
    ga, nga, R0, t0 = PC.all_outside_scan()
    for mpp in PC.MARGINS:
        vol, cnt, p = post_of(om, ga, nga, R0, t0, margin_per_point=mpp)
        assert vol.max() == 0 and cnt[0] == 200
        assert (p["valid"], p["n_within"], p["margin"]) == (1, 289, mpp * 200)
        assert p["m0"] == 289 * 65536
        assert p["mean_c"] == [8.0, 8.0, 0.0]                       # the winner is flat index 0, the mean the window's middle
        assert p["cov_c"] == [24.0, 0.0, 0.0, 24.0, 0.0, 0.0]       # (17^2 - 1) / 12
        assert p["mean"] == [8.0 * 0.1, 8.0 * 0.1, 0.0]
        assert p["cov"] == [(24.0 * 0.1) * 0.1, 0.0, 0.0, (24.0 * 0.1) * 0.1, 0.0, 0.0]
        assert p["blocks_evaluated"] == 9
        # the second mode: the lowest flat index outside |o| <= 2 of candidate (0, 0) is a = 3, b = 0
        assert (p["second_score"], p["second_k"], p["second_a"], p["second_b"]) == (0, 0, 3, 0)


def test_the_tie():
    kw, m_ga, m_nga, ga, nga, R0, t0, winner, other, score = K.tie_case()
    om = CO.OracleMatcher(m_ga, m_nga, **kw)
    vol, cnt, p = post_of(om, ga, nga, R0, t0, margin_per_point=0)
    assert (p["n_within"], p["margin"]) == (2, 0)
    assert (p["second_score"], p["second_k"], p["second_a"], p["second_b"]) == (score, *other)
    assert p["m0"] == 2 * 65536
    assert p["mean_c"] == [(other[1] - winner[1]) / 2.0, (other[2] - winner[2]) / 2.0, 0.0]      # halfway between the two
    assert p["cov_c"][0] == 4.5 ** 2 and p["cov_c"][3] == 0.25 and p["cov_c"][1] == -4.5 * 0.5


@pytest.mark.parametrize("win,ht", [((8, 8), 4), ((2, 16), 0), ((0, 8), 4)])
def test_margin_255_is_the_whole_volume(win, ht):
    box = K.box_model()
    om = CO.OracleMatcher(box[0], box[1])
    om.set_window(win[0], win[1], ht, 0.01)
    ga, nga = K.scan_of(box, 65, K.TRUE_POSE, 103)
    R0, t0 = K.pose_Rt(K.TRUE_POSE[0] + 0.2, K.TRUE_POSE[1] - 0.3, K.TRUE_POSE[2] + 0.02)
    vol, cnt, p = post_of(om, ga, nga, R0, t0, margin_per_point=255)
    N = vol.size
    assert p["n_within"] == N and p["blocks_evaluated"] == int(np.prod(om.block_dims))   # 17 = 2 x 8 + 1: a ragged block's phantoms would count
    k, b, a = (int(v) for v in np.unravel_index(int(np.argmax(vol)), vol.shape))
    M = 255 * int(cnt[k])
    w = WTAB[((int(vol.max()) - vol.astype(np.int64)) * 256) // M].astype(object)
    Kk, B, A = np.indices(vol.shape)
    o = [(A - a).astype(object), (B - b).astype(object), (Kk - k).astype(object)]
    assert p["m0"] == int(w.sum())
    assert p["m1"] == [int((w * o[i]).sum()) for i in range(3)]
    assert p["m2"] == [int((w * o[i] * o[j]).sum()) for i, j in PO.PAIRS]


def test_enumeration_by_bounds_covers_the_margin():
    box = K.box_model()
    om = CO.OracleMatcher(box[0], box[1])
    D = om.params.block
    for name, ga, nga, R0, t0, win, ht in K.volume_cases():
        om.set_window(win[0], win[1], ht, 0.01)
        vol, cnt = om.volume(ga, nga, R0, t0, counted=True)
        U = om.bounds(ga, nga, R0, t0)
        for mpp in PC.MARGINS:
            (k, b, a), top, M, d, mask = PO.within(vol, cnt, mpp)
            listed = U.astype(np.int64) >= top - M
            assert listed[k, b // D, a // D], name                   # the top block included
            kk, bb, aa = np.nonzero(mask)
            assert listed[kk, bb // D, aa // D].all(), (name, mpp)   # no candidate within the margin sits in a block left out
            if mpp == 255:
                assert mask.all() and listed.all(), name


def test_room_scene_is_well_determined():
    m_ga, m_nga, ga, nga, R0, t0 = PC.room_scene()
    om = CO.OracleMatcher(m_ga, m_nga)
    om.set_window(*PC.SCENE_WINDOW)
    vol, cnt, p = post_of(om, ga, nga, R0, t0)
    print("room: n_within %d, blocks %d of %d, cov_c diag %.3f %.3f %.3f, second %d" %
          (p["n_within"], p["blocks_evaluated"], int(np.prod(om.block_dims)), p["cov_c"][0], p["cov_c"][3], p["cov_c"][5], p["second_score"]))
    assert max(p["cov_c"][0], p["cov_c"][3], p["cov_c"][5]) < 0.5
    assert p["second_score"] == -1
    assert p["blocks_evaluated"] < int(np.prod(om.block_dims)) // 10


def test_corridor_scene_is_flat_along_x():
    m_ga, m_nga, ga, nga, R0, t0 = PC.corridor_scene()
    om = CO.OracleMatcher(m_ga, m_nga)
    om.set_window(*PC.SCENE_WINDOW)
    vol, cnt, p = post_of(om, ga, nga, R0, t0)
    n_points = int(cnt[np.unravel_index(int(np.argmax(vol)), vol.shape)[0]])
    print("corridor: n_within %d, blocks %d of %d, cov_c xx %.3f yy %.3f tt %.3f, second deficit %d" %
          (p["n_within"], p["blocks_evaluated"], int(np.prod(om.block_dims)), p["cov_c"][0], p["cov_c"][3], p["cov_c"][5],
           int(vol.max()) - p["second_score"]))
    assert p["cov_c"][0] >= 100.0 * p["cov_c"][3]
    assert p["second_score"] >= 0 and int(vol.max()) - p["second_score"] <= n_points


def test_short_scan_is_invalid():
    p = PO.posterior(np.zeros((1, 3, 3), np.int32), np.zeros(1, np.int32), 4, WTAB, 0.1, 0.01)
    assert p["valid"] == 0 and p["second_score"] == -1 and PO.pack(p) == PO.pack(PO.invalid())
    assert len(PO.pack(p)) == C.sizeof(api.CsmPosterior)


# ------------------------------------------------------------------ the ctypes mirrors
def test_csm_post_structs_mirror_the_header(tmp_path):
    structs = {"slam_csm_post_params": api.CsmPostParams, "slam_csm_posterior": api.CsmPosterior}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (f, name, f))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])   # still C
    out = subprocess.check_output([str(exe)], text=True)
    assert len(out.strip().splitlines()) == 2
    for line in out.strip().splitlines():
        parts = line.split()
        cls = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), (parts[0], parts[1], C.sizeof(cls))
        assert len(parts) - 2 == len(cls._fields_)
        for p in parts[2:]:
            f, off = p.split("=")
            assert getattr(cls, f).offset == int(off), (parts[0], f, off, getattr(cls, f).offset)
            if cls is api.CsmPosterior:
                assert api.CSM_POST_DTYPE.fields[f][1] == int(off)
    assert api.CSM_POST_DTYPE.itemsize == C.sizeof(api.CsmPosterior) == 184
    # the packed restatement is laid out the same way: 8 int32, 10 int64, 9 doubles, no padding
    assert api.CsmPosterior.m0.offset == 32 and api.CsmPosterior.mean.offset == 112


def test_post_defaults_are_the_issue_values():
    from slam_amd import build
    build.build()
    p = api.csm_default_post_params()
    assert (p.margin_per_point, p.beta, p.excl_xy, p.excl_theta) == (16, 8.0, 2, 2)
    assert PO.DEFAULTS == dict(margin_per_point=16, beta=8.0, excl_xy=2, excl_theta=2)


def test_overflow_guard_against_python_integers():
    # the defaults: about 2^52
    n = 81 * 81 * 241
    assert PO.guard_ok(81, 81, 241) and 2 ** 51 < 65536 * 240 * 240 * n < 2 ** 53
    # the widest x window with five angles: 65536 * 32766^2 * 163835 is just above 2^63; one angle fewer is below it
    assert not PO.guard_ok(2 * 16383 + 1, 1, 5) and 65536 * 32766 ** 2 * 163835 >= 2 ** 63
    assert PO.guard_ok(2 * 16383 + 1, 1, 3)
    # the worst term of any sum is w o_i o_j <= 65536 Dmax^2, so N of them stay below the guard's product
    assert 65536 * 32766 ** 2 * (32767 * 3) < 2 ** 63
