"""ctypes wrapper of tests/cpp/sc_oracle.cpp, the scalar restatement of the scan-context contract (docs/SCAN_CONTEXT.md)
that slam_kf_sc_* is held against.  Compiled on first use by tests/oracle_build.py.  Nothing of the library is used."""
import ctypes as C
import os

import numpy as np

from oracle_build import load, ptr as _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sc_oracle.cpp")
MUT_NONE, MUT_RING_STRICT, MUT_SECTOR_STRICT, MUT_QUADRANT_TURN, MUT_TIE_HIGHEST, MUT_ROLL_DIRECTION, MUT_H_NO_PLUS_ONE = range(7)
MUTATIONS = {"ring_strict": MUT_RING_STRICT, "sector_strict": MUT_SECTOR_STRICT, "quadrant_turn": MUT_QUADRANT_TURN,
             "tie_highest": MUT_TIE_HIGHEST, "roll_direction": MUT_ROLL_DIRECTION, "h_no_plus_one": MUT_H_NO_PLUS_ONE}
FIELDS = ("distance", "shift", "n_query", "n_candidate", "n_both")
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("sc_oracle", SRC)
    vp = C.c_void_p
    L.sco_tables.argtypes = [C.c_int, C.c_int, C.c_double, vp, vp, vp]
    L.sco_tables.restype = None
    L.sco_descriptor.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp, C.c_int, vp]
    L.sco_descriptor.restype = None
    L.sco_match.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.sco_match.restype = None
    _lib = L
    return L


class Params:
    """The fields of slam_kf_sc_params, with the same defaults."""

    def __init__(self, n_rings=20, n_sectors=64, max_range=80.0, z_min=-2.0, z_step=0.02):
        self.n_rings, self.n_sectors, self.max_range, self.z_min, self.z_step = n_rings, n_sectors, max_range, z_min, z_step

    def dict(self):
        return dict(n_rings=self.n_rings, n_sectors=self.n_sectors, max_range=self.max_range, z_min=self.z_min, z_step=self.z_step)


def tables(p):
    """(edge2, cos, sin) from the restatement's own libm"""
    e, c, s = np.zeros(p.n_rings), np.zeros(p.n_sectors // 4), np.zeros(p.n_sectors // 4)
    lib().sco_tables(p.n_rings, p.n_sectors, p.max_range, _p(e), _p(c), _p(s))
    return e, c, s


def descriptor(xyz, p, tabs=None, mutation=MUT_NONE):
    """[n_rings, n_sectors] u8 of an [n, >= 3] f32 cloud; tabs: the tables to bin by (the library's), default tables(p)"""
    a = np.ascontiguousarray(xyz, dtype=np.float32)
    a = a.reshape(-1, a.shape[1] if a.ndim == 2 else 3)
    e, c, s = [np.ascontiguousarray(t, dtype=np.float64) for t in (tabs or tables(p))]
    assert len(e) == p.n_rings and len(c) == len(s) == p.n_sectors // 4
    out = np.zeros((p.n_rings, p.n_sectors), np.uint8)
    lib().sco_descriptor(_p(a), len(a), a.shape[1], p.n_rings, p.n_sectors, p.z_min, p.z_step, _p(e), _p(c), _p(s), mutation, _p(out))
    return out


def match(a, b, mutation=MUT_NONE):
    """(distance, shift, n_query, n_candidate, n_both) of query a against candidate b"""
    a, b = np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(b, dtype=np.uint8)
    assert a.shape == b.shape and a.ndim == 2
    out = np.zeros(5, np.int32)
    lib().sco_match(_p(a), _p(b), a.shape[0], a.shape[1], mutation, _p(out))
    return tuple(int(v) for v in out)
