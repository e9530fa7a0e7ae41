"""ctypes wrapper of tests/cpp/pgo_oracle.cpp, the scalar restatement of the pose-graph optimiser's contract (docs/PGO.md)
that slam_pgo_* is held against.  Compiled on first use by tests/oracle_build.py.  The result structure is slam_amd.api's
(the header's); nothing else of the library is used."""
import ctypes as C
import os

import numpy as np

from oracle_build import load, ptr as _p
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pgo_oracle.cpp")
MUT_NONE, MUT_LEFT_UPDATE, MUT_NO_FLIP, MUT_SCALE_NO_EPS, MUT_KEEP_LAMBDA = 0, 1, 2, 3, 4
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("pgo_oracle", SRC)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.pgoo_create.restype = vp
    L.pgoo_create.argtypes = []
    L.pgoo_destroy.argtypes = [vp]
    L.pgoo_destroy.restype = None
    L.pgoo_set_mutation.argtypes = [vp, C.c_int]
    L.pgoo_set_mutation.restype = None
    L.pgoo_set_params.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    L.pgoo_set_params.restype = None
    L.pgoo_add_vertex.argtypes = [vp, vp, C.c_int]
    L.pgoo_set_vertex.argtypes = [vp, C.c_int, vp]
    L.pgoo_add_edge.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.pgoo_read_vertices.argtypes = [vp, vp]
    L.pgoo_read_vertices.restype = None
    L.pgoo_chi2.argtypes = [vp, vp, vp]
    L.pgoo_chi2.restype = C.c_double
    L.pgoo_jacobians.argtypes = [vp, C.c_int, vp, vp]
    L.pgoo_jacobians.restype = None
    L.pgoo_system.argtypes = [vp, vp, vp]
    L.pgoo_system.restype = None
    L.pgoo_rcm.argtypes = [vp, vp, ip]
    L.pgoo_step.argtypes = [vp, C.c_double, C.c_int, vp, vp]
    L.pgoo_step.restype = None
    L.pgoo_optimize.argtypes = [vp, C.c_int, C.c_int, C.POINTER(api.PgoResult), vp]
    L.pgoo_from_mqt.argtypes = [vp, vp]
    L.pgoo_from_mqt.restype = None
    L.pgoo_to_mqt.argtypes = [vp, C.c_int, vp]
    L.pgoo_to_mqt.restype = None
    L.pgoo_oplus.argtypes = [vp, vp, C.c_int, vp]
    L.pgoo_oplus.restype = None
    L.pgoo_compose.argtypes = [vp, vp, vp]
    L.pgoo_compose.restype = None
    _lib = L
    return L


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(n)


def from_mqt(v):
    out = np.zeros(7)
    lib().pgoo_from_mqt(_p(_f(v, 6)), _p(out))
    return out


def to_mqt(pose7, flip=True):
    out = np.zeros(6)
    lib().pgoo_to_mqt(_p(_f(pose7, 7)), int(flip), _p(out))
    return out


def oplus(pose7, delta, left=False):
    out = np.zeros(7)
    lib().pgoo_oplus(_p(_f(pose7, 7)), _p(_f(delta, 6)), int(left), _p(out))
    return out


def compose(a7, b7):
    out = np.zeros(7)
    lib().pgoo_compose(_p(_f(a7, 7)), _p(_f(b7, 7)), _p(out))
    return out


class OracleGraph:
    """The restatement's graph, with the method names of slam_amd.api.PoseGraph."""

    def __init__(self, mutation=MUT_NONE, banded=False, max_trials=10, tau=1e-5, good_lower=1.0 / 3.0, good_upper=2.0 / 3.0):
        self.h = lib().pgoo_create()
        self.banded = banded
        self.nv = self.ne = 0
        lib().pgoo_set_mutation(self.h, mutation)
        lib().pgoo_set_params(self.h, max_trials, tau, good_lower, good_upper)

    def __del__(self):
        if getattr(self, "h", None):
            lib().pgoo_destroy(self.h)
            self.h = None

    def add_vertex(self, id, pose7, fixed=False):
        assert id == self.nv
        if lib().pgoo_add_vertex(self.h, _p(_f(pose7, 7)), int(bool(fixed))) != 0:
            raise ValueError("vertex %d" % id)
        self.nv += 1

    def set_vertex(self, id, pose7):
        if lib().pgoo_set_vertex(self.h, int(id), _p(_f(pose7, 7))) != 0:
            raise ValueError("vertex %d" % id)

    def add_edge(self, from_, to, meas7, info36):
        if lib().pgoo_add_edge(self.h, int(from_), int(to), _p(_f(meas7, 7)), _p(_f(info36, 36))) != 0:
            raise ValueError("edge %d -> %d" % (from_, to))
        self.ne += 1

    def size(self):
        return self.nv, self.ne

    def read_vertices(self):
        out = np.zeros((self.nv, 7))
        lib().pgoo_read_vertices(self.h, _p(out))
        return out

    def chi2(self):
        e, ce = np.zeros((self.ne, 6)), np.zeros(self.ne)
        return lib().pgoo_chi2(self.h, _p(e), _p(ce)), e, ce

    def jacobians(self, edge):
        Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
        lib().pgoo_jacobians(self.h, int(edge), _p(Ji), _p(Jj))
        return Ji, Jj

    def system(self):
        """(H [6 nv, 6 nv], b [nv, 6]) in vertex numbering; rows and columns of fixed vertices are zero"""
        H, b = np.zeros((6 * self.nv, 6 * self.nv)), np.zeros((self.nv, 6))
        lib().pgoo_system(self.h, _p(H), _p(b))
        return H, b

    def rcm(self):
        perm, w = np.zeros(max(self.nv, 1), np.int32), C.c_int()
        n = lib().pgoo_rcm(self.h, _p(perm), C.byref(w))
        return perm[:n].copy(), w.value

    def step(self, lam, banded=None):
        delta, out = np.zeros((self.nv, 6)), np.zeros(4)
        lib().pgoo_step(self.h, float(lam), int(self.banded if banded is None else banded), _p(delta), _p(out))
        return dict(delta=delta, chi2_before=out[0], chi2_after=out[1], scale=out[2], pivot=int(out[3]))

    def optimize(self, iterations=10, banded=None):
        """(api.PgoResult, margins of the traced trials); raises ValueError without a fixed vertex"""
        res, margins = api.PgoResult(), np.zeros(api.PGO_TRACE)
        rc = lib().pgoo_optimize(self.h, int(iterations), int(self.banded if banded is None else banded), C.byref(res), _p(margins))
        if rc != 0:
            raise ValueError("optimize: %d" % rc)
        res.margins = margins[:min(res.n_trials, api.PGO_TRACE)].copy()
        return res


def trace(res):
    """[(lambda, rho, chi2', accepted)] of the traced trials of a PgoResult"""
    return [(t.lambda_, t.rho, t.chi2, t.accepted) for t in res.trace[:min(res.n_trials, api.PGO_TRACE)]]
