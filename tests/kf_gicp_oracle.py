"""ctypes wrapper of tests/cpp/kf_gicp_oracle.cpp, the scalar restatement of the store's Generalized ICP
(docs/KF_GICP.md) that slam_kf_compute_covariances and slam_kf_register_gicp are held against.  Compiled on first use
by tests/oracle_build.py."""
import ctypes as C
import os

import numpy as np

import kf_edge_oracle as K
from oracle_build import load, ptr as _p
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kf_gicp_oracle.cpp")
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("kf_gicp_oracle", SRC, (K.COMMON,))
    vp = C.c_void_p
    L.kgo_covariances.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, vp, vp]
    L.kgo_plane_covariance.argtypes = [vp, C.c_double, vp]
    L.kgo_plane_covariance.restype = None
    L.kgo_pair.argtypes = [vp] * 7 + [C.POINTER(C.c_double)]
    L.kgo_pair.restype = None
    L.kgo_step.argtypes = [vp] * 4
    L.kgo_index_create.restype = vp
    L.kgo_index_create.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp]
    L.kgo_index_destroy.argtypes = [vp]
    L.kgo_index_destroy.restype = None
    L.kgo_gicp.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_double, C.POINTER(api.KfGicpParams),
                           C.POINTER(api.KfGicpResult), vp, C.c_int, C.POINTER(C.c_double)]
    L.kgo_gicp.restype = None
    L.kgo_fitness.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.POINTER(api.KfGicpResult), C.POINTER(C.c_double)]
    L.kgo_fitness.restype = None
    _lib = L
    return L


def default_gicp(**kw):
    """slam_kf_gicp_default_params' values without the library."""
    p = api.KfGicpParams(20, 0.0, 1e-3, 10, 1e-6, 2e-3, 4)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def cov_radius(kf_params, gp):
    return gp.cov_radius if gp.cov_radius > 0 else 2.0 * K.lattice_edge(kf_params)


def plane_covariance(c6, eps):
    c6 = np.ascontiguousarray(c6, np.float64)
    out = np.zeros(6)
    lib().kgo_plane_covariance(_p(c6), eps, _p(out))
    return out


def sym(c6):
    xx, xy, xz, yy, yz, zz = c6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def pair_terms(T, p, q, Cp, Cq):
    """One pair's (H [6, 6], g [6], cost) at the transform T [3 or 4, 4]."""
    T = np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4])
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    Cp, Cq = np.ascontiguousarray(Cp, np.float64), np.ascontiguousarray(Cq, np.float64)
    h, g, c = np.zeros(21), np.zeros(6), C.c_double()
    lib().kgo_pair(_p(T), _p(p), _p(q), _p(Cp), _p(Cq), _p(h), _p(g), C.byref(c))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = h
    return H + np.triu(H, 1).T, g, c.value


def step(H, g, T):
    """(ok, N [3, 4]): the Gauss-Newton step composed with T."""
    H, g = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(g, np.float64)
    T = np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4])
    N = np.zeros((3, 4))
    ok = lib().kgo_step(_p(H), _p(g), _p(T), _p(N))
    return bool(ok), N


class OracleCloud:
    """A filtered cloud ([n, >= 3] f32) with the restatement's neighbour lists, covariances and search lattice.
    Raises ValueError for a cloud of fewer than k points."""

    def __init__(self, xyz, kf_params=None, gp=None):
        self.params = kf_params or K.default_params()
        self.gp = gp or default_gicp()
        self.xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        n, k = len(self.xyz), self.gp.k_correspondences
        self.cov = np.zeros((n, 6))
        self.index, self.dist2 = np.zeros((n, k), np.int32), np.zeros((n, k), np.float32)
        self.count = np.zeros(n, np.int32)
        rc = lib().kgo_covariances(_p(self.xyz), n, 3, k, cov_radius(self.params, self.gp), self.gp.gicp_epsilon,
                                   self.gp.cov_min_neighbours, _p(self.cov), _p(self.index), _p(self.dist2), _p(self.count))
        self.h = None
        if rc != 0:
            raise ValueError("a cloud of %d points has fewer than k = %d" % (n, k))
        self.h = lib().kgo_index_create(_p(self.xyz), n, 3, K.lattice_edge(self.params), _p(self.cov))
        self._lum = None

    def __del__(self):
        if getattr(self, "h", None):
            lib().kgo_index_destroy(self.h)
            self.h = None

    def lum_keyframe(self):
        if self._lum is None:
            self._lum = K.OracleKeyframe(self.xyz, self.params)
        return self._lum


def register_gicp(target, source, init, gp=None, trace=64, order=None):
    """The restatement of one slam_kf_register_gicp request on two OracleClouds (target = `from`, source = `to`).
    order: a permutation of the source points (the sums then run in that order).  Returns api.kf_gicp_result_dict's
    fields plus 'pairs_trace', 'margin' (the smallest relative margin of a stop test) and 'fitness_sum'."""
    gp = gp or target.gp
    src, cov = source.xyz, source.cov
    if order is not None:
        src, cov = np.ascontiguousarray(src[order]), np.ascontiguousarray(cov[order])
    init = np.ascontiguousarray(np.asarray(init, np.float32).reshape(16))
    res = api.KfGicpResult()
    tr = np.full(max(trace, 1), -1, np.int32)
    margin, fsum = C.c_double(), C.c_double()
    L = lib()
    L.kgo_gicp(target.h, _p(src), len(src), 3, _p(cov), _p(init), target.params.gate, C.byref(gp), C.byref(res), _p(tr), int(trace),
               C.byref(margin))
    L.kgo_fitness(target.h, _p(src), len(src), 3, target.params.gate, C.byref(res), C.byref(fsum))
    K.lib().kfo_lum(target.lum_keyframe().h, _p(src), len(src), 3, target.params.gate, C.byref(res.edge), None, None, None)
    out = api.kf_gicp_result_dict(res)
    out["pairs_trace"], out["margin"], out["fitness_sum"] = tr, margin.value, fsum.value
    return out
