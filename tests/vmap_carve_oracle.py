"""ctypes wrapper of tests/cpp/vmap_carve_oracle.cpp, the scalar restatement of the voxel map with free-space carving
(docs/VOXEL_MAP.md sections 1 and 8) that slam_vmap_carve* is held against bit for bit, and the map builder restated over
it.  Compiled on first use by tests/oracle_build.py.  Nothing of the library is used: the structs are checked against the
header's by vco_layout."""
import ctypes as C
import os

import numpy as np

import vmap_oracle as V
from oracle_build import load, ptr as _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vmap_carve_oracle.cpp")
MUT_NONE, MUT_END_CELL, MUT_GE, MUT_NO_PROTECTION, MUT_PER_RAY, MUT_TRUNCATE = 0, 1, 2, 3, 4, 5
COUNTERS = ("n_rays", "n_dropped", "n_skipped", "n_steps", "n_seen", "n_missed")
_lib = None


class CarveParams(C.Structure):
    """the restatement's own mirror of slam_vmap_carve_params (the defaults are the contract's, written out)"""
    _fields_ = [("end_margin", C.c_int), ("tail_num", C.c_int), ("tail_den", C.c_int), ("max_ray_cells", C.c_int)]


class CarveResult(C.Structure):
    _fields_ = [(f, C.c_int64) for f in COUNTERS]


def params(end_margin=1, tail_num=1, tail_den=8, max_ray_cells=512):
    return CarveParams(end_margin, tail_num, tail_den, max_ray_cells)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("vmap_carve_oracle", SRC)
    vp = C.c_void_p
    L.vco_create.restype = vp
    L.vco_create.argtypes = [C.c_double]
    for f in (L.vco_destroy, L.vco_clear):
        f.argtypes, f.restype = [vp], None
    L.vco_set_mutation.argtypes, L.vco_set_mutation.restype = [vp, C.c_int], None
    for f in (L.vco_n_voxels, L.vco_n_points):
        f.argtypes, f.restype = [vp], C.c_longlong
    L.vco_integrate.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.vco_carve.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(CarveParams), C.POINTER(CarveResult)]
    L.vco_ray_cells.argtypes = [vp, vp, C.POINTER(CarveParams), C.c_int, vp, C.c_int]
    L.vco_extract.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int]
    L.vco_layout.argtypes, L.vco_layout.restype = [vp], None
    _lib = L
    return L


def layout():
    """sizeof and offsets of slam_vmap_carve_params (5 numbers) and slam_vmap_carve_result (7) in the header"""
    out = np.zeros(12, np.int32)
    lib().vco_layout(_p(out))
    return [int(v) for v in out[:5]], [int(v) for v in out[5:]]


def ray_cells(c0, c1, p=None, mutation=MUT_NONE):
    """the cells [m, 3] a ray from cell c0 to cell c1 visits, by the iteration; None when the ray is skipped"""
    p = p or params()
    c0, c1 = np.ascontiguousarray(c0, np.int32), np.ascontiguousarray(c1, np.int32)
    n = lib().vco_ray_cells(_p(c0), _p(c1), C.byref(p), mutation, None, 0)
    if n < 0:
        return None
    out = np.zeros(max(n, 1), np.uint64)
    lib().vco_ray_cells(_p(c0), _p(c1), C.byref(p), mutation, _p(out), n)
    return np.stack(V.cells_of(out[:n]), axis=1).reshape(n, 3)


def closed_form_cells(c0, c1, p=None):
    """numpy's restatement of the closed form: step i of axis k is c0_k + s_k floor((2 a_k i + n - 1) / (2 n)), i = 0 .. n - T - 1"""
    p = p or params()
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    a, s = np.abs(c1 - c0), np.sign(c1 - c0)
    n = int(a.max())
    if n > p.max_ray_cells:
        return None
    T = max(p.end_margin, -((-n * p.tail_num) // p.tail_den))
    i = np.arange(max(n - T, 0), dtype=np.int64)[:, None]
    if n == 0:
        return np.zeros((0, 3), np.int64)
    return c0[None, :] + s[None, :] * ((2 * a[None, :] * i + n - 1) // (2 * n))


class CarveOracleMap:
    """vmap_oracle.OracleMap's interface, with carve(), read_carve() and the carved extraction"""

    def __init__(self, leaf=0.30, mutation=MUT_NONE):
        self.leaf = float(leaf)
        self.h = lib().vco_create(self.leaf)
        lib().vco_set_mutation(self.h, mutation)

    def __del__(self):
        if getattr(self, "h", None):
            lib().vco_destroy(self.h)
            self.h = None

    def clear(self):
        lib().vco_clear(self.h)

    @property
    def n_voxels(self):
        return lib().vco_n_voxels(self.h)

    @property
    def n_points(self):
        return lib().vco_n_points(self.h)

    @staticmethod
    def _cloud(xyz, R, t):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        if R is not None:
            R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
            t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        return xyz, R, t

    def integrate(self, xyz, R=None, t=None):
        """the number of points dropped"""
        xyz, R, t = self._cloud(xyz, R, t)
        return lib().vco_integrate(self.h, _p(xyz), len(xyz), xyz.shape[1], _p(R), _p(t))

    def carve(self, xyz, R=None, t=None, origin=None, p=None, **kw):
        """the six counters as a dict; ValueError when the origin has no cell"""
        xyz, R, t = self._cloud(xyz, R, t)
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        p, r = p or params(**kw), CarveResult()
        if lib().vco_carve(self.h, _p(xyz), len(xyz), xyz.shape[1], _p(R), _p(t), _p(o), C.byref(p), C.byref(r)) != 0:
            raise ValueError("the origin has no cell")
        return {f: int(getattr(r, f)) for f in COUNTERS}

    def _extract(self, lo, hi, min_count, max_miss):
        if lo is not None:
            lo, hi = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
        num, den = (0, 0) if max_miss is None else (int(max_miss[0]), int(max_miss[1]))
        n = lib().vco_extract(self.h, _p(lo), _p(hi), int(min_count), num, den, None, None, None, None, None, None, 0)
        xyz4, count = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
        key, sums = np.zeros(n, np.uint64), np.zeros((n, 3), np.int64)
        seen, miss = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n:
            lib().vco_extract(self.h, _p(lo), _p(hi), int(min_count), num, den, _p(xyz4), _p(count), _p(key), _p(sums), _p(seen), _p(miss), n)
        return xyz4, count, key, sums, seen, miss

    def extract(self, lo=None, hi=None, min_count=0, max_miss=None):
        """(xyz4 [n, 4] f32, count [n] u32, key [n] u64, sums [n, 3] i64); max_miss = (num, den): the carved extraction"""
        return self._extract(lo, hi, min_count, max_miss)[:4]

    def read_carve(self):
        """(seen [n] u32, miss [n] u32, key [n] u64) of every voxel"""
        e = self._extract(None, None, 0, None)
        return e[4], e[5], e[2]


class OracleCarveBuilder(V.OracleBuilder):
    """slam_amd.api.GlobalMapBuilder with its `carve` switch, restated on CarveOracleMap: every accepted cloud is carved
    with trans_full right after it is integrated, and the map the next cloud registers against is the carved extraction."""

    def __init__(self, filter=None, leaf=0.30, gate=2.0, carve=True):
        super().__init__(filter, leaf, gate)
        self.vmap = CarveOracleMap(leaf)
        self.carve = bool(carve)
        self.CARVE_NUM, self.CARVE_DEN = 1, 1
        self.carve_params = params()
        self.last_carve = None

    def max_miss(self):
        return (self.CARVE_NUM, self.CARVE_DEN) if self.carve else None

    def map(self):
        return self.vmap.extract(max_miss=self.max_miss())[0]

    def register(self, xyz):
        lo, hi = self.crop_box()
        map_x = self.vmap.extract(lo, hi, max_miss=self.max_miss())[0]
        if len(map_x) == 0:
            return False, None
        tgt = self.KG.OracleCloud(self.filter(map_x[:, :3]), self.kf_params, self.gp)
        src = self.KG.OracleCloud(self.filter(xyz), self.kf_params, self.gp)
        self.last_sizes = (len(tgt.xyz), len(src.xyz))
        r = self.KG.register_gicp(tgt, src, self.trans_full, self.gp, trace=self.gp.max_iterations + 1)
        ok = r["fitness_pairs"] > 0 and bool(r["converged"]) and not r["fitness"] > self.MAX_SCORE
        return ok, r

    def add_cloud(self, xyz, adopt=None):
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        if self.vmap.n_points == 0:
            self.vmap.integrate(xyz)
            if self.carve:
                self.last_carve = self.vmap.carve(xyz, p=self.carve_params)
            return True, None
        ok, r = self.register(xyz)
        take, T = (ok, r["transform"] if r else None) if adopt is None else adopt
        if take:
            self.trans_full = np.array(T, np.float32).reshape(4, 4)
            T64 = self.trans_full.astype(np.float64)
            self.vmap.integrate(xyz, T64[:3, :3], T64[:3, 3])
            if self.carve:
                self.last_carve = self.vmap.carve(xyz, T64[:3, :3], T64[:3, 3], p=self.carve_params)
        return ok, r
