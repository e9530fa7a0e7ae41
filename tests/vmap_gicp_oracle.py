"""ctypes wrapper of tests/cpp/vmap_gicp_oracle.cpp, the scalar restatement of the voxel map's moments, plane
distributions and the Generalized ICP against them (docs/VOXEL_MAP.md section 9).  Compiled on first use by
tests/oracle_build.py.  The restated `direct` builder (slam_amd.api.GlobalMapBuilder(direct=True)) is at the end."""
import ctypes as C
import os

import numpy as np

import kf_edge_oracle as KE
from oracle_build import load, ptr as _p
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vmap_gicp_oracle.cpp")
GICP_SRC = os.path.join(ROOT, "tests", "cpp", "kf_gicp_oracle.cpp")
MUT_NONE, MUT_TRUNCATE_E, MUT_CLOSED_GATE, MUT_PAIR_ALL, MUT_NO_TIE_RULE = 0, 1, 2, 3, 4
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("vmap_gicp_oracle", SRC, (GICP_SRC, KE.COMMON))
    vp = C.c_void_p
    L.vgo_default_dist_params.argtypes, L.vgo_default_dist_params.restype = [C.POINTER(api.VmapDistParams)], None
    L.vgo_default_gicp_params.argtypes, L.vgo_default_gicp_params.restype = [C.POINTER(api.VmapGicpParams)], None
    L.vgo_create.restype = vp
    L.vgo_create.argtypes = [C.c_double]
    L.vgo_enable.argtypes = [vp, C.POINTER(api.VmapDistParams)]
    for f in (L.vgo_destroy, L.vgo_clear):
        f.argtypes, f.restype = [vp], None
    L.vgo_set_mutation.argtypes, L.vgo_set_mutation.restype = [vp, C.c_int], None
    L.vgo_n_voxels.argtypes, L.vgo_n_voxels.restype = [vp], C.c_longlong
    L.vgo_integrate.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.vgo_set_carve.argtypes, L.vgo_set_carve.restype = [vp, vp, vp, vp, C.c_int], None
    L.vgo_read.argtypes = [vp, C.c_int] + [vp] * 10
    L.vgo_register.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(api.VmapGicpParams), C.POINTER(api.VmapGicpResult), vp, C.c_int,
                               C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vgo_register.restype = None
    L.vgo_layout.argtypes, L.vgo_layout.restype = [vp], None
    _lib = L
    return L


def default_dist(**kw):
    """slam_vmap_default_dist_params' values without the library"""
    p = api.VmapDistParams()
    lib().vgo_default_dist_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_gicp(**kw):
    """slam_vmap_default_gicp_params' values without the library"""
    p = api.VmapGicpParams()
    lib().vgo_default_gicp_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def layout():
    """sizeof and offsetof of slam_vmap_dist_params, _gicp_req, _gicp_params and _gicp_result, in the header's order"""
    out = np.zeros(28, np.int32)
    lib().vgo_layout(_p(out))
    return [int(v) for v in out]


def mirror_layout():
    """the same numbers from the ctypes mirrors of slam_amd.api"""
    out = []
    for T in (api.VmapDistParams, api.VmapGicpReq, api.VmapGicpParams, api.VmapGicpResult):
        out.append(C.sizeof(T))
        out += [getattr(T, f).offset for f, _ in T._fields_]
    return out


class OracleDistMap:
    """The restated map with distributions enabled.  Raises ValueError for what slam_vmap_enable_distributions refuses."""

    def __init__(self, leaf=1.0, params=None, mutation=MUT_NONE, **kw):
        self.leaf = float(leaf)
        self.h = lib().vgo_create(self.leaf)
        lib().vgo_set_mutation(self.h, mutation)
        self.enable(params, **kw)

    def enable(self, params=None, **kw):
        p = params or default_dist(**kw)
        if lib().vgo_enable(self.h, C.byref(p)) != 0:
            raise ValueError("refused: the map holds voxels, or leaf %g is more than 8" % self.leaf)
        self.params = p

    def __del__(self):
        if getattr(self, "h", None):
            lib().vgo_destroy(self.h)
            self.h = None

    def clear(self):
        lib().vgo_clear(self.h)

    @property
    def n_voxels(self):
        return lib().vgo_n_voxels(self.h)

    def integrate(self, xyz, R=None, t=None):
        """the number of points dropped"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        if R is not None:
            R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
            t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        return lib().vgo_integrate(self.h, _p(xyz), len(xyz), xyz.shape[1], _p(R), _p(t))

    def set_carve(self, seen, miss, key):
        """seen and miss of the voxels named by key, as VoxelMap.read_carve or OracleCarveMap give them"""
        seen, miss = np.ascontiguousarray(seen, np.uint32), np.ascontiguousarray(miss, np.uint32)
        key = np.ascontiguousarray(key, np.uint64)
        lib().vgo_set_carve(self.h, _p(key), _p(seen), _p(miss), len(key))

    def read(self):
        """every voxel in key order: a dict of key, count, sums, E, M, centroid, normal, cov6, eig, flag"""
        n = lib().vgo_read(self.h, 0, *([None] * 10))
        d = dict(key=np.zeros(n, np.uint64), count=np.zeros(n, np.uint32), sums=np.zeros((n, 3), np.int64), E=np.zeros((n, 3), np.int64),
                 M=np.zeros((n, 6), np.int64), centroid=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3)), cov6=np.zeros((n, 6)),
                 eig=np.zeros((n, 3)), flag=np.zeros(n, np.uint8))
        if n:
            lib().vgo_read(self.h, n, *[_p(d[k]) for k in ("key", "count", "sums", "E", "M", "centroid", "normal", "cov6", "eig", "flag")])
        return d

    def register(self, src_xyz, src_cov, init, params=None, trace=128, **kw):
        """The restatement of one slam_vmap_register_gicp request: api.vmap_gicp_result_dict's fields plus 'pairs_trace',
        'margin' (the smallest relative margin of a stop test) and 'fitness_sum'."""
        src = np.ascontiguousarray(np.asarray(src_xyz, np.float32)[:, :3])
        cov = np.ascontiguousarray(src_cov, np.float64)
        init = np.ascontiguousarray(np.asarray(init, np.float32).reshape(16))
        p = params or default_gicp(**kw)
        res = api.VmapGicpResult()
        tr = np.full(max(trace, 1), -1, np.int32)
        margin, fsum = C.c_double(), C.c_double()
        lib().vgo_register(self.h, _p(src), len(src), 3, _p(cov), _p(init), C.byref(p), C.byref(res), _p(tr), int(trace), C.byref(margin),
                           C.byref(fsum))
        out = api.vmap_gicp_result_dict(res)
        out["pairs_trace"], out["margin"], out["fitness_sum"] = tr, margin.value, fsum.value
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ the direct builder (docs/VOXEL_MAP.md section 9)
class OracleDirectBuilder:
    """slam_amd.api.GlobalMapBuilder(direct=True) restated on tests/vmap_oracle.py's OracleMap (the 0.30 m map),
    OracleDistMap (the 1 m map the registration runs against) and tests/kf_gicp_oracle.py's source covariances.  `filter`
    stands for the store's voxel filter, as in tests/vmap_oracle.py's OracleBuilder."""
    DIST_LEAF = 1.0

    def __init__(self, filter=None, leaf=0.30, gate=2.0):
        import kf_gicp_oracle as KG
        import vmap_oracle as V
        self.KG = KG
        self.LEAF_SIZE, self.MAX_SCORE = float(leaf), 1.0
        self.kf_params = KE.default_params(leaf_size=leaf, gate=gate, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
        self.gp = KG.default_gicp(max_iterations=100, transformation_epsilon=1e-6)
        self.vp = default_gicp(gate=gate, max_iterations=100, transformation_epsilon=1e-6)
        self.filter = filter or V.cpu_filter(leaf)
        self.vmap = V.OracleMap(leaf)
        self.dmap = OracleDistMap(self.DIST_LEAF)
        self.trans_full = np.eye(4, dtype=np.float32)
        self.n_source = 0

    def register(self, xyz):
        """the request of one later cloud at the present state, nothing changed: (accepted, result)"""
        src = self.KG.OracleCloud(self.filter(xyz), self.kf_params, self.gp)
        self.n_source = len(src.xyz)
        r = self.dmap.register(src.xyz, src.cov, self.trans_full, params=self.vp, trace=self.vp.max_iterations + 1)
        ok = r["fitness_pairs"] > 0 and bool(r["converged"]) and not r["fitness"] > self.MAX_SCORE
        return ok, r

    def add_cloud(self, xyz, adopt=None):
        """adopt: (accepted, f32 4 x 4) of another builder (the device's), taken over after this one's own request"""
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        if self.vmap.n_points == 0:
            self.vmap.integrate(xyz)
            self.dmap.integrate(xyz)
            return True, None
        ok, r = self.register(xyz)
        take, T = (ok, r["transform"]) if adopt is None else adopt
        if take:
            self.trans_full = np.array(T, np.float32).reshape(4, 4)
            T64 = self.trans_full.astype(np.float64)
            self.vmap.integrate(xyz, T64[:3, :3], T64[:3, 3])
            self.dmap.integrate(xyz, T64[:3, :3], T64[:3, 3])
        return ok, r
