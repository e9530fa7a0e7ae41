"""ctypes wrapper of tests/cpp/vmap_oracle.cpp, the scalar restatement of the voxel map's contract (docs/VOXEL_MAP.md
section 1) that slam_vmap_* is held against bit for bit.  Compiled on first use by tests/oracle_build.py.  Nothing of the
library is used: the parameter struct is checked against the header's by vmo_params_layout."""
import ctypes as C
import os

import numpy as np

from oracle_build import load, ptr as _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "vmap_oracle.cpp")
MUT_NONE, MUT_TRUNCATE, MUT_OPEN_BOX, MUT_ARRIVAL_ORDER = 0, 1, 2, 3
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("vmap_oracle", SRC)
    vp = C.c_void_p
    L.vmo_create.restype = vp
    L.vmo_create.argtypes = [C.c_double]
    for f in (L.vmo_destroy, L.vmo_clear):
        f.argtypes, f.restype = [vp], None
    L.vmo_set_mutation.argtypes, L.vmo_set_mutation.restype = [vp, C.c_int], None
    for f in (L.vmo_n_voxels, L.vmo_n_points):
        f.argtypes, f.restype = [vp], C.c_longlong
    L.vmo_integrate.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.vmo_extract.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int]
    L.vmo_params_layout.argtypes, L.vmo_params_layout.restype = [vp], None
    _lib = L
    return L


def params_layout():
    """(sizeof, offsetof leaf, offsetof initial_capacity) of the header's slam_vmap_params"""
    out = np.zeros(3, np.int32)
    lib().vmo_params_layout(_p(out))
    return tuple(int(v) for v in out)


class OracleMap:
    def __init__(self, leaf=0.30, mutation=MUT_NONE):
        self.leaf = float(leaf)
        self.h = lib().vmo_create(self.leaf)
        lib().vmo_set_mutation(self.h, mutation)

    def __del__(self):
        if getattr(self, "h", None):
            lib().vmo_destroy(self.h)
            self.h = None

    def clear(self):
        lib().vmo_clear(self.h)

    @property
    def n_voxels(self):
        return lib().vmo_n_voxels(self.h)

    @property
    def n_points(self):
        return lib().vmo_n_points(self.h)

    def integrate(self, xyz, R=None, t=None):
        """the number of points dropped"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        if R is not None:
            R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
            t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        return lib().vmo_integrate(self.h, _p(xyz), len(xyz), xyz.shape[1], _p(R), _p(t))

    def extract(self, lo=None, hi=None, min_count=0):
        """(xyz4 [n, 4] f32, count [n] u32, key [n] u64, sums [n, 3] i64)"""
        if lo is not None:
            lo, hi = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
        n = lib().vmo_extract(self.h, _p(lo), _p(hi), int(min_count), None, None, None, None, 0)
        xyz4, count = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
        key, sums = np.zeros(n, np.uint64), np.zeros((n, 3), np.int64)
        if n:
            lib().vmo_extract(self.h, _p(lo), _p(hi), int(min_count), _p(xyz4), _p(count), _p(key), _p(sums), n)
        return xyz4, count, key, sums


def key_of(ix, iy, iz):
    return ((int(iz) + (1 << 20)) << 42) | ((int(iy) + (1 << 20)) << 21) | (int(ix) + (1 << 20))


def cells_of(key):
    """(ix, iy, iz) arrays of an array of keys"""
    key = np.asarray(key, dtype=np.uint64)
    m = np.uint64((1 << 21) - 1)
    return tuple(((key >> np.uint64(s)) & m).astype(np.int64) - (1 << 20) for s in (0, 21, 42))


# ------------------------------------------------------------------ the builder loop (docs/VOXEL_MAP.md section 5)
def cpu_filter(leaf):
    """oracle_lib.voxel_downsample as the store's filter: [n, >= 3] f32 -> [m, 3] f32"""
    import oracle_lib

    def f(xyz):
        out, n = oracle_lib.voxel_downsample(np.ascontiguousarray(xyz, np.float32), leaf=(leaf, leaf, leaf))
        return np.ascontiguousarray(out[:max(n, 0), :3])
    return f


class OracleBuilder:
    """slam_amd.api.GlobalMapBuilder restated on OracleMap and tests/kf_gicp_oracle.py.  `filter` stands for the store's
    voxel filter (cpu_filter without a device; the device's own filter where the device is held against this)."""

    def __init__(self, filter=None, leaf=0.30, gate=2.0):
        import kf_edge_oracle as KE
        import kf_gicp_oracle as KG
        self.KG = KG
        self.LEAF_SIZE, self.CROP_DIST, self.MAX_SCORE = float(leaf), 100.0, 1.0
        self.kf_params = KE.default_params(leaf_size=leaf, gate=gate, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
        self.gp = KG.default_gicp(max_iterations=100, transformation_epsilon=1e-6)
        self.filter = filter or cpu_filter(leaf)
        self.vmap = OracleMap(leaf)
        self.trans_full = np.eye(4, dtype=np.float32)
        self.last_sizes = (0, 0)

    def crop_box(self):
        c = [float(self.trans_full[0, 3]), float(self.trans_full[1, 3])]
        return (np.array([-self.CROP_DIST + c[0], -self.CROP_DIST + c[1]], np.float32),
                np.array([self.CROP_DIST + c[0], self.CROP_DIST + c[1]], np.float32))

    def register(self, xyz):
        """the request of one later cloud at the present state, nothing changed: (accepted, result or None)"""
        lo, hi = self.crop_box()
        map_x = self.vmap.extract(lo, hi)[0]
        if len(map_x) == 0:
            return False, None
        tgt = self.KG.OracleCloud(self.filter(map_x[:, :3]), self.kf_params, self.gp)
        src = self.KG.OracleCloud(self.filter(xyz), self.kf_params, self.gp)
        self.last_sizes = (len(tgt.xyz), len(src.xyz))
        r = self.KG.register_gicp(tgt, src, self.trans_full, self.gp, trace=self.gp.max_iterations + 1)
        ok = r["fitness_pairs"] > 0 and bool(r["converged"]) and not r["fitness"] > self.MAX_SCORE
        return ok, r

    def add_cloud(self, xyz, adopt=None):
        """adopt: (accepted, f32 4 x 4) of another builder (the device's), taken over after this one's own request so that
        both face the same map at the next cloud"""
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        if self.vmap.n_points == 0:
            self.vmap.integrate(xyz)
            return True, None
        ok, r = self.register(xyz)
        take, T = (ok, r["transform"] if r else None) if adopt is None else adopt
        if take:
            self.trans_full = np.array(T, np.float32).reshape(4, 4)
            T64 = self.trans_full.astype(np.float64)
            self.vmap.integrate(xyz, T64[:3, :3], T64[:3, 3])
        return ok, r


def builder_clouds(ks=range(6)):
    """the sequence of docs/VOXEL_MAP.md section 7: (cloud [8192, 3] f32, pose) of make_cloud3d(k, n_loop=50, rings=16, n_az=512)"""
    from slam_amd import synth
    return [synth.make_cloud3d(k, n_loop=50, rings=16, n_az=512) for k in ks]


def truth_in_first_frame(pose0, pose):
    """4 x 4 f64 of the planar pose `pose` seen from `pose0` (the first cloud's frame is the map's)"""
    def mat(p):
        c, s = np.cos(p[2]), np.sin(p[2])
        return np.array([[c, -s, 0, p[0]], [s, c, 0, p[1]], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return np.linalg.inv(mat(pose0)) @ mat(pose)


def pose_error(T, truth):
    """(metres in 3-D, radians of yaw) between two 4 x 4 transforms: the planar measure of tests/kf_gicp_cases.py's
    pose_error, which the truth (a planar pose) supports; the tilt a registration adds on top shows in the metres"""
    d = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(T, np.float64)
    return float(np.linalg.norm(d[:3, 3])), float(abs(np.arctan2(d[1, 0], d[0, 0])))
