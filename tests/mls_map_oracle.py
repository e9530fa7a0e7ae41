"""ctypes wrapper of tests/cpp/mls_map_oracle.cpp, the scalar restatement of the height-cluster MLS
(mls.cpp:18-53, 152-402, 481-556) that slam_mls_* is held against.  Compiled on first use by
tests/oracle_build.py."""
import ctypes as C
import os

import numpy as np

from oracle_build import load, ptr as _p
from slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mls_map_oracle.cpp")
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = load("mls_map_oracle", SRC)
    vp = C.c_void_p
    L.mlso_create.restype = vp
    L.mlso_create.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(api.MlsParams)]
    L.mlso_destroy.argtypes = [vp]
    L.mlso_set_params.argtypes = [vp, C.POINTER(api.MlsParams)]
    L.mlso_clear.argtypes = [vp]
    L.mlso_set_pose.argtypes = [vp, C.c_double, C.c_double]
    L.mlso_add_cloud.restype = C.c_double
    L.mlso_add_cloud.argtypes = [vp, vp, C.c_int, C.c_int]
    L.mlso_offset_z.argtypes = [vp, C.c_double]
    L.mlso_read_drivability.argtypes = [vp, vp]
    L.mlso_segmented.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), vp, C.c_int, C.POINTER(C.c_int)]
    L.mlso_read_cells.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.mlso_touched.restype = C.c_int
    L.mlso_touched.argtypes = [vp, vp, C.c_int]
    L.mlso_update_dist.restype = C.c_int
    L.mlso_update_dist.argtypes = [vp]
    L.mlso_updates.restype = C.c_long
    L.mlso_updates.argtypes = [vp]
    L.mlso_outside_updates.restype = C.c_long
    L.mlso_outside_updates.argtypes = [vp]
    _lib = L
    return L


class OracleMls:
    """The same calls as api.MlsMap, computed serially on the host."""

    def __init__(self, size_x, size_y, resolution, params):
        self.size_x, self.size_y, self.resolution = int(size_x), int(size_y), float(resolution)
        self.cells = self.size_x * self.size_y
        self.p = api.MlsParams()
        C.pointer(self.p)[0] = params
        self.capacity = params.max_clusters
        self.h = lib().mlso_create(self.size_x, self.size_y, self.resolution, C.byref(self.p))
        if not self.h:
            raise ValueError("the start pad does not fit in a %d x %d grid" % (self.size_x, self.size_y))
        self.p.update_dist = lib().mlso_update_dist(self.h)
        self.last_seconds = 0.0

    def close(self):
        if self.h:
            lib().mlso_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        for k, v in kw.items():
            setattr(self.p, k, v)
        lib().mlso_set_params(self.h, C.byref(self.p))
        self.p.update_dist = lib().mlso_update_dist(self.h)

    def clear(self):
        lib().mlso_clear(self.h)

    def set_pose(self, x, y):
        lib().mlso_set_pose(self.h, float(x), float(y))

    def add_cloud(self, xyz, pose=None):
        if pose is not None:
            self.set_pose(pose[0], pose[1])
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self.last_seconds = lib().mlso_add_cloud(self.h, _p(a), len(a), 3)

    def offset_z(self, dz):
        lib().mlso_offset_z(self.h, float(dz))

    def read_drivability(self):
        out = np.empty(self.cells, np.int8)
        lib().mlso_read_drivability(self.h, _p(out))
        return out

    def segmented_clouds(self):
        no, ng = C.c_int(), C.c_int()
        lib().mlso_segmented(self.h, None, 0, C.byref(no), None, 0, C.byref(ng))
        obs, gnd = np.empty((no.value, 3), np.float32), np.empty((ng.value, 3), np.float32)
        lib().mlso_segmented(self.h, _p(obs), len(obs), C.byref(no), _p(gnd), len(gnd), C.byref(ng))
        return obs, gnd

    def read_cells(self, cells, clusters=True):
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        n = len(cells)
        out = {"n_clusters": np.zeros(n, np.int32), "clusters": np.zeros((n, self.capacity, 5)) if clusters else None,
               "drivable": np.zeros(n, np.int8), "byte": np.zeros(n, np.int8), "updated": np.zeros(n, np.uint8),
               "pending": np.zeros(n, np.int32)}
        if n:
            lib().mlso_read_cells(self.h, _p(cells), n, self.capacity, _p(out["n_clusters"]), _p(out["clusters"]),
                                  _p(out["drivable"]), _p(out["byte"]), _p(out["updated"]), _p(out["pending"]))
        return out

    def touched(self):
        """every cell with clusters, pending points, a raised flag or a drivable state"""
        n = lib().mlso_touched(self.h, None, 0)
        out = np.empty(n, np.int32)
        lib().mlso_touched(self.h, _p(out), n)
        return out

    def updates(self):
        return lib().mlso_updates(self.h)

    def outside_updates(self):
        """updateCell calls on cells outside the window, made by the neighbour recursion"""
        return lib().mlso_outside_updates(self.h)


def keyframe_cloud(k, n_loop=50):
    """synth.make_cloud3d keyframe k in the map frame, transformed as graph_slam.cpp:271-275 does
    (pcl::transformPointCloud with the pose: double arithmetic, stored as float) and its pose (x, y, th)."""
    from slam_amd import synth
    xyz, (x, y, th) = synth.make_cloud3d(k, n_loop=n_loop)
    R, t = keyframe_Rt(x, y, th)
    return transform(xyz, R, t), (x, y, th)


def keyframe_Rt(x, y, th):
    c, s = np.cos(th), np.sin(th)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return R, np.array([x, y, 0.0])


def transform(xyz, R, t):
    """(float)(r0*x + r1*y + r2*z + t) per coordinate, term by term in double (slam_grid_transform_cloud_dev)"""
    p = xyz.astype(np.float64)
    out = np.empty_like(xyz, dtype=np.float32)
    for k in range(3):
        out[:, k] = (((R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1]) + R[k, 2] * p[:, 2]) + t[k]).astype(np.float32)
    return out


def compare(dev, ora, what=""):
    """Bit-exact comparison of the whole map: every cell's cluster count, drivable state, byte, flag and pending count,
    then the clusters of every cell that holds any, and the drivability bytes.  Returns the cells with clusters."""
    every = np.arange(ora.cells, dtype=np.int32)
    a, b = dev.read_cells(every, clusters=False), ora.read_cells(every, clusters=False)
    for k in ("n_clusters", "drivable", "byte", "updated", "pending"):
        bad = np.nonzero(a[k] != b[k])[0]
        assert not len(bad), "%s %s differs at %d cells, first cell %d: device %s oracle %s" % (
            what, k, len(bad), bad[0], a[k][bad[0]], b[k][bad[0]])
    cells = np.nonzero(b["n_clusters"] > 0)[0].astype(np.int32)
    a, b = dev.read_cells(cells), ora.read_cells(cells)
    ca, cb = a["clusters"].view(np.uint64), b["clusters"].view(np.uint64)
    bad = np.nonzero((ca != cb).any(axis=(1, 2)))[0]
    assert not len(bad), "%s clusters differ at %d cells, first cell %d:\n%s\n%s" % (
        what, len(bad), cells[bad[0]], a["clusters"][bad[0]][:a["n_clusters"][bad[0]]],
        b["clusters"][bad[0]][:b["n_clusters"][bad[0]]])
    assert np.array_equal(dev.read_drivability(), ora.read_drivability()), what + " drivability bytes"
    return cells


class Checked:
    """A device map (api.MlsMap) and the restatement side by side: every call goes to both, and every read first
    compares the whole map (compare) and then answers with the device's values."""

    def __init__(self, size_x, size_y, resolution, params):
        self.dev = api.MlsMap(size_x, size_y, resolution, params=params)
        self.ora = OracleMls(size_x, size_y, resolution, self.dev.params)
        self.cells, self.capacity = self.ora.cells, self.ora.capacity
        self.calls = 0

    def _both(self, name, *a, **kw):
        getattr(self.dev, name)(*a, **kw)
        getattr(self.ora, name)(*a, **kw)
        self.calls += 1

    def set_params(self, **kw):
        self._both("set_params", **kw)

    def clear(self):
        self._both("clear")

    def set_pose(self, x, y):
        self._both("set_pose", x, y)

    def add_cloud(self, xyz, pose=None):
        self._both("add_cloud", xyz, pose)

    def offset_z(self, dz):
        self._both("offset_z", dz)

    def check(self, what=""):
        return compare(self.dev, self.ora, what)

    def read_cells(self, cells, clusters=True):
        self.check("read_cells")
        return self.dev.read_cells(cells, clusters)

    def read_drivability(self):
        self.check("read_drivability")
        return self.dev.read_drivability()

    def touched(self):
        self.check("touched")
        return self.ora.touched()

    def segmented_clouds(self):
        (o1, g1), (o2, g2) = self.dev.segmented_clouds(), self.ora.segmented_clouds()
        assert o1.shape == o2.shape and g1.shape == g2.shape, (o1.shape, o2.shape, g1.shape, g2.shape)
        assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
        return o1, g1

    def close(self):
        self.dev.close()
        self.ora.close()
