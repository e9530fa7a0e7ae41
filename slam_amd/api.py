"""ctypes binding of the C-ABI in include/slam_mi355x.h -- plumbing for tests,
bench.py and __graft_entry__.py.  The product is the shared library (HIP
kernels + C++ host code); this file only marshals numpy arrays and device
pointers across that ABI.  There is no CPU path: if the library is missing or
no HIP device is usable, calls raise SlamError.
"""
import ctypes as C
import math
import os

import numpy as np

from . import cdecl

HERE = os.path.dirname(os.path.abspath(__file__))
# SLAM_AMD_MEASURE=1 loads the measurement build (python -m slam_amd.build --measure) for the tools/ scripts
LIB_PATH = os.path.join(HERE, "lib", "libslam_mi355x_measure.so" if os.environ.get("SLAM_AMD_MEASURE") == "1"
                        else "libslam_mi355x.so")
RCCL_LIB_PATH = os.path.join(HERE, "lib", "libslam_mi355x_rccl.so")

# Everything the headers declare comes from them (slam_amd/cdecl.py): the symbol lists, every restype / argtypes, the
# structs and the #defines.  A new entry point is declared in the header and nowhere else; a struct gets a line in
# STRUCTS only if Python needs it by name.
_H = cdecl.Header()
EXPORTS = _H.read("slam_mi355x.h")                  # every symbol include/slam_mi355x.h declares (tests check the .so exports them all)
RCCL_EXPORTS = _H.read("slam_mi355x_rccl.h")        # those of include/slam_mi355x_rccl.h alone
_MEASURE_EXPORTS = _H.read("slam_mi355x_measure.h") if os.environ.get("SLAM_AMD_MEASURE") == "1" else []

_D = _H.defines
SLAM_OK = _D["SLAM_OK"]
E_INVALID, E_NO_DEVICE, E_HIP, E_TOO_FEW_MODEL, E_TOO_FEW_SCENE, E_NOMEM, E_UNSUPPORTED, E_TIMEOUT, E_COMM, E_IO = \
    (_D["SLAM_E_" + n] for n in ("INVALID", "NO_DEVICE", "HIP", "TOO_FEW_MODEL_POINTS", "TOO_FEW_SCENE_POINTS", "NOMEM",
                                 "UNSUPPORTED", "TIMEOUT", "COMM", "IO"))
ICP_P2P, ICP_P2L = _D["SLAM_ICP_P2P"], _D["SLAM_ICP_P2L"]
RAYCAST_TILED, RAYCAST_GLOBAL, RAYCAST_TILED_MERGE = (_D["SLAM_RAYCAST_" + n] for n in ("TILED", "GLOBAL", "TILED_MERGE"))
GDIST_FAR = _D["SLAM_GDIST_FAR"]
GNAV_FAR = _D["SLAM_GNAV_FAR"]
GSEG_DROPPED, GSEG_GROUND, GSEG_OBSTACLE, GSEG_OVERHEAD = (_D["SLAM_GSEG_" + n] for n in ("DROPPED", "GROUND", "OBSTACLE", "OVERHEAD"))
KF_NOT_CONVERGED, KF_ITERATIONS, KF_TRANSFORM, KF_ABS_MSE, KF_REL_MSE, KF_NO_CORRESPONDENCES, KF_DEGENERATE = \
    (_D["SLAM_KF_" + n] for n in ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES", "DEGENERATE"))
PGO_ORDER_RCM, PGO_ORDER_NATURAL, PGO_TRACE = _D["SLAM_PGO_ORDER_RCM"], _D["SLAM_PGO_ORDER_NATURAL"], _D["SLAM_PGO_TRACE"]
PGO_STOP_ITERATIONS, PGO_STOP_MAX_TRIALS, PGO_STOP_RHO_ZERO = (_D["SLAM_PGO_STOP_" + n] for n in ("ITERATIONS", "MAX_TRIALS", "RHO_ZERO"))
COMM_SUM, COMM_MIN = _D["SLAM_COMM_SUM"], _D["SLAM_COMM_MIN"]
MERGE_THEN_NOTHING, MERGE_THEN_FINALIZE_RESET, MERGE_THEN_FOLD_FINALIZE = \
    (_D["SLAM_MERGE_THEN_" + n] for n in ("NOTHING", "FINALIZE_RESET", "FOLD_FINALIZE"))
HOST_ALLREDUCE_FN = _H.callbacks["slam_host_allreduce_fn"]

# Python name -> the header's struct.  Two fields carry a trailing underscore because the header's names are Python
# keywords: KfEdgeReq.from_ and PgoTrial.lambda_.
STRUCTS = {
    "IcpParams": "slam_icp_params", "IcpResult": "slam_icp_result", "GridParams": "slam_grid_params",
    "GdistParams": "slam_gdist_params", "MapperParams": "slam_mapper_params", "GsegParams": "slam_gseg_params",
    "MlsParams": "slam_mls_params", "KfParams": "slam_kf_params", "KfEdgeReq": "slam_kf_edge_req",
    "KfEdgeResult": "slam_kf_edge_result", "KfGicpParams": "slam_kf_gicp_params", "KfGicpResult": "slam_kf_gicp_result",
    "KfScParams": "slam_kf_sc_params", "KfScMatch": "slam_kf_sc_match_t", "CsmParams": "slam_csm_params",
    "CsmResult": "slam_csm_result", "CsmPostParams": "slam_csm_post_params", "VmapParams": "slam_vmap_params",
    "VmapCarveParams": "slam_vmap_carve_params", "VmapCarveResult": "slam_vmap_carve_result",
    "VmapDistParams": "slam_vmap_dist_params", "VmapGicpReq": "slam_vmap_gicp_req", "VmapGicpParams": "slam_vmap_gicp_params",
    "VmapGicpResult": "slam_vmap_gicp_result", "VmapSearchParams": "slam_vmap_search_params",
    "VmapSearchHit": "slam_vmap_search_hit", "PgoParams": "slam_pgo_params", "PgoTrial": "slam_pgo_trial",
    "PgoResult": "slam_pgo_result", "CommStats": "slam_comm_stats",
    "PfParams": "slam_pf_params", "PfMotion": "slam_pf_motion", "PfState": "slam_pf_state",
    "GnavParams": "slam_gnav_params", "GnavState": "slam_gnav_state",
}
globals().update((py, _H.structs[c]) for py, c in STRUCTS.items())


class SlamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("slam_mi355x error %d: %s" % (code, msg))
        self.code = code


class CsmPosterior(_H.structs["slam_csm_posterior"]):
    """slam_csm_posterior (docs/CSM.md section 6).  The helpers mirror slam_amd::Posterior of correlative.hpp operation for
    operation; `u` is (resolution, resolution, theta_step), which CorrelativeMatcher.match_post fills in."""
    u = (0.0, 0.0, 0.0)
    score = n_points = 0

    def covariance(self, floor=True):
        """3 x 3, row-major x y theta; floor: u_i^2 / 12 on the diagonal, a pose is not known better than one cell"""
        c = self.cov
        out = np.array([c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]], np.float64)
        if floor:
            for i in range(3):
                out[4 * i] = out[4 * i] + (np.float64(self.u[i]) * np.float64(self.u[i])) / np.float64(12.0)
        return out.reshape(3, 3)

    def information(self):
        """the inverse of the floored covariance by the symmetric adjugate, or None when the determinant is not positive
        and finite"""
        m = self.covariance(True).reshape(9)
        a, b, c, d, e, f = (np.float64(m[i]) for i in (0, 1, 2, 4, 5, 8))
        A, B, Cc = d * f - e * e, c * e - b * f, b * e - c * d
        D, E, F = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * A + b * B) + c * Cc
        if not (det > 0.0 and np.isfinite(det)):
            return None
        return np.array([A / det, B / det, Cc / det, B / det, D / det, E / det, Cc / det, E / det, F / det]).reshape(3, 3)

    def ambiguous(self, max_deficit_per_point):
        """a second, separate pose scores within max_deficit_per_point * n_points of the winner"""
        return bool(self.valid and self.second_score >= 0 and
                    self.score - self.second_score <= int(max_deficit_per_point) * self.n_points)


CSM_RESULT_DTYPE = np.dtype([(f, np.int32) for f, _ in CsmResult._fields_])
CSM_POST_DTYPE = np.dtype([(f, np.int32) for f, _ in CsmPosterior._fields_[:8]] +
                          [("m0", np.int64), ("m1", np.int64, (3,)), ("m2", np.int64, (6,)), ("mean", np.float64, (3,)),
                           ("cov", np.float64, (6,))])

# one motion in a device buffer, as slam_pf_predict_dev reads it there: slam_pf_motion without its reserved word
_m = np.dtype(PfMotion)
_f = [n for n in _m.names if n != "reserved"]
PF_MOTION_DTYPE = np.dtype({"names": _f, "formats": [_m.fields[n][0] for n in _f], "offsets": [_m.fields[n][1] for n in _f],
                            "itemsize": _m.itemsize})
GNAV_REACHED, GNAV_NO_START, GNAV_CUT, GNAV_NOT_CONVERGED = \
    (_D["SLAM_GNAV_PATH_" + n] for n in ("REACHED", "NO_START", "CUT", "NOT_CONVERGED"))

KF_LATTICE_MARGIN = 1.0 + 2.0 ** -16   # the search lattice's edge is cell_size (or the gate) times this

RESULT_DTYPE = np.dtype([("iters", np.int32), ("n_corr", np.int32), ("delta", np.float64)])

_vp = C.c_void_p
_lib = None


def lib():
    """Loads slam_amd/lib/libslam_mi355x.so (built by slam_amd.build).  Loud if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SlamError(E_NO_DEVICE, "HIP library not built: %s is missing "
                        "(run `python -m slam_amd.build`); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    _H.bind(L, EXPORTS + _MEASURE_EXPORTS)
    _lib = L
    return L


def check(rc):
    if rc != SLAM_OK:
        raise SlamError(rc, lib().slam_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    check(lib().slam_device_count(C.byref(n)))
    return n.value


def set_device(i):
    check(lib().slam_set_device(int(i)))


def device_info():
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(), C.c_size_t()
    check(lib().slam_device_info(name, 256, C.byref(cu), C.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def synchronize():
    check(lib().slam_device_synchronize())


def _ptr(a):
    return a.ctypes.data_as(_vp) if a is not None and a.size else None


class DeviceArray:
    """A typed block of HBM owned through slam_malloc / slam_free."""

    def __init__(self, shape, dtype):
        self.shape = tuple(np.atleast_1d(shape).tolist()) if not isinstance(shape, tuple) else shape
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = _vp()
        check(lib().slam_malloc(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value

    @classmethod
    def from_host(cls, a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        d = cls(a.shape, a.dtype)
        d.upload(a)
        return d

    def upload(self, a, stream=None):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes
        check(lib().slam_memcpy_h2d(self.ptr, _ptr(a), self.nbytes, stream))

    def download(self, stream=None):
        out = np.empty(self.shape, dtype=self.dtype)
        check(lib().slam_memcpy_d2h(_ptr(out), self.ptr, self.nbytes, stream))
        return out

    def upload_async(self, pinned, stream):
        assert pinned.nbytes == self.nbytes
        check(lib().slam_memcpy_h2d_async(self.ptr, pinned.ptr, self.nbytes, _sp(stream)))

    def download_async(self, pinned, stream):
        assert pinned.nbytes == self.nbytes
        check(lib().slam_memcpy_d2h_async(pinned.ptr, self.ptr, self.nbytes, _sp(stream)))

    def copy_from(self, other, stream=None):
        assert other.nbytes == self.nbytes
        check(lib().slam_memcpy_d2d(self.ptr, other.ptr, self.nbytes, _sp(stream)))

    def zero(self, stream=None):
        check(lib().slam_memset(self.ptr, 0, self.nbytes, _sp(stream)))

    def view(self, first, shape):
        """`shape` elements of this block from element `first` on: shares the memory, does not own it."""
        v = object.__new__(DeviceArray)
        v.shape = tuple(shape)
        v.dtype = self.dtype
        v.nbytes = int(np.prod(v.shape)) * self.dtype.itemsize
        assert first >= 0 and first * self.dtype.itemsize + v.nbytes <= self.nbytes
        v.ptr = self.ptr + first * self.dtype.itemsize
        v.owner = self   # keeps the block alive
        return v

    def free(self):
        if getattr(self, "ptr", None) and getattr(self, "owner", None) is None:
            lib().slam_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """A numpy view over pinned host memory (slam_host_alloc), for asynchronous copies."""

    def __init__(self, shape, dtype):
        self.shape = shape if isinstance(shape, tuple) else (int(shape),)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = _vp()
        check(lib().slam_host_alloc(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value
        buf = (C.c_char * max(self.nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib().slam_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Handle:
    """What the library creates and Python owns.  A subclass names, once, the entry point that frees it (`_destroy`) and,
    if it is not `h`, the attribute that holds it (`_field`).  close() may be called any number of times, also on an object
    whose constructor raised before the handle existed; `with` closes."""
    _destroy = None
    _field = "h"
    _library = staticmethod(lib)

    def close(self):
        p = getattr(self, self._field, None)
        if p:
            getattr(self._library(), self._destroy)(p)
            setattr(self, self._field, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Stream(_Handle):
    _destroy, _field = "slam_stream_destroy", "ptr"

    def __init__(self, priority=None, reserve_cus_per_xcd=0, private_queue=False):
        """reserve_cus_per_xcd > 0: a stream whose kernels leave that many CUs of every XCD alone; private_queue: a stream with a
        hardware queue of its own (slam_stream_create_reserving_cus with 0; such streams have no priority of their own)."""
        p = _vp()
        if reserve_cus_per_xcd or private_queue:
            check(lib().slam_stream_create_reserving_cus(C.byref(p), int(reserve_cus_per_xcd)))
        elif priority is None:
            check(lib().slam_stream_create(C.byref(p)))
        else:
            check(lib().slam_stream_create_with_priority(C.byref(p), int(priority)))
        self.ptr = p.value

    def synchronize(self):
        check(lib().slam_stream_synchronize(self.ptr))

    def wait_event(self, ev):
        check(lib().slam_stream_wait_event(self.ptr, ev.ptr))

class Graph:
    """hipGraph of the library calls issued on `stream` inside the with-block (record once, replay).  Not a _Handle: its
    with-block records, it does not close."""

    def __init__(self, stream):
        self.stream, self.ptr = stream, None

    def __enter__(self):
        check(lib().slam_graph_begin_capture(self.stream.ptr))
        return self

    def __exit__(self, *exc):
        p = _vp()
        rc = lib().slam_graph_end_capture(self.stream.ptr, C.byref(p))
        if exc[0] is None:
            check(rc)
            self.ptr = p.value
        return False

    def launch(self, stream=None):
        check(lib().slam_graph_launch(self.ptr, (stream or self.stream).ptr))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().slam_graph_destroy(self.ptr)
            self.ptr = None


class Event(_Handle):
    _destroy, _field = "slam_event_destroy", "ptr"

    def __init__(self):
        p = _vp()
        check(lib().slam_event_create(C.byref(p)))
        self.ptr = p.value

    def record(self, stream=None):
        check(lib().slam_event_record(self.ptr, stream.ptr if isinstance(stream, Stream) else stream))

    def synchronize(self):
        check(lib().slam_event_synchronize(self.ptr))

    def query(self):
        """True when the work recorded before the event has finished (no wait)."""
        d = C.c_int()
        check(lib().slam_event_query(self.ptr, C.byref(d)))
        return bool(d.value)

    def elapsed_ms(self, later):
        ms = C.c_float()
        check(lib().slam_event_elapsed_ms(self.ptr, later.ptr, C.byref(ms)))
        return ms.value


def _sp(stream):
    return stream.ptr if isinstance(stream, Stream) else stream


def _defaults(struct, entry_point, kw):
    """the library's defaults of a parameter struct, with the fields named in kw set over them"""
    p = struct()
    getattr(lib(), entry_point)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _as(struct, address):
    """an address (a device array of structs, or None) for a parameter the header types as `struct *`"""
    return C.cast(address, C.POINTER(struct))


def icp_default_params(**kw):
    return _defaults(IcpParams, "slam_icp_default_params", kw)


class Icp(_Handle):
    """IcpPointToPoint-shaped handle (icpPointToPoint.h:26-40) over the C-ABI."""
    _destroy = "slam_icp_destroy"

    def __init__(self, m_ga, m_nga, params=None, **kw):
        self.m_ga = np.ascontiguousarray(m_ga, dtype=np.float64).reshape(-1, 2)
        self.m_nga = np.ascontiguousarray(m_nga, dtype=np.float64).reshape(-1, 2)
        self.params = params or icp_default_params(**kw)
        h = _vp()
        check(lib().slam_icp_create(_ptr(self.m_ga), len(self.m_ga), _ptr(self.m_nga),
                                    len(self.m_nga), C.byref(self.params), C.byref(h)))
        self.h = h.value

    @classmethod
    def from_device(cls, d_ga, n_ga, d_nga, n_nga, params=None, **kw):
        """slam_icp_create_dev: the model arrays (f64 xy) are DeviceArrays / device pointers."""
        self = object.__new__(cls)
        self.m_ga = self.m_nga = None
        self.n_model = (int(n_ga), int(n_nga))
        self.params = params or icp_default_params(**kw)
        h = _vp()
        check(lib().slam_icp_create_dev(getattr(d_ga, "ptr", d_ga), int(n_ga), getattr(d_nga, "ptr", d_nga), int(n_nga),
                                        C.byref(self.params), C.byref(h)))
        self.h = h.value
        return self

    def build_info(self):
        on, ms = C.c_int(0), (C.c_double * 4)()
        check(lib().slam_icp_build_info(self.h, C.byref(on), ms))
        return bool(on.value), list(ms)

    def index_blob(self, which):
        """The cell index (which = 0) or the halo lists (1) as they lie in HBM, as bytes."""
        n = C.c_size_t(0)
        check(lib().slam_icp_index_blob(self.h, int(which), None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        if n.value:
            check(lib().slam_icp_index_blob(self.h, int(which), _ptr(buf), n.value, None))
        return buf

    def read_model(self, cls):
        """The points of class cls (0 GA, 1 NGA) as the index holds them: f32 xy in original order within the class."""
        n = C.c_int(0)
        rc = lib().slam_icp_read_model(self.h, int(cls), None, 0, C.byref(n))    # the count: E_NOMEM says "more than 0"
        if rc not in (SLAM_OK, E_NOMEM):
            check(rc)
        out =np.zeros((n.value, 2), np.float32)
        if n.value:
            check(lib().slam_icp_read_model(self.h, int(cls), _ptr(out), n.value, C.byref(n)))
        return out

    def set_max_iterations(self, v):
        check(lib().slam_icp_set_max_iterations(self.h, int(v)))

    def set_min_delta(self, v):
        check(lib().slam_icp_set_min_delta(self.h, float(v)))

    def index_info(self):
        nx, ny, lanes, in_lds = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        cell, lds = C.c_double(), C.c_size_t()
        check(lib().slam_icp_index_info(self.h, C.byref(nx), C.byref(ny), C.byref(cell),
                                        C.byref(in_lds), C.byref(lds), C.byref(lanes)))
        two, first = C.c_int(), C.c_int()
        pitch, halo, cert, lb = C.c_double(), C.c_double(), C.c_double(), C.c_size_t()
        check(lib().slam_icp_list_info(self.h, C.byref(two), C.byref(first), C.byref(pitch), C.byref(halo),
                                       C.byref(cert), C.byref(lb)))
        return dict(nx=nx.value, ny=ny.value, cell=cell.value, in_lds=bool(in_lds.value),
                    lds_bytes=lds.value, lanes_per_point=lanes.value, two_forms=bool(two.value),
                    first_iterations=first.value, list_pitch=pitch.value, list_halo=halo.value,
                    list_certified_radius=cert.value, list_bytes=lb.value)

    def fit(self, t_ga, t_nga, R, t, indist=5.0):
        """Icp::fit (icp.cpp:80-114), host arrays; returns (R, t, IcpResult)."""
        t_ga = np.ascontiguousarray(t_ga, dtype=np.float64).reshape(-1, 2)
        t_nga = np.ascontiguousarray(t_nga, dtype=np.float64).reshape(-1, 2)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(4).copy()
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(2).copy()
        res = IcpResult()
        check(lib().slam_icp_fit(self.h, _ptr(t_ga), len(t_ga), _ptr(t_nga), len(t_nga),
                                 _ptr(R), _ptr(t), float(indist), C.byref(res)))
        return R.reshape(2, 2), t, res

    def fit_batch_dev(self, d_pts, d_off, d_nga, n_scans, d_R, d_t, indist=5.0, d_result=None,
                      d_trace=None, stream=None):
        check(lib().slam_icp_fit_batch_dev(
            self.h, d_pts.ptr, d_off.ptr, d_nga.ptr, int(n_scans), d_R.ptr, d_t.ptr, float(indist),
            _as(IcpResult, d_result.ptr if d_result is not None else None),
            d_trace.ptr if d_trace is not None else None, _sp(stream)))

    def fit_batch_from_dev(self, d_pts, d_off, d_nga, n_scans, d_R0, d_t0, d_R, d_t, indist=5.0, d_result=None,
                           d_trace=None, stream=None):
        """Initial poses read from d_R0 / d_t0, registered poses written to d_R / d_t."""
        check(lib().slam_icp_fit_batch_from_dev(
            self.h, d_pts.ptr, d_off.ptr, d_nga.ptr, int(n_scans), d_R0.ptr, d_t0.ptr, d_R.ptr, d_t.ptr, float(indist),
            _as(IcpResult, d_result.ptr if d_result is not None else None),
            d_trace.ptr if d_trace is not None else None, _sp(stream)))

    def fit_batch(self, batch, indist=5.0, trace=False):
        """Host convenience: uploads a synth.ScanBatch, runs, downloads.
        Returns (R[S,4], t[S,2], result[S], trace[S,max_iter,8] or None)."""
        S = batch.n_scans
        d_pts = DeviceArray.from_host(batch.pts, np.float64)
        d_off = DeviceArray.from_host(batch.scan_off, np.int32)
        d_nga = DeviceArray.from_host(batch.scan_nga, np.int32)
        d_R = DeviceArray.from_host(batch.R, np.float64)
        d_t = DeviceArray.from_host(batch.t, np.float64)
        d_res = DeviceArray((S,), RESULT_DTYPE)
        d_res.zero()
        d_tr = None
        if trace:
            d_tr = DeviceArray((S, max(self.params.max_iter, 1), 8), np.float64)
            d_tr.zero()
        self.fit_batch_dev(d_pts, d_off, d_nga, S, d_R, d_t, indist, d_res, d_tr)
        synchronize()
        return d_R.download(), d_t.download(), d_res.download(), (d_tr.download() if trace else None)

    def edge_weight(self):
        """IcpPointToPoint::getEdgeWeight (icpPointToPoint.cpp:233-316) of the last fit()."""
        out = np.zeros(9)
        check(lib().slam_icp_get_edge_weight(self.h, _ptr(out)))
        return out.reshape(3, 3)

    def normals(self):
        n = sum(self.n_model) if self.m_ga is None else len(self.m_ga) + len(self.m_nga)
        out = np.zeros((n, 2))
        check(lib().slam_icp_get_normals(self.h, _ptr(out)))
        return out

    def nearest(self, cls, q_xy):
        """KDTree::n_nearest(q, 1) for every row of q_xy (f32): (dis[n], idx[n])."""
        q = np.ascontiguousarray(q_xy, dtype=np.float32).reshape(-1, 2)
        d_q = DeviceArray.from_host(q)
        d_d = DeviceArray((len(q),), np.float32)
        d_i = DeviceArray((len(q),), np.int32)
        check(lib().slam_icp_nearest_dev(self.h, int(cls), d_q.ptr, len(q), d_d.ptr, d_i.ptr, None))
        synchronize()
        return d_d.download(), d_i.download()


def csm_default_params(**kw):
    return _defaults(CsmParams, "slam_csm_default_params", kw)


def csm_default_post_params(**kw):
    return _defaults(CsmPostParams, "slam_csm_default_post_params", kw)


class CorrelativeMatcher(_Handle):
    """The correlative scan matcher (slam_csm_*, docs/CSM.md): the best of N_theta x N_y x N_x poses around a start pose,
    the wide-basin start for Icp.fit.  The model arrays are Icp's."""
    _destroy = "slam_csm_destroy"

    def __init__(self, m_ga, m_nga, params=None, **kw):
        m_ga = np.ascontiguousarray(m_ga, dtype=np.float64).reshape(-1, 2)
        m_nga = np.ascontiguousarray(m_nga, dtype=np.float64).reshape(-1, 2)
        self.params = params or csm_default_params(**kw)
        h = _vp()
        check(lib().slam_csm_create(_ptr(m_ga), len(m_ga), _ptr(m_nga), len(m_nga), C.byref(self.params), C.byref(h)))
        self.h = h.value
        self.params = self.info()["params"]

    @classmethod
    def from_device(cls, d_ga, n_ga, d_nga, n_nga, params=None, **kw):
        """slam_csm_create_dev: the model arrays (f64 xy) are DeviceArrays / device pointers."""
        self = object.__new__(cls)
        self.params = params or csm_default_params(**kw)
        h = _vp()
        check(lib().slam_csm_create_dev(getattr(d_ga, "ptr", d_ga), int(n_ga), getattr(d_nga, "ptr", d_nga), int(n_nga),
                                        C.byref(self.params), C.byref(h)))
        self.h = h.value
        self.params = self.info()["params"]
        return self

    @classmethod
    def from_plane(cls, plane, origin_x, origin_y, params=None, shape=None, **kw):
        """slam_csm_create_from_plane[_dev] (docs/GRID_MATCH.md): the table is the u8 plane itself, [h, w] with element (0, 0) at
        lattice cell (origin_x, origin_y).  plane: a host array, or a DeviceArray / device pointer with shape=(h, w)."""
        self = object.__new__(cls)
        self.params = params or csm_default_params(**kw)
        h = _vp()
        if isinstance(plane, DeviceArray) or isinstance(plane, int):
            ph, pw = shape if shape is not None else plane.shape
            check(lib().slam_csm_create_from_plane_dev(getattr(plane, "ptr", plane), int(pw), int(ph), int(origin_x), int(origin_y),
                                                       C.byref(self.params), C.byref(h)))
        else:
            plane = np.ascontiguousarray(plane, dtype=np.uint8)
            assert plane.ndim == 2
            ph, pw = plane.shape
            check(lib().slam_csm_create_from_plane(plane.ctypes.data_as(_vp), int(pw), int(ph), int(origin_x), int(origin_y),
                                                   C.byref(self.params), C.byref(h)))
        self.h = h.value
        self.plane_shape = (int(ph), int(pw))
        self.params = self.info()["params"]
        return self

    def set_plane_dev(self, d_plane, origin_x, origin_y, stream=None):
        """slam_csm_set_plane_dev: another plane of the same size (a DeviceArray is held to it; a bare pointer cannot be) at
        any origin, a copy and the slide enqueued on `stream`"""
        if isinstance(d_plane, DeviceArray) and getattr(self, "plane_shape", None) is not None \
                and d_plane.nbytes != self.plane_shape[0] * self.plane_shape[1]:
            raise SlamError(E_INVALID, "CorrelativeMatcher.set_plane_dev: a plane of %d bytes, the handle's has %d x %d"
                            % (d_plane.nbytes, self.plane_shape[1], self.plane_shape[0]))
        check(lib().slam_csm_set_plane_dev(self.h, getattr(d_plane, "ptr", d_plane), int(origin_x), int(origin_y), _sp(stream)))

    @staticmethod
    def poses(theta, tx, ty):
        """[P, 4] f64 (cos, sin, tx, ty) of poses given by angle and translation: what score_poses reads (host libm)"""
        theta = np.asarray(theta, np.float64).ravel()
        return np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta), np.asarray(tx, np.float64).ravel(),
                                              np.asarray(ty, np.float64).ravel()], axis=1))

    def score_poses_dev(self, d_pts, n, n_ga, d_poses, n_poses, d_score, d_counted, stream=None):
        check(lib().slam_csm_score_poses_dev(self.h, getattr(d_pts, "ptr", d_pts), int(n), int(n_ga), getattr(d_poses, "ptr", d_poses),
                                             int(n_poses), getattr(d_score, "ptr", d_score), getattr(d_counted, "ptr", d_counted),
                                             _sp(stream)))

    def score_poses(self, t_ga, t_nga, poses):
        """slam_csm_score_poses, host arrays; poses [P, 4] (cos, sin, tx, ty): (score int32 [P], counted int32 [P])"""
        t_ga, t_nga = np.reshape(t_ga, (-1, 2)), np.reshape(t_nga, (-1, 2))
        pts = np.ascontiguousarray(np.concatenate([t_ga, t_nga]), dtype=np.float64)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        score, counted = np.zeros(len(poses), np.int32), np.zeros(len(poses), np.int32)
        check(lib().slam_csm_score_poses(self.h, _ptr(pts), len(pts), len(t_ga), _ptr(poses), len(poses), _ptr(score), _ptr(counted)))
        return score, counted

    def info(self):
        p, dims, tb, sb, ms = CsmParams(), (C.c_int * 5)(), C.c_size_t(), C.c_size_t(), C.c_int()
        check(lib().slam_csm_info(self.h, C.byref(p), dims, C.byref(tb), C.byref(sb), C.byref(ms)))
        return dict(params=p, n_theta=dims[0], n_x=dims[1], n_y=dims[2], blocks_x=dims[3], blocks_y=dims[4],
                    table_bytes=tb.value, scratch_bytes=sb.value, max_scans=ms.value)

    def reserve(self, max_scans):
        check(lib().slam_csm_reserve(self.h, int(max_scans)))

    def set_window(self, half_x, half_y, half_theta, theta_step):
        check(lib().slam_csm_set_window(self.h, int(half_x), int(half_y), int(half_theta), float(theta_step)))
        self.params = self.info()["params"]

    def set_exhaustive(self, on):
        check(lib().slam_csm_set_exhaustive(self.h, int(bool(on))))
        self.params.exhaustive = int(bool(on))

    def angles(self, R0):
        """cos, sin of every candidate angle around R0's: [N_theta, 2] f64 (host libm; the device reads them)."""
        R0 = np.ascontiguousarray(R0, dtype=np.float64).reshape(4)
        cs = np.zeros((2 * self.params.half_theta + 1, 2))
        check(lib().slam_csm_angles(self.h, _ptr(R0), _ptr(cs)))
        return cs

    def table(self, cls, level=0):
        """(origin_x, origin_y, u8 [h, w]) of class cls: level 0 = T, 1 = W; a class without a table has shape (0, 0)."""
        ox, oy, w, h = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().slam_csm_read_table(self.h, int(cls), int(level), C.byref(ox), C.byref(oy), C.byref(w), C.byref(h), None, 0))
        buf = np.zeros((h.value, w.value), np.uint8)
        if buf.size:
            check(lib().slam_csm_read_table(self.h, int(cls), int(level), None, None, None, None, _ptr(buf), buf.size))
        return ox.value, oy.value, buf

    def match(self, t_ga, t_nga, R, t):
        """slam_csm_match, host arrays: (R, t, CsmResult)."""
        t_ga = np.ascontiguousarray(t_ga, dtype=np.float64).reshape(-1, 2)
        t_nga = np.ascontiguousarray(t_nga, dtype=np.float64).reshape(-1, 2)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(4).copy()
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(2).copy()
        res = CsmResult()
        check(lib().slam_csm_match(self.h, _ptr(t_ga), len(t_ga), _ptr(t_nga), len(t_nga), _ptr(R), _ptr(t), C.byref(res)))
        return R.reshape(2, 2), t, res

    def match_batch_dev(self, d_pts, d_off, d_nga, n_scans, d_R0, d_t0, d_cs, d_R, d_t, d_result=None, stream=None):
        check(lib().slam_csm_match_batch_dev(self.h, d_pts.ptr, d_off.ptr, d_nga.ptr, int(n_scans), d_R0.ptr, d_t0.ptr, d_cs.ptr,
                                             d_R.ptr, d_t.ptr, _as(CsmResult, d_result.ptr if d_result is not None else None), _sp(stream)))

    def match_batch(self, batch, R0=None, t0=None):
        """Host convenience over a synth.ScanBatch: (R [S, 4], t [S, 2], result [S] of CSM_RESULT_DTYPE)."""
        S = batch.n_scans
        R0 = np.ascontiguousarray(batch.R if R0 is None else R0, dtype=np.float64).reshape(S, 4)
        t0 = np.ascontiguousarray(batch.t if t0 is None else t0, dtype=np.float64).reshape(S, 2)
        self.reserve(S)
        d_pts = DeviceArray.from_host(batch.pts, np.float64)
        d_off = DeviceArray.from_host(batch.scan_off, np.int32)
        d_nga = DeviceArray.from_host(batch.scan_nga, np.int32)
        d_R0, d_t0 = DeviceArray.from_host(R0), DeviceArray.from_host(t0)
        d_cs = DeviceArray.from_host(np.stack([self.angles(R0[s]) for s in range(S)]))
        d_R, d_t = DeviceArray((S, 4), np.float64), DeviceArray((S, 2), np.float64)
        d_res = DeviceArray((S,), CSM_RESULT_DTYPE)
        self.match_batch_dev(d_pts, d_off, d_nga, S, d_R0, d_t0, d_cs, d_R, d_t, d_res)
        synchronize()
        return d_R.download(), d_t.download(), d_res.download()

    # ---- the posterior of a match (docs/CSM.md section 6)
    def set_post_params(self, params=None, **kw):
        """slam_csm_set_post_params: the weight table and the per-scan scratch; the match_post calls need it first"""
        self.post_params = params or csm_default_post_params(**kw)
        check(lib().slam_csm_set_post_params(self.h, C.byref(self.post_params)))

    def post_table(self):
        """the 257 weights in force, uint32"""
        w = np.zeros(257, np.uint32)
        check(lib().slam_csm_read_post_table(self.h, _ptr(w), 257))
        return w

    def _units(self):
        return (self.params.resolution, self.params.resolution, self.params.theta_step)

    def match_post(self, t_ga, t_nga, R, t):
        """slam_csm_match_post, host arrays: (R, t, CsmResult, CsmPosterior)"""
        t_ga = np.ascontiguousarray(t_ga, dtype=np.float64).reshape(-1, 2)
        t_nga = np.ascontiguousarray(t_nga, dtype=np.float64).reshape(-1, 2)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(4).copy()
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(2).copy()
        res, post = CsmResult(), CsmPosterior()
        check(lib().slam_csm_match_post(self.h, _ptr(t_ga), len(t_ga), _ptr(t_nga), len(t_nga), _ptr(R), _ptr(t), C.byref(res),
                                        C.byref(post)))
        post.u, post.score, post.n_points = self._units(), res.score, res.n_points
        return R.reshape(2, 2), t, res, post

    def match_post_batch_dev(self, d_pts, d_off, d_nga, n_scans, d_R0, d_t0, d_cs, d_R, d_t, d_result, d_post, stream=None):
        check(lib().slam_csm_match_post_batch_dev(self.h, d_pts.ptr, d_off.ptr, d_nga.ptr, int(n_scans), d_R0.ptr, d_t0.ptr,
                                                  d_cs.ptr, d_R.ptr, d_t.ptr, _as(CsmResult, d_result.ptr if d_result is not None else None),
                                                  _as(CsmPosterior, d_post.ptr), _sp(stream)))

    def match_post_batch(self, batch, R0=None, t0=None):
        """match_batch with the posteriors: (R [S, 4], t [S, 2], result [S], posterior [S] of CSM_POST_DTYPE)."""
        S = batch.n_scans
        R0 = np.ascontiguousarray(batch.R if R0 is None else R0, dtype=np.float64).reshape(S, 4)
        t0 = np.ascontiguousarray(batch.t if t0 is None else t0, dtype=np.float64).reshape(S, 2)
        self.reserve(S)
        d_pts = DeviceArray.from_host(batch.pts, np.float64)
        d_off = DeviceArray.from_host(batch.scan_off, np.int32)
        d_nga = DeviceArray.from_host(batch.scan_nga, np.int32)
        d_R0, d_t0 = DeviceArray.from_host(R0), DeviceArray.from_host(t0)
        d_cs = DeviceArray.from_host(np.stack([self.angles(R0[s]) for s in range(S)]))
        d_R, d_t = DeviceArray((S, 4), np.float64), DeviceArray((S, 2), np.float64)
        d_res, d_post = DeviceArray((S,), CSM_RESULT_DTYPE), DeviceArray((S,), CSM_POST_DTYPE)
        self.match_post_batch_dev(d_pts, d_off, d_nga, S, d_R0, d_t0, d_cs, d_R, d_t, d_res, d_post)
        synchronize()
        return d_R.download(), d_t.download(), d_res.download(), d_post.download()

    def score_volume(self, t_ga, t_nga, R0, t0):
        """Every score of one scan: int32 [N_theta, N_y, N_x] (slam_csm_score_volume_dev)."""
        pts = np.ascontiguousarray(np.concatenate([np.reshape(t_ga, (-1, 2)), np.reshape(t_nga, (-1, 2))]), dtype=np.float64)
        i = self.info()
        d_pts = DeviceArray.from_host(pts)
        d_t0 = DeviceArray.from_host(np.ascontiguousarray(t0, dtype=np.float64).reshape(2))
        d_cs = DeviceArray.from_host(self.angles(R0))
        d_vol = DeviceArray((i["n_theta"], i["n_y"], i["n_x"]), np.int32)
        check(lib().slam_csm_score_volume_dev(self.h, d_pts.ptr, len(pts), len(np.reshape(t_ga, (-1, 2))), d_t0.ptr, d_cs.ptr,
                                              d_vol.ptr, None))
        synchronize()
        return d_vol.download()


def pgo_default_params(**kw):
    return _defaults(PgoParams, "slam_pgo_default_params", kw)


class PoseGraph(_Handle):
    """The pose-graph optimiser (slam_pgo_*, docs/PGO.md): SE3 vertices (x y z, quaternion x y z w) and edges with a 6 x 6
    information, Levenberg-Marquardt as graph_slam's optimizeGraph runs it.  The graph is host state; optimize, chi2,
    read_system and step run on the device."""
    _destroy = "slam_pgo_destroy"

    def __init__(self, params=None, **kw):
        self.params = params or pgo_default_params(**kw)
        h = _vp()
        check(lib().slam_pgo_create(C.byref(self.params), C.byref(h)))
        self.h = h.value

    @staticmethod
    def _f64(a, n):
        return np.ascontiguousarray(a, dtype=np.float64).reshape(n)

    def clear(self):
        check(lib().slam_pgo_clear(self.h))

    def add_vertex(self, id, pose7, fixed=False):
        check(lib().slam_pgo_add_vertex(self.h, int(id), _ptr(self._f64(pose7, 7)), int(bool(fixed))))

    def set_vertex(self, id, pose7):
        check(lib().slam_pgo_set_vertex(self.h, int(id), _ptr(self._f64(pose7, 7))))

    def add_edge(self, from_, to, meas7, info36):
        check(lib().slam_pgo_add_edge(self.h, int(from_), int(to), _ptr(self._f64(meas7, 7)), _ptr(self._f64(info36, 36))))

    def size(self):
        """(vertices, edges)"""
        nv, ne = C.c_int(), C.c_int()
        check(lib().slam_pgo_size(self.h, C.byref(nv), C.byref(ne)))
        return nv.value, ne.value

    def optimize(self, iterations=10, stream=None):
        """slam_pgo_optimize: the PgoResult; the estimates replace the poses (read_vertices)."""
        res = PgoResult()
        check(lib().slam_pgo_optimize(self.h, int(iterations), C.byref(res), _sp(stream)))
        return res

    def read_vertices(self):
        """[n, 7] f64, quaternions with w >= 0"""
        n = self.size()[0]
        out = np.zeros((n, 7))
        got = C.c_int()
        check(lib().slam_pgo_read_vertices(self.h, _ptr(out), n, C.byref(got)))
        return out

    def chi2(self, stream=None):
        """slam_pgo_chi2: (chi2, e [edges, 6], chi2 per edge) at the current poses"""
        ne = self.size()[1]
        total, e, ce = C.c_double(), np.zeros((ne, 6)), np.zeros(ne)
        check(lib().slam_pgo_chi2(self.h, C.byref(total), _ptr(e), _ptr(ce), _sp(stream)))
        return total.value, e, ce

    def read_system(self, stream=None):
        """slam_pgo_read_system: dict(rows, cols, blocks [k, 6, 6], b [vertices, 6], perm, w) of the undamped system"""
        nb, nf, w = C.c_int(), C.c_int(), C.c_int()
        check(lib().slam_pgo_read_system(self.h, None, None, None, 0, C.byref(nb), None, None, C.byref(nf), C.byref(w), _sp(stream)))
        rows, cols = np.zeros(nb.value, np.int32), np.zeros(nb.value, np.int32)
        blocks, b, perm = np.zeros((nb.value, 6, 6)), np.zeros((self.size()[0], 6)), np.zeros(nf.value, np.int32)
        check(lib().slam_pgo_read_system(self.h, _ptr(rows), _ptr(cols), _ptr(blocks), nb.value, C.byref(nb), _ptr(b), _ptr(perm),
                                         C.byref(nf), C.byref(w), _sp(stream)))
        return dict(rows=rows, cols=cols, blocks=blocks, b=b, perm=perm, w=w.value)

    def step(self, lam, stream=None):
        """slam_pgo_step: dict(delta [vertices, 6], chi2_before, chi2_after, scale, pivot) of one trial; applies nothing"""
        delta = np.zeros((self.size()[0], 6))
        c0, c1, sc, pv = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(lib().slam_pgo_step(self.h, float(lam), _ptr(delta), C.byref(c0), C.byref(c1), C.byref(sc), C.byref(pv), _sp(stream)))
        return dict(delta=delta, chi2_before=c0.value, chi2_after=c1.value, scale=sc.value, pivot=pv.value)

    # ---- the calls of slam_amd::PoseGraphOptimizer (include/slam_amd/pose_graph.hpp), graph_slam.cpp's optimiser globals
    def init_optimizer(self, cur_pose):
        """initOptimizer (:286-306): an empty graph with vertex 0 fixed at the origin in cur_pose's orientation; the first node's pose"""
        self.clear()
        first = np.concatenate([np.zeros(3), self._f64(cur_pose, 7)[3:]])
        self.add_vertex(0, first, True)
        return first

    @staticmethod
    def _tf_yaw(p):
        """tf::getYaw as slam_amd::detail::tf_yaw (include/slam_amd/pose.hpp) computes it"""
        qx, qy, qz, qw = (float(v) for v in p[3:7])
        s = 2.0 / (qx * qx + qy * qy + qz * qz + qw * qw)
        ys, zs = qy * s, qz * s
        wy, wz, xy, xz, yy, zz = qw * ys, qw * zs, qx * ys, qx * zs, qy * ys, qz * zs
        m00, m10, m20 = 1.0 - (yy + zz), xy + wz, xz - wy
        if abs(m20) >= 1.0:
            return 0.0
        cp = math.cos(-math.asin(m20))
        return math.atan2(m10 / cp, m00 / cp)

    @classmethod
    def pose_offset(cls, pre, post, cur_pose):
        """graph_slam.cpp:356-384 as written (not a rigid transform; see include/slam_amd/pose_graph.hpp)"""
        def wrapped(d):
            return -(d - 2 * math.pi) if d > math.pi else (-(d + 2 * math.pi) if d < -math.pi else d)
        pre, post, cur = ([float(v) for v in p] for p in (pre, post, cur_pose))
        vnx, vny, vnz = post[0] - pre[0], post[1] - pre[1], post[2] - pre[2]
        vnth = wrapped(cls._tf_yaw(post) - cls._tf_yaw(pre))
        vpx, vpy = cur[0] - pre[0], cur[1] - pre[1]
        vpth = wrapped(cls._tf_yaw(cur) - cls._tf_yaw(pre))
        half = (vnth + vpth) * 0.5
        return np.array([(vpx * math.cos(vnth) + vpy * math.sin(vnth) + vnx) - vpx, (vpy * math.cos(vnth) + vpx * math.sin(vnth) + vny) - vpy,
                         vnz, 0.0, 0.0, math.sin(half), math.cos(half)])

    def optimize_graph(self, node_poses, cur_pose, iterations=10):
        """optimizeGraph (:322-390): (the estimates [n, 7] that replace node_poses, the pose offset, the PgoResult)"""
        node_poses = np.reshape(np.asarray(node_poses, dtype=np.float64), (-1, 7))
        res = self.optimize(iterations)
        est = self.read_vertices()[:len(node_poses)]
        return est, self.pose_offset(node_poses[-1], est[-1], cur_pose), res


def vmap_default_params(**kw):
    return _defaults(VmapParams, "slam_vmap_default_params", kw)


def vmap_default_carve_params(**kw):
    return _defaults(VmapCarveParams, "slam_vmap_default_carve_params", kw)


def vmap_default_dist_params(**kw):
    return _defaults(VmapDistParams, "slam_vmap_default_dist_params", kw)


def vmap_default_gicp_params(**kw):
    return _defaults(VmapGicpParams, "slam_vmap_default_gicp_params", kw)


def vmap_default_search_params(**kw):
    return _defaults(VmapSearchParams, "slam_vmap_default_search_params", kw)


def vmap_search_hit_dict(h):
    return {"score": h.score, "k": h.k, "dx": h.dx, "dy": h.dy, "dz": h.dz, "n_with_cell": h.n_with_cell,
            "init": np.array(h.init[:], np.float32).reshape(4, 4)}


def vmap_gicp_result_dict(r):
    return {"transform": np.array(r.transform[:], np.float32).reshape(4, 4),
            "transform64": np.array(r.transform64[:], np.float64).reshape(4, 4), "iterations": r.iterations, "state": r.state,
            "converged": r.converged, "pairs": r.pairs, "mse": r.mse, "cost": r.cost,
            "hessian": np.array(r.hessian[:], np.float64).reshape(6, 6), "fitness": r.fitness, "fitness_pairs": r.fitness_pairs}


def vmap_carve_result_dict(r):
    return {f: int(getattr(r, f)) for f, _ in VmapCarveResult._fields_}


class VoxelMap(_Handle):
    """The exact sparse voxel map (slam_vmap_*, docs/VOXEL_MAP.md): clouds are integrated in place, each with its own
    transform; a voxel's centroid is the exact mean of its points in units of 2^-20 m, the same bits in any order."""
    _destroy = "slam_vmap_destroy"

    def __init__(self, params=None, **kw):
        self.params = params or vmap_default_params(**kw)
        h = _vp()
        check(lib().slam_vmap_create(C.byref(self.params), C.byref(h)))
        self.h = h.value

    @staticmethod
    def _Rt(R, t):
        if R is None and t is None:
            return None, None
        return (np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3))

    @staticmethod
    def _box(lo, hi):
        if lo is None and hi is None:
            return None, None
        return np.ascontiguousarray(lo, dtype=np.float32).reshape(2), np.ascontiguousarray(hi, dtype=np.float32).reshape(2)

    def info(self):
        nv, cap, npts, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_size_t()
        check(lib().slam_vmap_info(self.h, C.byref(nv), C.byref(cap), C.byref(npts), C.byref(b)))
        return dict(n_voxels=nv.value, capacity=cap.value, n_points=npts.value, device_bytes=b.value)

    def clear(self, stream=None):
        check(lib().slam_vmap_clear(self.h, _sp(stream)))

    def integrate(self, xyz, R=None, t=None):
        """slam_vmap_integrate, host array [n, >= 3] f32: the number of points dropped."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        R, t = self._Rt(R, t)
        nd = C.c_int()
        check(lib().slam_vmap_integrate(self.h, _ptr(xyz), len(xyz), xyz.shape[1], _ptr(R), _ptr(t), C.byref(nd)))
        return nd.value

    def integrate_dev(self, d_xyz, n, stride=3, R=None, t=None, stream=None):
        R, t = self._Rt(R, t)
        nd = C.c_int()
        check(lib().slam_vmap_integrate_dev(self.h, getattr(d_xyz, "ptr", d_xyz), int(n), int(stride), _ptr(R), _ptr(t), C.byref(nd),
                                            _sp(stream)))
        return nd.value

    def carve(self, xyz, R=None, t=None, origin=None, params=None, **kw):
        """slam_vmap_carve, host array [n, >= 3] f32 and the sensor origin in the cloud's frame (None: 0, 0, 0): the six
        counters of the call as a dict.  params: a VmapCarveParams, or its fields as keywords over the defaults."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        R, t = self._Rt(R, t)
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        p, r = params or vmap_default_carve_params(**kw), VmapCarveResult()
        check(lib().slam_vmap_carve(self.h, _ptr(xyz), len(xyz), xyz.shape[1], _ptr(R), _ptr(t), _ptr(o), C.byref(p), C.byref(r)))
        return vmap_carve_result_dict(r)

    def carve_dev(self, d_xyz, n, stride=3, R=None, t=None, origin=None, params=None, stream=None, **kw):
        """slam_vmap_carve_dev: as carve, on a device array of n points `stride` floats apart."""
        R, t = self._Rt(R, t)
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        p, r = params or vmap_default_carve_params(**kw), VmapCarveResult()
        check(lib().slam_vmap_carve_dev(self.h, getattr(d_xyz, "ptr", d_xyz), int(n), int(stride), _ptr(R), _ptr(t), _ptr(o), C.byref(p),
                                        C.byref(r), _sp(stream)))
        return vmap_carve_result_dict(r)

    def read_carve(self):
        """slam_vmap_read_carve: (seen [n] u32, miss [n] u32, key [n] u64) of every voxel; zeros on a map never carved."""
        n = self.info()["n_voxels"]
        seen, miss, key = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        got = C.c_int()
        check(lib().slam_vmap_read_carve(self.h, _ptr(seen), _ptr(miss), _ptr(key), n, C.byref(got)))
        assert got.value == n
        return seen, miss, key

    def extract_dev(self, d_xyz4, cap, lo=None, hi=None, min_count=0, d_count=None, d_key=None, stream=None, max_miss=None):
        """slam_vmap_extract_dev: the number of voxels written; SlamError(E_NOMEM) with .needed set when cap is too small.
        max_miss = (num, den): slam_vmap_extract_carved_dev, which keeps a voxel iff miss den <= max(seen, 1) num."""
        lo, hi = self._box(lo, hi)
        n = C.c_int()
        out = (getattr(d_xyz4, "ptr", d_xyz4), getattr(d_count, "ptr", d_count), getattr(d_key, "ptr", d_key), int(cap), C.byref(n), _sp(stream))
        if max_miss is not None:
            rc = lib().slam_vmap_extract_carved_dev(self.h, _ptr(lo), _ptr(hi), int(min_count), int(max_miss[0]), int(max_miss[1]), *out)
        else:
            rc = lib().slam_vmap_extract_dev(self.h, _ptr(lo), _ptr(hi), int(min_count), *out)
        if rc != SLAM_OK:
            e = SlamError(rc, lib().slam_last_error().decode("utf-8", "replace"))
            e.needed = n.value
            raise e
        return n.value

    def read(self, lo=None, hi=None, min_count=0, max_miss=None):
        """slam_vmap_read: (xyz4 [n, 4] f32, count [n] u32, key [n] u64) in ascending key order.  max_miss = (num, den):
        slam_vmap_read_carved."""
        lo, hi = self._box(lo, hi)
        n = C.c_int()
        if max_miss is not None:
            def call(*out):
                return lib().slam_vmap_read_carved(self.h, _ptr(lo), _ptr(hi), int(min_count), int(max_miss[0]), int(max_miss[1]), *out)
        else:
            def call(*out):
                return lib().slam_vmap_read(self.h, _ptr(lo), _ptr(hi), int(min_count), *out)
        rc = call(None, None, None, 0, C.byref(n))
        if rc not in (SLAM_OK, E_NOMEM):
            check(rc)
        xyz4, count, key = np.zeros((n.value, 4), np.float32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64)
        if n.value:
            check(call(_ptr(xyz4), _ptr(count), _ptr(key), n.value, C.byref(n)))
        return xyz4, count, key

    def read_sums(self):
        """slam_vmap_read_sums: (sums [n, 3] i64 in units of 2^-20 m, count [n] u32, key [n] u64) of every voxel."""
        n = self.info()["n_voxels"]
        sums, count, key = np.zeros((n, 3), np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        got = C.c_int()
        check(lib().slam_vmap_read_sums(self.h, _ptr(sums), _ptr(count), _ptr(key), n, C.byref(got)))
        assert got.value == n
        return sums, count, key

    # ---- plane distributions and Generalized ICP against the map (docs/VOXEL_MAP.md section 9)
    def enable_distributions(self, params=None, **kw):
        """slam_vmap_enable_distributions: legal on a map without voxels only.  params: a VmapDistParams, or its fields as
        keywords over the defaults."""
        p = params or vmap_default_dist_params(**kw)
        check(lib().slam_vmap_enable_distributions(self.h, C.byref(p)))
        self.dist_params = p

    def compute_distributions(self, stream=None):
        check(lib().slam_vmap_compute_distributions(self.h, _sp(stream)))

    def read_moments(self):
        """slam_vmap_read_moments: (E [n, 3] i64, M [n, 6] i64 as xx xy xz yy yz zz, key [n] u64) of every voxel."""
        n = self.info()["n_voxels"]
        E, M, key = np.zeros((n, 3), np.int64), np.zeros((n, 6), np.int64), np.zeros(n, np.uint64)
        got = C.c_int()
        check(lib().slam_vmap_read_moments(self.h, _ptr(E), _ptr(M), _ptr(key), n, C.byref(got)))
        assert got.value == n
        return E, M, key

    def read_distributions(self):
        """slam_vmap_read_distributions: a dict of centroid [n, 3] f32, normal [n, 3], cov6 [n, 6], eig [n, 3] f64 (descending),
        flag [n] u8 (1: plane voxel) and key [n] u64 of every voxel in key order."""
        n = self.info()["n_voxels"]
        d = dict(centroid=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3)), cov6=np.zeros((n, 6)), eig=np.zeros((n, 3)),
                 flag=np.zeros(n, np.uint8), key=np.zeros(n, np.uint64))
        got = C.c_int()
        check(lib().slam_vmap_read_distributions(self.h, _ptr(d["centroid"]), _ptr(d["normal"]), _ptr(d["cov6"]), _ptr(d["eig"]),
                                                 _ptr(d["flag"]), _ptr(d["key"]), n, C.byref(got)))
        assert got.value == n
        return d

    def register_gicp(self, store, src, init=None, params=None, trace=0, stream=None, **kw):
        """slam_vmap_register_gicp[_traced]: keyframe `src` of the KeyframeStore `store` against the map's plane voxels from
        the 4 x 4 `init`.  src may be a list of (src, init) pairs: one launch, a list of results.  Returns
        vmap_gicp_result_dict's fields ('pairs_trace' when trace > 0).  params: a VmapGicpParams, or its fields as keywords."""
        single = not isinstance(src, (list, tuple))
        reqs = [(src, init)] if single else list(src)
        n = len(reqs)
        req = (VmapGicpReq * max(n, 1))()
        for e, (kid, T) in enumerate(reqs):
            req[e].src = int(kid)
            req[e].init[:] = np.asarray(np.eye(4) if T is None else T, dtype=np.float32).reshape(16).tolist()
        p = params or vmap_default_gicp_params(**kw)
        res = (VmapGicpResult * max(n, 1))()
        tr = np.full((max(n, 1), max(trace, 1)), -1, np.int32)
        if trace > 0:
            check(lib().slam_vmap_register_gicp_traced(self.h, store.h, req, n, C.byref(p), res, _ptr(tr),
                                                       int(trace), _sp(stream)))
        else:
            check(lib().slam_vmap_register_gicp(self.h, store.h, req, n, C.byref(p), res, _sp(stream)))
        out = [vmap_gicp_result_dict(res[e]) for e in range(n)]
        if trace > 0:
            for e in range(n):
                out[e]["pairs_trace"] = tr[e].copy()
        return out[0] if single else out

    # ---- exhaustive lattice pose search (docs/VOXEL_MAP.md section 13)
    def search(self, xyz=None, params=None, volume=False, store=None, kid=None, d_xyz=None, n=0, stride=3, stream=None, **kw):
        """slam_vmap_search (xyz: host array [n, >= 3] f32), slam_vmap_search_keyframe (store and kid: the keyframe's filtered
        cloud) or slam_vmap_search_dev (d_xyz: n device points `stride` floats apart): every pose (k, dx, dy, dz) of the window
        scored by the number of points whose cell, moved by whole cells, holds a qualifying voxel.  (hits, volume): hits is a
        list of vmap_search_hit_dict's fields, best first; volume is the int32 [n_yaw, 2 wz + 1, 2 wy + 1, 2 wx + 1] scores
        when asked for, else None.  params: a VmapSearchParams, or its fields as keywords over the defaults."""
        p = params or vmap_default_search_params(**kw)
        hits, got = (VmapSearchHit * max(p.top_m, 1))(), C.c_int()
        vol = None
        if volume:
            vol = np.zeros((max(p.n_yaw, 0), 2 * p.wz + 1, 2 * p.wy + 1, 2 * p.wx + 1), np.int32)
        tail = (C.byref(p), hits, C.byref(got), _ptr(vol))
        if store is not None:
            check(lib().slam_vmap_search_keyframe(self.h, store.h, int(kid), *tail, _sp(stream)))
        elif d_xyz is not None:
            check(lib().slam_vmap_search_dev(self.h, getattr(d_xyz, "ptr", d_xyz), int(n), int(stride), *tail, _sp(stream)))
        else:
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
            xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
            check(lib().slam_vmap_search(self.h, _ptr(xyz), len(xyz), xyz.shape[1], *tail))
        return [vmap_search_hit_dict(hits[e]) for e in range(got.value)], vol

    # ---- snapshots and merging by the integer accumulators (docs/VOXEL_MAP.md section 10)
    def layout(self):
        """slam_vmap_layout: what a snapshot needs and info() does not tell: a dict of leaf, carved, distributions and
        dist_params (a VmapDistParams; the defaults' zeros of a map without distributions)."""
        leaf, carved, dist, dp = C.c_double(), C.c_int(), C.c_int(), VmapDistParams()
        check(lib().slam_vmap_layout(self.h, C.byref(leaf), C.byref(carved), C.byref(dist), C.byref(dp)))
        return dict(leaf=leaf.value, carved=bool(carved.value), distributions=bool(dist.value), dist_params=dp)

    def absorb(self, key, count, sums, seen=None, miss=None, E3=None, M6=None):
        """slam_vmap_absorb: adds n voxel records (key [n] u64, count [n] u32, sums [n, 3] i64, optionally seen and miss [n] u32,
        optionally E3 [n, 3] and M6 [n, 6] i64: what read_sums, read_carve and read_moments return) into the map by key.
        The number of records rejected."""
        key = np.ascontiguousarray(key, dtype=np.uint64).reshape(-1)
        n = len(key)

        def arr(a, dt, w):
            return None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(n * w)
        a = [key, arr(count, np.uint32, 1), arr(sums, np.int64, 3), arr(seen, np.uint32, 1), arr(miss, np.uint32, 1),
             arr(E3, np.int64, 3), arr(M6, np.int64, 6)]
        rej = C.c_int64()
        check(lib().slam_vmap_absorb(self.h, *[_ptr(x) for x in a], n, C.byref(rej)))
        return rej.value

    def absorb_dev(self, d_key, d_count, d_sums, n, d_seen=None, d_miss=None, d_E3=None, d_M6=None, stream=None):
        """slam_vmap_absorb_dev: as absorb, on device arrays of n records."""
        rej = C.c_int64()
        check(lib().slam_vmap_absorb_dev(self.h, *[getattr(x, "ptr", x) for x in (d_key, d_count, d_sums, d_seen, d_miss, d_E3, d_M6)],
                                         int(n), C.byref(rej), _sp(stream)))
        return rej.value

    def merge(self, other, stream=None):
        """slam_vmap_merge: every voxel of `other` (same leaf, distributions on both or neither) added into this map straight
        from its table; `other` is unchanged.  The number of records rejected (0 for a sound source)."""
        rej = C.c_int64()
        check(lib().slam_vmap_merge(self.h, other.h, C.byref(rej), _sp(stream)))
        return rej.value

    def coarsen(self, src, stream=None):
        """slam_vmap_coarsen: every voxel of the finer map `src` (this map's leaf is src's times 2, 4 .. 256, bit for bit;
        distributions on both or neither) added into the voxel of this map that contains it, the moments re-centred in
        integers: the bits of a map that integrated src's clouds at this leaf (docs/VOXEL_MAP.md section 11).  `src` is
        unchanged; carve planes are not derived."""
        check(lib().slam_vmap_coarsen(self.h, src.h, _sp(stream)))

    def save(self, path):
        """slam_vmap_save: the map's accumulators into the file of section 10.4; the bytes depend on the contents alone."""
        check(lib().slam_vmap_save(self.h, os.fsencode(path)))

    @classmethod
    def load(cls, path):
        """slam_vmap_load: a new map from a file of section 10.4 (SlamError E_INVALID: malformed, E_IO: unreadable)."""
        h = _vp()
        check(lib().slam_vmap_load(os.fsencode(path), C.byref(h)))
        m = cls.__new__(cls)
        m.h = h.value
        lay = m.layout()
        m.params = VmapParams(leaf=lay["leaf"], initial_capacity=m.info()["capacity"])
        if lay["distributions"]:
            m.dist_params = lay["dist_params"]
        return m


def grid_default_params(**kw):
    return _defaults(GridParams, "slam_grid_default_params", kw)


class Grid(_Handle):
    """MLS-in-occupancy-mode-shaped handle (mls.h:104-242) over the C-ABI."""
    _destroy = "slam_grid_destroy"

    def __init__(self, size_x, size_y, resolution, params=None, **kw):
        self.size_x, self.size_y, self.resolution = int(size_x), int(size_y), float(resolution)
        self.params = params or grid_default_params(**kw)
        h = _vp()
        check(lib().slam_grid_create(self.size_x, self.size_y, self.resolution,
                                     C.byref(self.params), C.byref(h)))
        self.h = h.value
        self.cells = self.size_x * self.size_y

    def clear(self, stream=None):
        check(lib().slam_grid_clear(self.h, _sp(stream)))

    def reset_counts(self, stream=None):
        check(lib().slam_grid_reset_counts(self.h, _sp(stream)))

    def set_pose(self, x, y, stream=None):
        check(lib().slam_grid_set_pose(self.h, float(x), float(y), _sp(stream)))

    def get_pose(self):
        x, y = C.c_double(), C.c_double()
        check(lib().slam_grid_get_pose(self.h, C.byref(x), C.byref(y)))
        return x.value, y.value

    def set_min_cluster_points(self, v):
        check(lib().slam_grid_set_min_cluster_points(self.h, int(v)))

    def set_max_range(self, v):
        check(lib().slam_grid_set_max_range(self.h, float(v)))

    @staticmethod
    def _pts(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim == 1:
            a = a.reshape(-1, 2)
        return a

    def add_endpoints(self, obs, gnd):
        obs, gnd = self._pts(obs), self._pts(gnd)
        stride = obs.shape[1] if obs.size else (gnd.shape[1] if gnd.size else 2)
        check(lib().slam_grid_add_endpoints(self.h, _ptr(obs), len(obs), _ptr(gnd), len(gnd), stride))

    def add_scan_inorder(self, obs, gnd):
        obs, gnd = self._pts(obs), self._pts(gnd)
        stride = obs.shape[1] if obs.size else (gnd.shape[1] if gnd.size else 2)
        check(lib().slam_grid_add_scan_inorder(self.h, _ptr(obs), len(obs), _ptr(gnd), len(gnd),
                                               stride))

    def raycast(self, origin_xy, end_xy):
        o, e = self._pts(origin_xy), self._pts(end_xy)
        assert o.shape == e.shape and o.shape[1] == 2
        check(lib().slam_grid_raycast(self.h, _ptr(o), _ptr(e), len(e)))

    def raycast_dev(self, d_origin, d_end, n, stream=None):
        check(lib().slam_grid_raycast_dev(self.h, d_origin.ptr, d_end.ptr, int(n), _sp(stream)))

    def raycast_scans_dev(self, d_pts, d_off, n_scans, n_points, d_R, d_t, stream=None):
        check(lib().slam_grid_raycast_scans_dev(self.h, d_pts.ptr, d_off.ptr, int(n_scans),
                                                int(n_points), d_R.ptr, d_t.ptr, _sp(stream)))

    def reserve(self, max_beams):
        check(lib().slam_grid_reserve(self.h, int(max_beams)))

    def finalize(self, stream=None):
        check(lib().slam_grid_finalize(self.h, _sp(stream)))

    def finalize_reset(self, stream=None):
        check(lib().slam_grid_finalize_reset(self.h, _sp(stream)))

    def read_counts(self):
        hits = np.empty(self.cells, dtype=np.int32)
        misses = np.empty(self.cells, dtype=np.int32)
        check(lib().slam_grid_read_counts(self.h, _ptr(hits), _ptr(misses)))
        return hits, misses

    def read_occupancy(self):
        occ = np.empty(self.cells, dtype=np.int8)
        check(lib().slam_grid_read_occupancy(self.h, _ptr(occ)))
        return occ

    def read_num_pts(self):
        v = np.empty(self.cells, dtype=np.float64)
        check(lib().slam_grid_read_num_pts(self.h, _ptr(v)))
        return v

    def total_updates(self):
        n = C.c_uint64()
        check(lib().slam_grid_total_updates(self.h, C.byref(n)))
        return n.value

    def info(self):
        sx, sy, ox, oy, res = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(lib().slam_grid_info(self.h, C.byref(sx), C.byref(sy), C.byref(res), C.byref(ox),
                                   C.byref(oy)))
        return dict(size_x=sx.value, size_y=sy.value, resolution=res.value, origin_x=ox.value,
                    origin_y=oy.value)

    def window_cell(self):
        x, y = C.c_int(), C.c_int()
        check(lib().slam_grid_window_cell(self.h, C.byref(x), C.byref(y)))
        return x.value, y.value

    def raycast_stats(self):
        t, i, s = C.c_int(), C.c_int(), C.c_int()
        check(lib().slam_grid_raycast_stats(self.h, C.byref(t), C.byref(i), C.byref(s)))
        return dict(tiles=t.value, items=i.value, tile_write_backs=s.value)

    def dirty_rows(self):
        lo, hi = C.c_int(), C.c_int()
        check(lib().slam_grid_dirty_rows(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def enable_accumulator(self):
        check(lib().slam_grid_enable_accumulator(self.h))

    def fold(self, row_lo, row_hi, stream=None):
        check(lib().slam_grid_fold(self.h, int(row_lo), int(row_hi), _sp(stream)))

    def mark_rows(self, lo, hi, stream=None):
        """storage rows lo..hi of the planes were written through counts_dev()'s pointer"""
        check(lib().slam_grid_mark_rows(self.h, int(lo), int(hi), _sp(stream)))

    def counts_dev(self):
        p, n = _vp(), C.c_size_t()
        check(lib().slam_grid_counts_dev(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def distance_field(self, df, stream=None):
        """df (a DistanceField of this grid's size) computed over the plane read_occupancy() returns; enqueues on `stream`"""
        check(lib().slam_grid_distance_field(self.h, df.h, _sp(stream)))

    def nav_field(self, distance_field, nav, goals, rounds=0, stream=None):
        """nav (a NavField of this grid's size) restarted from `goals` over distance_field's cost plane as it lies at this
        point of `stream`, then `rounds` rounds; goals: a device buffer of int32 pairs, or a host array (uploaded first)"""
        d_goals, n = nav._goals(goals)
        check(lib().slam_grid_nav_field(self.h, distance_field.h, nav.h, d_goals.ptr, n, int(rounds), _sp(stream)))


def gdist_default_params(**kw):
    return _defaults(GdistParams, "slam_gdist_default_params", kw)


def inflation_table(resolution, inscribed_radius, inflation_radius, cost_scaling, max_cells):
    """costmap_2d's inflation curve as the byte table a DistanceField looks its costs up in: np.uint8[max_cells**2 + 2],
    indexed by the squared distance in cells (slam_grid_inflation_table; host only)"""
    n = max(int(max_cells), 0) ** 2 + 2
    t = np.zeros(n, dtype=np.uint8)
    check(lib().slam_grid_inflation_table(float(resolution), float(inscribed_radius), float(inflation_radius), float(cost_scaling),
                                          int(max_cells), _ptr(t), n))
    return t


def likelihood_table(resolution, sigma, max_cells):
    """the correlative matcher's Gaussian stamp as the byte table a DistanceField looks its plane up in: np.uint8[max_cells**2 + 2]
    indexed by the squared distance in cells (slam_grid_likelihood_table; host only)"""
    n = max(int(max_cells), 0) ** 2 + 2
    t = np.zeros(n, dtype=np.uint8)
    check(lib().slam_grid_likelihood_table(float(resolution), float(sigma), int(max_cells), _ptr(t), n))
    return t


class DistanceField(_Handle):
    """Exact squared distance to the nearest obstacle cell of an occupancy plane, capped at max_cells, and the costmap read
    off it through a byte table (slam_gdist_*, docs/GRID_DIST.md).  Planes are window order, data[x + size_x * y]."""
    _destroy = "slam_gdist_destroy"

    def __init__(self, size_x, size_y, params=None, **kw):
        self.size_x, self.size_y = int(size_x), int(size_y)
        self.params = params or gdist_default_params(**kw)
        self.cells = self.size_x * self.size_y
        self.has_table = False
        h = _vp()
        check(lib().slam_gdist_create(self.size_x, self.size_y, C.byref(self.params), C.byref(h)))
        self.h = h.value

    def set_table(self, table, n=None):
        """np.uint8[max_cells**2 + 2] (n: its length, if given), or None (and 0) to remove the table (no cost plane)"""
        if table is None:
            check(lib().slam_gdist_set_table(self.h, None, int(n or 0)))
            self.has_table = False
            return
        t = np.ascontiguousarray(table, dtype=np.uint8).ravel()
        assert n is None or int(n) == len(t)
        check(lib().slam_gdist_set_table(self.h, t.ctypes.data_as(_vp), len(t)))
        self.has_table = True

    def set_inflation(self, resolution, inscribed_radius, inflation_radius, cost_scaling):
        self.set_table(inflation_table(resolution, inscribed_radius, inflation_radius, cost_scaling, self.params.max_cells))

    def compute(self, occ):
        occ = np.ascontiguousarray(occ, dtype=np.int8).ravel()
        assert occ.size == self.cells
        check(lib().slam_gdist_compute(self.h, _ptr(occ)))

    def compute_dev(self, d_occ, stream=None):
        check(lib().slam_gdist_compute_dev(self.h, getattr(d_occ, "ptr", d_occ), _sp(stream)))

    def read(self, cost=None):
        """(dist2 np.uint16[cells], cost np.uint8[cells] or None without a table); cost=True asks for the cost plane regardless"""
        d = np.empty(self.cells, dtype=np.uint16)
        c = np.empty(self.cells, dtype=np.uint8) if (self.has_table if cost is None else cost) else None
        check(lib().slam_gdist_read(self.h, _ptr(d), _ptr(c) if c is not None else None))
        return d, c

    def planes_dev(self):
        d, c = _vp(), _vp()
        check(lib().slam_gdist_planes_dev(self.h, C.byref(d), C.byref(c)))
        return d.value, c.value


def gnav_default_params(**kw):
    return _defaults(GnavParams, "slam_gnav_default_params", kw)


def step_table(neutral=None, lethal_from=None, unknown_step=None):
    """np.uint32[256] indexed by a cost byte: neutral + c below lethal_from, 0 (closed) from there on, [255] = unknown_step
    (slam_grid_step_table; host only).  None: the library's default."""
    d = gnav_default_params()
    t = np.zeros(256, np.uint32)
    check(lib().slam_grid_step_table(int(d.neutral if neutral is None else neutral), int(d.lethal_from if lethal_from is None else lethal_from),
                                     int(d.unknown_step if unknown_step is None else unknown_step), _ptr(t), len(t)))
    return t


class NavField(_Handle):
    """Exact cost-to-go from every cell of a cost plane to the nearest goal cell, and the path down it (slam_gnav_*,
    docs/GRID_NAV.md).  Planes are window order, data[x + size_x * y]; goals and paths are int32 (x, y) pairs."""
    _destroy = "slam_gnav_destroy"

    def __init__(self, size_x, size_y, orth_w=None, diag_w=None, params=None):
        """params: a GnavParams (gnav_default_params(...)); orth_w, diag_w, where given, go over its weights"""
        self.params = params or gnav_default_params()
        self.size_x, self.size_y = int(size_x), int(size_y)
        if orth_w is not None:
            self.params.orth_w = int(orth_w)
        if diag_w is not None:
            self.params.diag_w = int(diag_w)
        self.orth_w, self.diag_w = self.params.orth_w, self.params.diag_w
        self.cells = self.size_x * self.size_y
        h = _vp()
        check(lib().slam_gnav_create(self.size_x, self.size_y, C.byref(self.params), C.byref(h)))
        self.h = h.value
        self._d_goals = None

    def set_table(self, table):
        t = np.ascontiguousarray(table, dtype=np.uint32).ravel()
        check(lib().slam_gnav_set_table(self.h, _ptr(t), len(t)))

    def _goals(self, goals):
        """(device buffer, n) of goals given as a DeviceArray of int32 pairs or as a host array (kept until the next call)"""
        if isinstance(goals, DeviceArray):
            return goals, goals.nbytes // 8
        g = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        self._d_goals = DeviceArray.from_host(g) if len(g) else DeviceArray((1, 2), np.int32)
        return self._d_goals, len(g)

    def compute(self, cost, goals, max_rounds=0):
        """host plane and goals; synchronous, to convergence (SlamError E_TIMEOUT when max_rounds rounds did not suffice)"""
        cost = np.ascontiguousarray(cost, dtype=np.uint8).ravel()
        g = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        assert cost.size == self.cells
        check(lib().slam_gnav_compute(self.h, _ptr(cost), _ptr(g), len(g), int(max_rounds)))

    def compute_dev(self, d_cost, goals, rounds, restart=True, stream=None):
        d_goals, n = self._goals(goals)
        check(lib().slam_gnav_compute_dev(self.h, getattr(d_cost, "ptr", d_cost), d_goals.ptr, n, int(rounds), int(bool(restart)), _sp(stream)))

    def potential(self):
        """np.uint32[cells]; waits for the device"""
        p = np.empty(self.cells, np.uint32)
        check(lib().slam_gnav_read(self.h, _ptr(p)))
        return p

    def potential_dev(self):
        p = _vp()
        check(lib().slam_gnav_potential_dev(self.h, C.byref(p)))
        return p.value

    def path(self, start, max_len=None):
        """(int32 [len, 2] from the start to the goal, status); max_len None: the plane's cell count, which no path exceeds"""
        max_len = self.cells if max_len is None else int(max_len)
        out = np.zeros((max(max_len, 1), 2), np.int32)
        n, st = C.c_int(), C.c_int()
        check(lib().slam_gnav_path(self.h, int(start[0]), int(start[1]), max_len, _ptr(out), C.byref(n), C.byref(st)))
        return out[:n.value].copy(), st.value

    def path_dev(self, start, max_len, d_path, d_len_status, stream=None):
        """d_path: room for max_len int32 pairs; d_len_status: two int32 (length, status); enqueues on `stream`"""
        check(lib().slam_gnav_path_dev(self.h, int(start[0]), int(start[1]), int(max_len), getattr(d_path, "ptr", d_path),
                                       getattr(d_len_status, "ptr", d_len_status), _sp(stream)))

    def state(self):
        s = GnavState()
        check(lib().slam_gnav_read_state(self.h, C.byref(s)))
        return s


class GridMatcher:
    """Localises a scan in an occupancy grid itself (docs/GRID_MATCH.md): a DistanceField with a likelihood table
    (unknown_keep_from = 0: unknown cells keep their likelihood byte) whose cost plane is the table of a plane-built
    CorrelativeMatcher at the grid's resolution.  max_cells = 0: ceil(3 sigma / resolution - 1e-9), the matcher's own rule.

    Frames: the grid's window is centred on grid.get_pose() (0, 0 unless it rolls); the matcher works in the window's frame,
    whose cell (u, v) is plane element (u + size_x // 2, v + size_y // 2), the grid's own cell_coord.  This adapter subtracts the
    centre from a start translation and adds it to the answer, one f64 operation each; the C-ABI stays in the window's frame.
    The matcher keeps its cell rule (floor, f64), the grid's is (int) truncation on f32 points: inside the window they agree."""

    def __init__(self, grid, sigma, max_cells=0, params=None, **kw):
        self.grid = grid
        res = grid.resolution
        R = int(max_cells) if max_cells else int(np.ceil(3.0 * float(sigma) / res - 1e-9))
        self.sigma, self.max_cells = float(sigma), R
        self.table = likelihood_table(res, sigma, R)
        self.field = DistanceField(grid.size_x, grid.size_y, max_cells=R, unknown_keep_from=0)
        self.field.set_table(self.table)
        self.origin = (-(grid.size_x // 2), -(grid.size_y // 2))
        params = params or csm_default_params(**kw)
        params.resolution = res
        self.field.compute(np.zeros(grid.cells, np.int8))        # a plane to make the matcher from: update() brings the grid's
        self.matcher = CorrelativeMatcher.from_plane(self.field.planes_dev()[1], self.origin[0], self.origin[1], params,
                                                     shape=(grid.size_y, grid.size_x))
        self.centre = self._centre()

    def _centre(self):
        """the window's centre in the map frame: a rolling grid's pose (whole cells from 0, 0); a fixed grid stays at 0, 0"""
        return self.grid.get_pose() if self.grid.params.rolling else (0.0, 0.0)

    def update(self, stream=None):
        """slam_grid_distance_field then slam_csm_set_plane_dev on `stream`; waits for nothing"""
        self.grid.distance_field(self.field, stream)
        self.matcher.set_plane_dev(self.field.planes_dev()[1], self.origin[0], self.origin[1], stream)
        self.centre = self._centre()

    def _to_window(self, t):
        t = np.asarray(t, np.float64)
        return t - np.asarray(self.centre, np.float64)

    def _to_map(self, t):
        return np.asarray(t, np.float64) + np.asarray(self.centre, np.float64)

    def match(self, t_ga, t_nga, R, t):
        R, t, res = self.matcher.match(t_ga, t_nga, R, self._to_window(np.reshape(t, 2)))
        return R, self._to_map(t), res

    def match_post(self, t_ga, t_nga, R, t):
        R, t, res, post = self.matcher.match_post(t_ga, t_nga, R, self._to_window(np.reshape(t, 2)))
        return R, self._to_map(t), res, post

    def match_batch(self, batch, R0=None, t0=None):
        t0 = np.reshape(batch.t if t0 is None else t0, (batch.n_scans, 2))
        R, t, res = self.matcher.match_batch(batch, R0, self._to_window(t0))
        return R, self._to_map(t), res

    def score_poses(self, t_ga, t_nga, poses):
        """poses [P, 4] (cos, sin, tx, ty) in the map frame"""
        poses = np.array(poses, dtype=np.float64).reshape(-1, 4)
        poses[:, 2:] = self._to_window(poses[:, 2:])
        return self.matcher.score_poses(t_ga, t_nga, poses)

    def relocalize(self, t_ga, t_nga, theta_step):
        """No prior: the window covers the whole grid and all angles, the start is the window's centre.  (R, t, CsmResult)"""
        half_theta = int(np.ceil(np.pi / float(theta_step)))
        self.matcher.set_window(self.grid.size_x // 2, self.grid.size_y // 2, half_theta, theta_step)
        return self.match(t_ga, t_nga, np.eye(2), np.asarray(self.centre, np.float64))

    def particle_filter(self, n, params=None, **kw):
        """A ParticleFilter of n particles bound to this matcher: its update scores against the grid's plane, at the grid's
        resolution, and passes the rolling centre (docs/PARTICLE_FILTER.md)"""
        return ParticleFilter(n, params, matcher=self, **kw)

    def close(self):
        for o in (getattr(self, "matcher", None), getattr(self, "field", None)):
            if o is not None:
                o.close()
        self.matcher = self.field = None


def pf_default_params(**kw):
    return _defaults(PfParams, "slam_pf_default_params", kw)


def pf_angle_table(n_angles):
    """np.float64[2 n_angles]: cos, sin(2 pi k / n_angles), the quadrants exact (slam_pf_angle_table; host only)"""
    cs = np.zeros(2 * max(int(n_angles), 0), np.float64)
    check(lib().slam_pf_angle_table(int(n_angles), _ptr(cs), len(cs)))
    return cs


def pf_gauss_table(bits):
    """np.float64[2^bits]: the standard normal quantiles of (i + 1/2) / 2^bits (slam_pf_gauss_table; host only)"""
    G = np.zeros(1 << min(max(int(bits), 0), 20), np.float64)
    check(lib().slam_pf_gauss_table(int(bits), _ptr(G), len(G)))
    return G


def pf_weight_table(scale, shift, L):
    """np.uint32[L]: rint(65536 exp(-(j << shift) / scale)) (slam_pf_weight_table; host only)"""
    w = np.zeros(min(max(int(L), 1), 1 << 20), np.uint32)
    check(lib().slam_pf_weight_table(float(scale), int(shift), int(L), _ptr(w)))
    return w


class ParticleFilter(_Handle):
    """Monte Carlo localisation over a grid matcher (slam_pf_*, docs/PARTICLE_FILTER.md).  matcher: a GridMatcher (update
    then passes its rolling centre) or a CorrelativeMatcher (centre 0, 0), or None: update takes one."""
    _destroy = "slam_pf_destroy"

    def __init__(self, n=None, params=None, matcher=None, **kw):
        self.params = params or pf_default_params(**kw)
        if n is not None:
            self.params.n_particles = int(n)
        self.matcher = matcher
        h = _vp()
        check(lib().slam_pf_create(C.byref(self.params), C.byref(h)))
        self.h = h.value
        self.n = self.params.n_particles
        self._motion = None

    def tables(self):
        """the tables a filter of these parameters is created with: (cs, G, wtab)"""
        p = self.params
        return pf_angle_table(p.n_angles), pf_gauss_table(p.gauss_bits), pf_weight_table(p.weight_scale, p.weight_shift, p.weight_len)

    def set_tables(self, cs=None, G=None, wtab=None):
        cs = None if cs is None else np.ascontiguousarray(cs, np.float64).ravel()
        G = None if G is None else np.ascontiguousarray(G, np.float64).ravel()
        wtab = None if wtab is None else np.ascontiguousarray(wtab, np.uint32).ravel()
        check(lib().slam_pf_set_tables(self.h, *(v for a in (cs, G, wtab) for v in ((None, 0) if a is None else (a.ctypes.data_as(_vp), len(a))))))

    def set_particles(self, x, y, k):
        x, y, k = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64), np.ascontiguousarray(k, np.int32)
        assert len(x) == len(y) == len(k)
        check(lib().slam_pf_set_particles(self.h, _ptr(x), _ptr(y), _ptr(k), len(x)))

    def particles(self):
        """(x f64 [n], y f64 [n], k int32 [n])"""
        x, y, k = np.empty(self.n, np.float64), np.empty(self.n, np.float64), np.empty(self.n, np.int32)
        check(lib().slam_pf_read_particles(self.h, _ptr(x), _ptr(y), _ptr(k)))
        return x, y, k

    def weights(self):
        """(acc int64 [n], w uint32 [n]) as the last update left them"""
        acc, w = np.empty(self.n, np.int64), np.empty(self.n, np.uint32)
        check(lib().slam_pf_read_weights(self.h, _ptr(acc), _ptr(w)))
        return acc, w

    def state(self):
        s = PfState()
        check(lib().slam_pf_read_state(self.h, C.byref(s)))
        return s

    def random_words(self, p0, n, t, purpose):
        """[n, 4] uint32: the device's Philox words of counters (p0 + i, t, purpose, 0)"""
        d = DeviceArray((max(int(n), 1), 4), np.uint32)
        check(lib().slam_pf_random_words_dev(self.h, int(p0), int(n), int(t), int(purpose), d.ptr))
        return d.download()[:int(n)]

    def init_gaussian(self, x, y, k, sx, sy, sk):
        check(lib().slam_pf_init_gaussian(self.h, float(x), float(y), int(k), float(sx), float(sy), float(sk)))

    @staticmethod
    def motion(dx, dy, sx, sy, sk, dk):
        """one motion as a host array of PF_MOTION_DTYPE, ready for a device buffer"""
        return np.array([(float(dx), float(dy), float(sx), float(sy), float(sk), int(dk))], PF_MOTION_DTYPE)

    def predict(self, motion):
        """motion: (dx, dy, sx, sy, sk, dk); synchronous"""
        dx, dy, sx, sy, sk, dk = motion
        check(lib().slam_pf_predict(self.h, C.byref(PfMotion(float(dx), float(dy), float(sx), float(sy), float(sk), int(dk)))))

    def predict_dev(self, d_motion, stream=None):
        """d_motion: a device buffer holding one motion (PF_MOTION_DTYPE)"""
        at = getattr(d_motion, "ptr", d_motion)      # (a view of the device's bytes, never read here: cheaper per call than a cast)
        check(lib().slam_pf_predict_dev(self.h, PfMotion.from_address(at) if at else None, _sp(stream)))

    def _centre(self, matcher, centre):
        """(the CorrelativeMatcher, the window's centre): a GridMatcher brings its own centre, anything else has (0, 0)
        unless `centre` says otherwise"""
        m = matcher if matcher is not None else self.matcher
        if isinstance(m, GridMatcher):
            return m.matcher, (m.centre if centre is None else centre)
        return m, ((0.0, 0.0) if centre is None else centre)

    def update(self, t_ga, t_nga, matcher=None, centre=None):
        """slam_pf_update, host arrays; returns state()"""
        pts = np.ascontiguousarray(np.concatenate([np.reshape(t_ga, (-1, 2)), np.reshape(t_nga, (-1, 2))]), dtype=np.float64)
        m, c = self._centre(matcher, centre)
        check(lib().slam_pf_update(self.h, m.h, _ptr(pts), len(pts), len(np.reshape(t_ga, (-1, 2))), float(c[0]), float(c[1])))
        return self.state()

    def update_dev(self, d_pts, n, n_ga, matcher=None, centre=None, stream=None):
        m, c = self._centre(matcher, centre)
        check(lib().slam_pf_update_dev(self.h, m.h, getattr(d_pts, "ptr", d_pts), int(n), int(n_ga), float(c[0]), float(c[1]), _sp(stream)))

    def resample_indices(self, w, r, stream=None):
        """the resampling rule alone over uint32 weights (len(w) <= n): src int32 [len(w)]"""
        w = np.ascontiguousarray(w, np.uint32)
        d_w, d_src = DeviceArray.from_host(w), DeviceArray((len(w),), np.int32)
        check(lib().slam_pf_resample_indices_dev(self.h, d_w.ptr, len(w), int(r), d_src.ptr, _sp(stream)))
        if stream is not None:
            stream.synchronize()
        return d_src.download()


def mls_default_params(**kw):
    return _defaults(MlsParams, "slam_mls_default_params", kw)


def kf_default_params(**kw):
    return _defaults(KfParams, "slam_kf_default_params", kw)


def kf_gicp_default_params(**kw):
    return _defaults(KfGicpParams, "slam_kf_gicp_default_params", kw)


SC_MATCH_DTYPE = np.dtype([(f, np.int32) for f, _ in KfScMatch._fields_])


def kf_sc_default_params(**kw):
    return _defaults(KfScParams, "slam_kf_sc_default_params", kw)


class KeyframeStore(_Handle):
    """graph_slam's keyframes on the device (slam_kf_*): each one voxel-filtered once and indexed by a 3-D lattice; edges
    (calcEdgeIcp: 3-D point-to-point ICP, then computeEdgeInformationLUM) registered in batches."""
    _destroy = "slam_kf_destroy"

    def __init__(self, params=None, **kw):
        self.h = None
        p = params or kf_default_params(**kw)
        h = _vp()
        check(lib().slam_kf_create(C.byref(p), C.byref(h)))
        self.h = h.value
        self.params = p

    def __len__(self):
        return int(lib().slam_kf_count(self.h))

    def set_params(self, **kw):
        for k, v in kw.items():
            setattr(self.params, k, v)
        check(lib().slam_kf_set_params(self.h, C.byref(self.params)))

    def add_keyframe(self, xyz):
        """[n, >= 3] f32 cloud -> keyframe id."""
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        kid = C.c_int(-1)
        check(lib().slam_kf_add_keyframe(self.h, _ptr(a), len(a), a.shape[1] if a.ndim == 2 else 3, C.byref(kid)))
        return kid.value

    def add_keyframe_dev(self, d_xyz, n, stride=3, stream=None):
        kid = C.c_int(-1)
        check(lib().slam_kf_add_keyframe_dev(self.h, d_xyz.ptr, int(n), int(stride), C.byref(kid), _sp(stream)))
        return kid.value

    def remove_keyframe(self, kid):
        """Frees keyframe kid; the id is never issued again and every later call that names it raises E_INVALID."""
        check(lib().slam_kf_remove_keyframe(self.h, int(kid)))

    def replace_keyframe_dev(self, kid, d_xyz, n, stride=3, stream=None):
        """add_keyframe_dev's filter and lattice into the existing id; a refused cloud leaves the old keyframe."""
        check(lib().slam_kf_replace_keyframe_dev(self.h, int(kid), getattr(d_xyz, "ptr", d_xyz), int(n), int(stride), _sp(stream)))

    def replace_keyframe(self, kid, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        a = a.reshape(-1, a.shape[1] if a.ndim == 2 else 3)
        d = DeviceArray.from_host(a) if a.size else None
        self.replace_keyframe_dev(kid, d, len(a), a.shape[1])

    def info(self, kid):
        v = [C.c_int() for _ in range(4)]
        b = C.c_long()
        check(lib().slam_kf_keyframe_info(self.h, int(kid), *[C.byref(x) for x in v], C.byref(b)))
        return {"n_points": v[0].value, "n_cells": v[1].value, "max_cell_points": v[2].value, "table_slots": v[3].value,
                "device_bytes": b.value}

    def read_keyframe(self, kid):
        """The filtered cloud, [n, 4] f32 (x, y, z and the filter's fourth field)."""
        n = self.info(kid)["n_points"]
        out = np.zeros((n, 4), np.float32)
        got = C.c_int(0)
        check(lib().slam_kf_read_keyframe(self.h, int(kid), _ptr(out), n, C.byref(got)))
        return out[:got.value]

    def nearest(self, kid, queries, strict=False):
        """Gated 1-NN of [n, >= 3] f32 queries in keyframe kid: (index or -1, f32 squared distance)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        n = len(q)
        d_q = DeviceArray.from_host(q)
        d_i, d_d = DeviceArray((n,), np.int32), DeviceArray((n,), np.float32)
        check(lib().slam_kf_nearest_dev(self.h, int(kid), d_q.ptr, n, q.shape[1], int(bool(strict)), d_i.ptr, d_d.ptr, None))
        synchronize()
        return d_i.download(), d_d.download()

    def _register(self, plain, traced, result_type, to_dict, edges, trace, stream):
        """One batch through a solver's plain and traced entry points: a dict per request by to_dict."""
        n = len(edges)
        req = (KfEdgeReq * max(n, 1))()
        for e, (f, t, init) in enumerate(edges):
            req[e].from_, req[e].to = int(f), int(t)
            req[e].init[:] = np.asarray(init, dtype=np.float32).reshape(16).tolist()
        res = (result_type * max(n, 1))()
        tr = np.full((max(n, 1), max(trace, 1)), -1, np.int32)
        if trace > 0:
            check(traced(self.h, req, n, res, _ptr(tr), int(trace), _sp(stream)))
        else:
            check(plain(self.h, req, n, res, _sp(stream)))
        out = [to_dict(res[e]) for e in range(n)]
        if trace > 0:
            for e in range(n):
                out[e]["pairs_trace"] = tr[e].copy()
        return out

    def register_edges(self, edges, trace=0, stream=None):
        """edges: [(from, to, init 4x4), ...] -> list of dicts (one per edge; 'pairs_trace' when trace > 0)."""
        L = lib()
        return self._register(L.slam_kf_register_edges, L.slam_kf_register_edges_traced, KfEdgeResult, kf_result_dict, edges, trace, stream)

    # ---- Generalized ICP (docs/KF_GICP.md)
    def set_gicp_params(self, params=None, **kw):
        p = params or kf_gicp_default_params(**kw)
        check(lib().slam_kf_set_gicp_params(self.h, C.byref(p)))
        self.gicp_params = p

    def compute_covariances(self, kid, stream=None):
        """Per-point covariances of keyframe kid (a second call does nothing)."""
        check(lib().slam_kf_compute_covariances(self.h, int(kid), _sp(stream)))

    def covariances(self, kid):
        """[n, 6] f64: xx xy xz yy yz zz per point of the filtered cloud."""
        n = self.info(kid)["n_points"]
        out = np.zeros((n, 6), np.float64)
        got = C.c_int(0)
        check(lib().slam_kf_read_covariances(self.h, int(kid), _ptr(out), n, C.byref(got)))
        return out[:got.value]

    def neighbours(self, kid):
        """The lists the covariances were summed over: (index [n, k] i32, -1 behind the last; f32 d^2 [n, k]; count [n])."""
        n = self.info(kid)["n_points"]
        k = C.c_int(0)
        check(lib().slam_kf_read_neighbours(self.h, int(kid), None, None, None, 0, C.byref(k)))
        idx, d2 = np.zeros((n, k.value), np.int32), np.zeros((n, k.value), np.float32)
        cnt = np.zeros(n, np.int32)
        check(lib().slam_kf_read_neighbours(self.h, int(kid), _ptr(idx), _ptr(d2), _ptr(cnt), n, C.byref(k)))
        return idx, d2, cnt

    def register_gicp(self, edges, params=None, trace=0, stream=None):
        """edges: [(from, to, init 4x4), ...] -> list of dicts: the fields of register_edges plus 'cost', 'hessian',
        'fitness', 'fitness_pairs' ('pairs_trace' when trace > 0).  params: a KfGicpParams to set first."""
        if params is not None:
            self.set_gicp_params(params)
        L = lib()
        return self._register(L.slam_kf_register_gicp, L.slam_kf_register_gicp_traced, KfGicpResult, kf_gicp_result_dict, edges, trace, stream)

    # ---- scan-context descriptors and loop-closure candidates (docs/SCAN_CONTEXT.md)
    def set_sc_params(self, params=None, **kw):
        p = params or kf_sc_default_params(**kw)
        check(lib().slam_kf_set_sc_params(self.h, C.byref(p)))
        self.sc_params = p

    def sc_compute(self, kid=-1, stream=None):
        """The descriptor of keyframe kid; -1: of every live keyframe that has none, in one launch."""
        check(lib().slam_kf_sc_compute(self.h, int(kid), _sp(stream)))

    def sc_read(self, kid):
        """[n_rings, n_sectors] u8: 0 = empty cell, else 1 + the height bin of the cell's highest point."""
        r, s = C.c_int(0), C.c_int(0)
        check(lib().slam_kf_sc_read(self.h, int(kid), None, 0, C.byref(r), C.byref(s)))
        out = np.zeros((r.value, s.value), np.uint8)
        check(lib().slam_kf_sc_read(self.h, int(kid), _ptr(out), out.size, C.byref(r), C.byref(s)))
        return out

    def sc_tables(self):
        """(edge2 [n_rings], cos [n_sectors / 4], sin [n_sectors / 4]) f64: the tables the kernel bins by."""
        p = getattr(self, "sc_params", None) or kf_sc_default_params()
        e, c, s = np.zeros(p.n_rings), np.zeros(p.n_sectors // 4), np.zeros(p.n_sectors // 4)
        check(lib().slam_kf_sc_read_tables(self.h, _ptr(e), _ptr(c), _ptr(s)))
        return e, c, s

    def sc_match(self, queries, stream=None):
        """[len(queries), len(self)] record array (distance, shift, n_query, n_candidate, n_both); distance -1 for a
        removed keyframe and for the query itself."""
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        out = np.zeros((len(q), len(self)), SC_MATCH_DTYPE)
        check(lib().slam_kf_sc_match(self.h, _ptr(q), len(q), _as(KfScMatch, _ptr(out)), _sp(stream)))
        return out

    def loop_candidates(self, kid, k=3, min_gap=10, max_distance=None):
        """Up to k keyframes before kid - min_gap, nearest by descriptor first (ties by id): [(id, distance, shift, yaw)],
        yaw = -shift 2 pi / n_sectors wrapped to (-pi, pi], the rotation about z that seeds the registration
        (target = candidate, source = kid)."""
        m = self.sc_match([kid])[0]
        n_sectors = (getattr(self, "sc_params", None) or kf_sc_default_params()).n_sectors
        ids = [i for i in range(len(m)) if i < kid - min_gap and m["distance"][i] >= 0 and
               (max_distance is None or m["distance"][i] <= max_distance)]
        ids.sort(key=lambda i: (int(m["distance"][i]), i))
        out = []
        for i in ids[:k]:
            yaw = -int(m["shift"][i]) * 2.0 * np.pi / n_sectors
            out.append((i, int(m["distance"][i]), int(m["shift"][i]), yaw + 2.0 * np.pi if yaw <= -np.pi else yaw))
        return out


class Lcg:
    """x <- 1664525 x + 1013904223 mod 2^32; next() is the top 24 bits as a float32 in [0, 1): slam_amd::Lcg of
    include/slam_amd/global_match.hpp, so that C++ and Python draw the same starts."""

    def __init__(self, seed=1):
        self.state = int(seed) & 0xffffffff

    def next(self):
        self.state = (self.state * 1664525 + 1013904223) & 0xffffffff
        return np.float32(self.state >> 8) * np.float32(1.0 / 16777216.0)


def global_match_starts(random, cur_x, cur_y, cur_yaw, iterations=20, dist_rng=10.0, angle_rng=2 * math.pi):
    """[(dx, dy, dth)] as float32: start 0 is the current pose, the others are drawn around it (global_match.cpp:105-118)."""
    out = [(np.float32(cur_x), np.float32(cur_y), np.float32(cur_yaw))]
    for _ in range(1, iterations):
        dx = np.float32(float(random()) * 2.0 * dist_rng - dist_rng + float(np.float32(cur_x)))
        dy = np.float32(float(random()) * 2.0 * dist_rng - dist_rng + float(np.float32(cur_y)))
        dth = np.float32(float(random()) * angle_rng)
        out.append((dx, dy, dth))
    return out


class GlobalMatcher:
    """global_matching's matcher (global_match.cpp:72-235) over KeyframeStore.register_gicp: the same behaviour as
    slam_amd::GlobalMatcher of include/slam_amd/global_match.hpp, member for member (docs/KF_GICP.md section 4)."""

    def __init__(self, leaf=1.5, gate=10.0, refine_leaf=0.25, refine_gate=1.0, seed=1, random=None):
        self.MAX_SCORE, self.MAX_TRIES, self.ITERATIONS = 0.002, 50, 20
        self.GUESS_DIST_RNG, self.GUESS_ANGLE_RNG, self.COV_YAW, self.COV_XY = 10.0, 2 * math.pi, 100.0, 1000.0
        self.random = random or Lcg(seed).next
        self.try_count = 0
        self.coarse = KeyframeStore(leaf_size=leaf, gate=gate)
        self.refine = KeyframeStore(leaf_size=refine_leaf, gate=refine_gate)
        self.map_coarse = self.map_refine = -1
        self.last, self.last_starts = [], []

    def close(self):
        self.coarse.close()
        self.refine.close()

    def set_map(self, xyz):
        self.map_coarse, self.map_refine = self.coarse.add_keyframe(xyz), self.refine.add_keyframe(xyz)

    @staticmethod
    def planar(dx, dy, dth):
        c, s = np.float32(math.cos(float(dth))), np.float32(math.sin(float(dth)))
        return np.array([[c, -s, 0, dx], [s, c, 0, dy], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)

    def starts(self, cur_x, cur_y, cur_yaw):
        return global_match_starts(self.random, cur_x, cur_y, cur_yaw, self.ITERATIONS, self.GUESS_DIST_RNG, self.GUESS_ANGLE_RNG)

    def _edge(self, id_, x, y, theta, **kw):
        cov = np.zeros(9)
        cov[0] = cov[4] = self.COV_XY
        cov[8] = self.COV_YAW
        return dict(kw, to=int(id_), x=float(x), y=float(y), theta=float(theta), covariance=cov, **{"from": 0})

    def match(self, cloud, cur_x, cur_y, cur_yaw, id_=1):
        """laser_callback: the edge (a dict; 'matched' False for the fallback edge of :204-221) or None."""
        scan = self.coarse.add_keyframe(cloud)
        n_scan = self.coarse.info(scan)["n_points"]
        self.last_starts = self.starts(cur_x, cur_y, cur_yaw)
        self.last = self.coarse.register_gicp([(self.map_coarse, scan, self.planar(*s)) for s in self.last_starts])
        for i, r in enumerate(self.last):
            norm_score = r["fitness"] / float(n_scan)
            if not (r["converged"] and r["fitness_pairs"] > 0 and norm_score < self.MAX_SCORE):
                continue
            fine = self.refine.add_keyframe(cloud)
            rr = self.refine.register_gicp([(self.map_refine, fine, r["transform"])])[0]
            T = rr["transform"]
            self.try_count = 0
            return self._edge(id_, T[0, 3], T[1, 3], math.atan2(float(T[1, 0]), float(T[0, 0])), matched=True, start=i,
                              norm_score=norm_score, coarse=r["transform"], refined=T, coarse_result=r, refine_result=rr)
        self.try_count += 1
        if self.try_count >= self.MAX_TRIES:
            return self._edge(id_, np.float32(cur_x), np.float32(cur_y), np.float32(cur_yaw), matched=False, start=-1)
        return None


class GlobalMapBuilder:
    """global_matching's map builder (global_generate.cpp:122-232) over VoxelMap and KeyframeStore.register_gicp: the
    same behaviour as slam_amd::GlobalMapBuilder of include/slam_amd/map_builder.hpp, whose head lists how the names
    correspond (docs/VOXEL_MAP.md section 5 states the deviations from the reference).  An error of the library raises
    SlamError here (C++ prints it and rejects the cloud); the scan keyframe is removed on every way out."""

    DIST_LEAF = 1.0     # leaf of the map that direct mode registers against (docs/VOXEL_MAP.md section 9)

    def __init__(self, leaf=0.30, gate=2.0, carve=False, direct=False):
        # global_generate.cpp:21-29, :84-90: macros and setup_gicp's values there, members here.  The store and the map are made
        # with the fixed ones (read-only properties below); MAX_SCORE and CROP_DIST are read at every add_cloud
        self._fixed = dict(LEAF_SIZE=float(leaf), gate=float(gate), MAX_ITERATIONS=100, TRANSFORMATION_EPSILON=1e-6,
                           FITNESS_EPSILON=1e-6, MAX_DIST=4.0, carve=bool(carve), direct=bool(direct))
        self.MAX_SCORE, self.CROP_DIST = 1.0, 100.0
        # free-space carving (docs/VOXEL_MAP.md section 8): the switch is fixed here, the rest is read at every call
        self.CARVE_NUM, self.CARVE_DEN = 1, 1
        self.carve_params = vmap_default_carve_params()
        self.last_carve = None  # the counters of the last accepted cloud's carve
        self.vmap = VoxelMap(leaf=self.LEAF_SIZE)
        self.store = KeyframeStore(leaf_size=self.LEAF_SIZE, gate=self.gate, transformation_epsilon=self.TRANSFORMATION_EPSILON,
                                   fitness_epsilon=self.FITNESS_EPSILON)
        self.store.set_gicp_params(max_iterations=self.MAX_ITERATIONS, transformation_epsilon=self.TRANSFORMATION_EPSILON)
        # direct mode (section 9): a second map of leaf DIST_LEAF with distributions, registered against without extraction;
        # fixed here like carve.  The carved rule is part of its plane rule when carve is on (CARVE_NUM / CARVE_DEN as they
        # stand now: the distributions' parameters are fixed with the map)
        self.dmap = None
        if self.direct:
            self.dmap = VoxelMap(leaf=self.DIST_LEAF)
            self.dmap.enable_distributions(max_miss_num=self.CARVE_NUM if self.carve else 0, max_miss_den=self.CARVE_DEN if self.carve else 0)
        self.trans_full = np.eye(4, dtype=np.float32)
        self.map_id, self.n_clouds, self.n_accepted = -1, 0, 0
        self.last = None        # the last request's result

    def close(self):
        self.vmap.close()
        if self.dmap is not None:
            self.dmap.close()
        self.store.close()

    LEAF_SIZE = property(lambda self: self._fixed["LEAF_SIZE"])
    gate = property(lambda self: self._fixed["gate"])
    MAX_ITERATIONS = property(lambda self: self._fixed["MAX_ITERATIONS"])
    TRANSFORMATION_EPSILON = property(lambda self: self._fixed["TRANSFORMATION_EPSILON"])
    FITNESS_EPSILON = property(lambda self: self._fixed["FITNESS_EPSILON"])
    MAX_DIST = property(lambda self: self._fixed["MAX_DIST"])    # kept for the name, without effect: the store's gate rules
    carve = property(lambda self: self._fixed["carve"])
    direct = property(lambda self: self._fixed["direct"])

    def _maps(self):
        return (self.vmap,) if self.dmap is None else (self.vmap, self.dmap)

    def _max_miss(self):
        return (self.CARVE_NUM, self.CARVE_DEN) if self.carve else None

    def pose(self):
        """trans_full: the accumulated transform of the last accepted cloud, 4 x 4 f32."""
        return self.trans_full.copy()

    def crop_box(self):
        """(lo_xy, hi_xy) of :149-157 as f32: -+CROP_DIST + trans_full(i, 3) in double, rounded once"""
        c = [float(self.trans_full[0, 3]), float(self.trans_full[1, 3])]
        return (np.array([-self.CROP_DIST + c[0], -self.CROP_DIST + c[1]], np.float32),
                np.array([self.CROP_DIST + c[0], self.CROP_DIST + c[1]], np.float32))

    def map(self):
        """The whole map as GlobalMatcher.set_map takes it: [n, 4] f32 (x, y, z, 0) in key order (the carved extraction
        when carve is on)."""
        return self.vmap.read(max_miss=self._max_miss())[0]

    def save(self, prefix):
        """The builder's state into prefix.vmap (the map), prefix.dmap (the second map, with `direct`) and prefix.pose
        (trans_full as 16 little-endian floats, then n_clouds and n_accepted as i32): docs/VOXEL_MAP.md section 10.5."""
        prefix = os.fspath(prefix)
        self.vmap.save(prefix + ".vmap")
        if self.dmap is not None:
            self.dmap.save(prefix + ".dmap")
        with open(prefix + ".pose", "wb") as f:
            f.write(np.ascontiguousarray(self.trans_full, dtype="<f4").tobytes())
            f.write(np.array([self.n_clouds, self.n_accepted], "<i4").tobytes())

    def resume(self, prefix):
        """Takes up what save(prefix) left: legal only before the first add_cloud, and only when the files' leaves, carve
        state and distribution parameters are those of this builder's construction (SlamError otherwise, nothing changed).
        The maps are loaded by slam_vmap_load and take the place of the builder's own empty ones."""
        prefix = os.fspath(prefix)
        if self.n_clouds != 0:
            raise SlamError(E_INVALID, "GlobalMapBuilder.resume: legal only on a builder that has added no cloud")
        if not self.direct and os.path.exists(prefix + ".dmap"):
            raise SlamError(E_INVALID, "GlobalMapBuilder.resume: %s.dmap exists: saved by a direct builder, this one is not" % prefix)
        try:
            pose = open(prefix + ".pose", "rb").read()
        except OSError as e:
            raise SlamError(E_IO, "GlobalMapBuilder.resume: %s" % e)
        if len(pose) != 72:
            raise SlamError(E_INVALID, "GlobalMapBuilder.resume: %s.pose holds %d bytes, not 72" % (prefix, len(pose)))
        loaded = []
        try:
            for ext, own in ((".vmap", self.vmap), (".dmap", self.dmap)):
                if own is None:
                    continue
                m = VoxelMap.load(prefix + ext)
                loaded.append(m)
                a, b = m.layout(), own.layout()
                same = (np.float64(a["leaf"]).tobytes() == np.float64(b["leaf"]).tobytes() and a["carved"] == self.carve
                        and a["distributions"] == b["distributions"]
                        and all(getattr(a["dist_params"], f) == getattr(b["dist_params"], f) for f, _ in VmapDistParams._fields_))
                if not same:
                    raise SlamError(E_INVALID, "GlobalMapBuilder.resume: %s%s was saved with another leaf, carve state or "
                                               "distribution parameters than this builder has" % (prefix, ext))
        except SlamError:
            for m in loaded:
                m.close()
            raise
        for m in self._maps():
            m.close()
        self.vmap = loaded[0]
        self.dmap = loaded[1] if self.direct else None
        self.trans_full = np.frombuffer(pose[:64], "<f4").astype(np.float32).reshape(4, 4).copy()
        self.n_clouds, self.n_accepted = (int(v) for v in np.frombuffer(pose[64:], "<i4"))

    def add_cloud(self, xyz):
        """One scan ([n, >= 3] f32, sensor frame): (accepted, result dict of register_gicp or None for the first cloud).
        With `direct` the result is VoxelMap.register_gicp's: its fitness is the point-to-plane score."""
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        a = a.reshape(-1, a.shape[1] if a.ndim == 2 else 3)
        self.n_clouds += 1
        if self.vmap.info()["n_points"] == 0:      # :63-70: the first cloud is the map
            for m in self._maps():
                m.integrate(a)
            if self.carve:
                self.last_carve = self.vmap.carve(a, params=self.carve_params)
                if self.dmap is not None:
                    self.dmap.carve(a, params=self.carve_params)
            self.n_accepted += 1
            self.last = None
            return True, None
        d_scan = DeviceArray.from_host(a)
        scan = self.store.add_keyframe_dev(d_scan, len(a), a.shape[1])
        try:
            if self.direct:                        # section 9: the scan against the plane voxels of the 1 m map, nothing extracted
                r = self.dmap.register_gicp(self.store, scan, self.trans_full, gate=self.gate, max_iterations=self.MAX_ITERATIONS,
                                            transformation_epsilon=self.TRANSFORMATION_EPSILON)
            else:
                lo, hi = self.crop_box()
                cap = max(self.vmap.info()["n_voxels"], 1)
                d_map = DeviceArray((cap, 4), np.float32)
                n_map = self.vmap.extract_dev(d_map, cap, lo=lo, hi=hi, max_miss=self._max_miss())
                synchronize()
                if n_map == 0:                         # nothing of the map near the pose: nothing to register against
                    self.last = None
                    return False, None
                if self.map_id < 0:
                    self.map_id = self.store.add_keyframe_dev(d_map, n_map, 4)
                else:
                    self.store.replace_keyframe_dev(self.map_id, d_map, n_map, 4)
                r = self.store.register_gicp([(self.map_id, scan, self.trans_full)])[0]
            self.last = r
            if r["fitness_pairs"] <= 0 or not r["converged"] or r["fitness"] > self.MAX_SCORE:      # :182
                return False, r
            self.trans_full = np.array(r["transform"], np.float32).reshape(4, 4)
            T = self.trans_full.astype(np.float64)
            for m in self._maps():
                m.integrate_dev(d_scan, len(a), a.shape[1], R=T[:3, :3], t=T[:3, 3])
            if self.carve:
                self.last_carve = self.vmap.carve_dev(d_scan, len(a), a.shape[1], R=T[:3, :3], t=T[:3, 3], params=self.carve_params)
                if self.dmap is not None:
                    self.dmap.carve_dev(d_scan, len(a), a.shape[1], R=T[:3, :3], t=T[:3, 3], params=self.carve_params)
            self.n_accepted += 1
            return True, r
        finally:
            self.store.remove_keyframe(scan)


class MapLocalizer:
    """Relocalises a scan in a voxel map with distributions by registering a set of starts down the map's own exact coarser
    levels, one slam_vmap_register_gicp call per level (docs/VOXEL_MAP.md section 11.3): the same behaviour as
    slam_amd::MapLocalizer of include/slam_amd/global_match.hpp, member for member.  Level k is a map of leaf
    ldexp(leaf, k) filled by slam_vmap_coarsen from level k - 1; level 0 is the map itself.  No random numbers.  An error
    of the library and a map the localiser cannot take raise SlamError here (C++ prints and returns false); the scan
    keyframe is removed on every way out."""

    # read at every call: set on the instance to change
    GATE_RATIO, N_YAW, MIN_PAIR_SHARE = 2.0, 8, 0.5
    MAX_SCORE = 0.03        # between the two level-0 fitness populations of section 11.3: sqrt(0.00745 * 0.0964)
    # relocalize's (section 13.4): the level searched and descended from, the rotations scored and the hits taken as starts
    SEARCH_LEVEL, SEARCH_YAWS, SEARCH_STARTS = 1, 64, 4

    def __init__(self, levels=4, leaf=0.30):
        # fixed at construction: the number of levels, and the store with the builder's leaf and epsilons
        self._fixed = dict(LEVELS=int(levels), LEAF_SIZE=float(leaf), MAX_ITERATIONS=100, TRANSFORMATION_EPSILON=1e-6, FITNESS_EPSILON=1e-6)
        if self.LEVELS < 1:
            raise SlamError(E_INVALID, "MapLocalizer: LEVELS must be at least 1")
        self.store = KeyframeStore(leaf_size=self.LEAF_SIZE, gate=2.0, transformation_epsilon=self.TRANSFORMATION_EPSILON,
                                   fitness_epsilon=self.FITNESS_EPSILON)
        self.store.set_gicp_params(max_iterations=self.MAX_ITERATIONS, transformation_epsilon=self.TRANSFORMATION_EPSILON)
        self.fine, self.owned = None, False
        self.coarse = []        # levels 1 .. LEVELS - 1, owned
        self.last, self.n_source = [], 0

    LEVELS = property(lambda self: self._fixed["LEVELS"])
    LEAF_SIZE = property(lambda self: self._fixed["LEAF_SIZE"])
    MAX_ITERATIONS = property(lambda self: self._fixed["MAX_ITERATIONS"])
    TRANSFORMATION_EPSILON = property(lambda self: self._fixed["TRANSFORMATION_EPSILON"])
    FITNESS_EPSILON = property(lambda self: self._fixed["FITNESS_EPSILON"])

    def _drop_map(self):
        for m in self.coarse:
            m.close()
        self.coarse = []
        if self.owned and self.fine is not None:
            self.fine.close()
        self.fine, self.owned = None, False

    def close(self):
        self._drop_map()
        self.store.close()

    def level(self, k):
        """the map of level k: 0 is the fine map, k >= 1 the derived ones"""
        return self.fine if k == 0 else self.coarse[k - 1]

    def _take(self, fine, owned):
        lay = fine.layout()
        if not lay["distributions"]:
            raise SlamError(E_INVALID, "MapLocalizer: the map has no distributions")
        if not math.ldexp(lay["leaf"], self.LEVELS - 1) <= 8.0:
            raise SlamError(E_INVALID, "MapLocalizer: leaf %g times 2^%d is more than the 8 m a map with distributions may have"
                            % (lay["leaf"], self.LEVELS - 1))
        coarse = []
        try:
            below = fine
            for k in range(1, self.LEVELS):
                m = VoxelMap(leaf=math.ldexp(lay["leaf"], k))
                coarse.append(m)
                m.enable_distributions(params=lay["dist_params"])
                m.coarsen(below)
                below = m
        except SlamError:
            for m in coarse:
                m.close()
            raise
        self._drop_map()
        self.fine, self.owned, self.coarse = fine, owned, coarse

    def set_map(self, fine):
        """The fine map (a VoxelMap with distributions, borrowed: the caller keeps and closes it) and its derived levels."""
        self._take(fine, False)

    def load(self, path):
        """The fine map from a file of slam_vmap_save (owned) and its derived levels."""
        fine = VoxelMap.load(path)
        try:
            self._take(fine, True)
        except SlamError:
            fine.close()
            raise

    def rebuild(self):
        """Clears and refills the derived levels, after the fine map has grown."""
        if self.fine is None:
            raise SlamError(E_INVALID, "MapLocalizer.rebuild: no map")
        below = self.fine
        for m in self.coarse:
            m.clear()
            m.coarsen(below)
            below = m

    @staticmethod
    def yaw_fan(x, y, yaw, n):
        """n planar starts at (x, y) with yaws (float)((double) yaw + 2 pi k / n), each GlobalMatcher.planar's matrix."""
        return [GlobalMatcher.planar(np.float32(x), np.float32(y), np.float32(float(np.float32(yaw)) + 2.0 * math.pi * k / n))
                for k in range(int(n))]

    def search(self, cloud, params=None, level=None, **kw):
        """The scan becomes a keyframe, as in localize, and VoxelMap.search scores it against the derived level `level` (None:
        SEARCH_LEVEL): the hits, best first."""
        if self.fine is None:
            raise SlamError(E_INVALID, "MapLocalizer.search: no map")
        level = self.SEARCH_LEVEL if level is None else int(level)
        if not 0 <= level < self.LEVELS:
            raise SlamError(E_INVALID, "MapLocalizer.search: level %d of %d" % (level, self.LEVELS))
        scan = self.store.add_keyframe(cloud)
        try:
            return self.level(level).search(store=self.store, kid=scan, params=params, **kw)[0]
        finally:
            self.store.remove_keyframe(scan)

    def relocalize(self, cloud, cx=0.0, cy=0.0, cz=0.0, radius=24.0):
        """The cold start: no yaw and no position closer than `radius` metres around (cx, cy) is asked for.  SEARCH_YAWS
        rotations over the full circle and every offset of ceil(radius / leaf) cells in x and y (none in z) are scored at level
        SEARCH_LEVEL, the SEARCH_STARTS best hits' `init` are the starts, and localize descends from that level.  localize's
        dict with 'hits' added; found is False when there is no hit."""
        if self.fine is None:
            raise SlamError(E_INVALID, "MapLocalizer.relocalize: no map")
        if not 0 <= self.SEARCH_LEVEL < self.LEVELS:
            raise SlamError(E_INVALID, "MapLocalizer.relocalize: SEARCH_LEVEL %d of %d levels" % (self.SEARCH_LEVEL, self.LEVELS))
        w = int(math.ceil(float(radius) / self.level(self.SEARCH_LEVEL).params.leaf))
        hits = self.search(cloud, n_yaw=self.SEARCH_YAWS, top_m=self.SEARCH_STARTS, cx=cx, cy=cy, cz=cz, wx=w, wy=w, wz=0)
        if not hits:
            self.last, self.n_source = [[] for _ in range(self.LEVELS)], 0
            return dict(found=False, index=-1, transform=None, transform64=None, x=0.0, y=0.0, theta=0.0, n_source=0, last=self.last,
                        hits=hits)
        out = self.localize(cloud, [h["init"] for h in hits], from_level=self.SEARCH_LEVEL)
        out["hits"] = hits
        return out

    def localize(self, cloud, starts=None, x=0.0, y=0.0, yaw=0.0, from_level=None):
        """One scan ([n, >= 3] f32, sensor frame) from `starts` (4 x 4 f32 each; None: yaw_fan(x, y, yaw, N_YAW)).  From the
        coarsest level (from_level, where given: the levels above it are not run) down one register_gicp call carries every live start, gated at GATE_RATIO times the level's leaf, from
        the level above's f32 transform; a start that ends a level without pairs or degenerate is out.  The winner among the
        level-0 results that converged with fitness <= MAX_SCORE and fitness_pairs >= MIN_PAIR_SHARE n_source has the most
        fitness_pairs, then the lowest index.  A dict of found, index (-1: nobody), transform, transform64, x, y, theta (of
        the f32 transform, as GlobalMatcher fills its edge), n_source and last[level][start] (None where a start was out)."""
        if self.fine is None:
            raise SlamError(E_INVALID, "MapLocalizer.localize: no map")
        if starts is None:
            starts = self.yaw_fan(x, y, yaw, self.N_YAW)
        top = self.LEVELS - 1 if from_level is None else int(from_level)
        if not 0 <= top < self.LEVELS:
            raise SlamError(E_INVALID, "MapLocalizer.localize: from_level %d of %d levels" % (top, self.LEVELS))
        T = [np.array(s, np.float32).reshape(4, 4) for s in starts]
        scan = self.store.add_keyframe(cloud)
        try:
            self.n_source = self.store.info(scan)["n_points"]
            alive = [True] * len(T)
            self.last = [[None] * len(T) for _ in range(self.LEVELS)]
            for k in range(top, -1, -1):
                ids = [i for i in range(len(T)) if alive[i]]
                if not ids:
                    break
                m = self.level(k)
                res = m.register_gicp(self.store, [(scan, T[i]) for i in ids], gate=self.GATE_RATIO * m.params.leaf,
                                      max_iterations=self.MAX_ITERATIONS, transformation_epsilon=self.TRANSFORMATION_EPSILON)
                for i, r in zip(ids, res):
                    self.last[k][i] = r
                    if r["state"] in (KF_NO_CORRESPONDENCES, KF_DEGENERATE):
                        alive[i] = False
                    else:
                        T[i] = r["transform"]
        finally:
            self.store.remove_keyframe(scan)
        best = -1
        for i, r in enumerate(self.last[0]):
            if r is None or not alive[i] or not r["converged"] or not r["fitness"] <= self.MAX_SCORE:
                continue
            if not r["fitness_pairs"] >= self.MIN_PAIR_SHARE * self.n_source:
                continue
            if best < 0 or r["fitness_pairs"] > self.last[0][best]["fitness_pairs"]:
                best = i
        out = dict(found=best >= 0, index=best, transform=None, transform64=None, x=0.0, y=0.0, theta=0.0, n_source=self.n_source,
                   last=self.last)
        if best >= 0:
            w = self.last[0][best]
            Tw = w["transform"]
            out.update(transform=Tw, transform64=w["transform64"], x=float(Tw[0, 3]), y=float(Tw[1, 3]),
                       theta=math.atan2(float(Tw[1, 0]), float(Tw[0, 0])))
        return out


def kf_gicp_result_dict(r):
    d = kf_result_dict(r.edge)
    d.update(cost=r.cost, hessian=np.array(r.hessian[:], np.float64).reshape(6, 6), fitness=r.fitness,
             fitness_pairs=r.fitness_pairs)
    return d


def kf_result_dict(r):
    return {"transform": np.array(r.transform[:], np.float32).reshape(4, 4),
            "transform64": np.array(r.transform64[:], np.float64).reshape(4, 4), "iterations": r.iterations, "state": r.state,
            "converged": r.converged, "pairs": r.pairs, "mse": r.mse,
            "information": np.array(r.information[:], np.float64).reshape(6, 6), "num_corr": r.num_corr,
            "singular": r.singular, "ss": np.float32(r.ss)}


class MlsMap(_Handle):
    """The height-cluster MLS map (class MLS, non-rolling: mls.h:154-237) over the C-ABI: graph_slam's global map."""
    _destroy = "slam_mls_destroy"

    def __init__(self, size_x, size_y, resolution, params=None, **kw):
        self.size_x, self.size_y, self.resolution = int(size_x), int(size_y), float(resolution)
        p = params or mls_default_params(**kw)
        h = _vp()
        check(lib().slam_mls_create(self.size_x, self.size_y, self.resolution, C.byref(p), C.byref(h)))
        self.h = h.value
        self.cells = self.size_x * self.size_y
        self.capacity = self.info()["capacity"]

    def info(self):
        sx, sy, cap, pend = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        res = C.c_double()
        p = MlsParams()
        check(lib().slam_mls_info(self.h, C.byref(sx), C.byref(sy), C.byref(res), C.byref(cap), C.byref(p), C.byref(pend)))
        return {"size_x": sx.value, "size_y": sy.value, "resolution": res.value, "capacity": cap.value, "params": p,
                "pending_points": pend.value}

    @property
    def params(self):
        return self.info()["params"]

    def set_params(self, **kw):
        p = self.params
        for k, v in kw.items():
            setattr(p, k, v)
        check(lib().slam_mls_set_params(self.h, C.byref(p)))

    def clear(self, stream=None):
        check(lib().slam_mls_clear(self.h, _sp(stream)))

    def set_pose(self, x, y):
        check(lib().slam_mls_set_pose(self.h, float(x), float(y)))

    def add_cloud(self, xyz, pose=None):
        """MLS::addToMap(cloud[, pose]) with the cloud already in the map frame; pose = (x, y) sets the pose first."""
        if pose is not None:
            self.set_pose(pose[0], pose[1])
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        if a.ndim == 1:
            a = a.reshape(-1, 3)
        check(lib().slam_mls_add_cloud(self.h, _ptr(a), len(a), a.shape[1] if a.size else 3))

    def add_cloud_dev(self, d_xyz, n, stride=3, stream=None):
        check(lib().slam_mls_add_cloud_dev(self.h, d_xyz.ptr, int(n), int(stride), _sp(stream)))

    def offset_z(self, dz, stream=None):
        check(lib().slam_mls_offset_z(self.h, float(dz), _sp(stream)))

    def read_drivability(self):
        out = np.empty(self.cells, np.int8)
        check(lib().slam_mls_read_drivability(self.h, _ptr(out)))
        return out

    def segmented_clouds(self):
        """(obstacle, ground) float32 [n, 3] in MLS::getSegmentedClouds' order."""
        no, ng = C.c_int(), C.c_int()
        rc = lib().slam_mls_segmented_clouds(self.h, None, 0, C.byref(no), None, 0, C.byref(ng))
        if rc not in (SLAM_OK, E_NOMEM):
            check(rc)
        obs, gnd = np.empty((no.value, 3), np.float32), np.empty((ng.value, 3), np.float32)
        check(lib().slam_mls_segmented_clouds(self.h, _ptr(obs), len(obs), C.byref(no), _ptr(gnd), len(gnd), C.byref(ng)))
        return obs, gnd

    def read_cells(self, cells, clusters=True):
        """dict of per-cell arrays: n_clusters, clusters [n, capacity, 5] (mean x, y, z, cov_zz, num_pts; None without
        clusters), drivable, byte, updated, pending"""
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        n = len(cells)
        out = {"n_clusters": np.zeros(n, np.int32), "clusters": np.zeros((n, self.capacity, 5)) if clusters else None,
               "drivable": np.zeros(n, np.int8), "byte": np.zeros(n, np.int8), "updated": np.zeros(n, np.uint8),
               "pending": np.zeros(n, np.int32)}
        check(lib().slam_mls_read_cells(self.h, _ptr(cells), n, _ptr(out["n_clusters"]), _ptr(out["clusters"]),
                                        _ptr(out["drivable"]), _ptr(out["byte"]), _ptr(out["updated"]), _ptr(out["pending"])))
        return out


class Mapper(_Handle):
    """slam_mapper_t: the streaming form of the path (BASELINE config 5).  push() copies a chunk of a ScanBatch into
    the next slot's pinned buffers and enqueues it; wait() returns its registered poses."""
    _destroy = "slam_mapper_destroy"

    def __init__(self, m_ga, m_nga, grid=None, icp=None, **kw):
        p = _defaults(MapperParams, "slam_mapper_default_params", kw)
        for k, v in (grid or {}).items():
            setattr(p.grid, k, v)
        for k, v in (icp or {}).items():
            setattr(p.icp, k, v)
        self.params = p
        m_ga = np.ascontiguousarray(m_ga, dtype=np.float64).reshape(-1, 2)
        m_nga = np.ascontiguousarray(m_nga, dtype=np.float64).reshape(-1, 2)
        h = _vp()
        check(lib().slam_mapper_create(C.byref(p), _ptr(m_ga), len(m_ga), _ptr(m_nga), len(m_nga), C.byref(h)))
        self.h = h.value
        self._views = {}
        ns = C.c_int()
        check(lib().slam_mapper_slots(self.h, C.byref(ns)))
        self.n_slots = ns.value
        g = _vp()
        check(lib().slam_mapper_grid(self.h, C.byref(g)))
        self.grid = object.__new__(Grid)
        self.grid.h, self.grid.size_x, self.grid.size_y = g.value, p.grid_size_x, p.grid_size_y
        self.grid.resolution, self.grid.cells, self.grid.params = p.resolution, p.grid_size_x * p.grid_size_y, p.grid
        self.grid.close = lambda: None      # owned by the mapper

    def _slot_views(self, slot):
        if slot not in self._views:
            ptrs = [_vp() for _ in range(5)]
            check(lib().slam_mapper_chunk_buffers(self.h, slot, *[C.byref(x) for x in ptrs]))
            ns, npts = self.params.max_scans, self.params.max_points

            def view(ptr, count, dtype):
                buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value)
                return np.frombuffer(buf, dtype=dtype, count=count)
            self._views[slot] = (view(ptrs[0], 2 * npts, np.float64), view(ptrs[1], ns + 1, np.int32),
                                 view(ptrs[2], ns, np.int32), view(ptrs[3], 4 * ns, np.float64),
                                 view(ptrs[4], 2 * ns, np.float64))
        return self._views[slot]

    def push(self, batch, window_xy=(0.0, 0.0)):
        """batch: a synth.ScanBatch (scan_off from 0).  Returns the slot."""
        slot = C.c_int()
        check(lib().slam_mapper_next_slot(self.h, C.byref(slot)))
        pts, off, nga, R, t = self._slot_views(slot.value)
        S, P = batch.n_scans, batch.n_points
        pts[:2 * P] = batch.pts.reshape(-1)
        off[:S + 1] = batch.scan_off
        nga[:S] = batch.scan_nga
        R[:4 * S] = batch.R.reshape(-1)
        t[:2 * S] = batch.t.reshape(-1)
        out = C.c_int()
        check(lib().slam_mapper_push(self.h, S, P, float(window_xy[0]), float(window_xy[1]), C.byref(out)))
        self._n = getattr(self, "_n", {})
        self._n[out.value] = S
        return out.value

    def wait(self, slot):
        S = self._n.get(slot, 0)
        R, t = np.zeros((S, 4)), np.zeros((S, 2))
        check(lib().slam_mapper_wait(self.h, int(slot), _ptr(R), _ptr(t)))
        return R, t

    def finish(self):
        check(lib().slam_mapper_finish(self.h))

    def stats(self):
        c, m, r = C.c_long(), C.c_long(), C.c_long()
        ms, rows = C.c_double(), (C.c_int * 2)()
        check(lib().slam_mapper_stats(self.h, C.byref(c), C.byref(m), C.byref(r), C.byref(ms), rows))
        return dict(chunks=c.value, merges=m.value, rebuilds=r.value, rebuild_ms=ms.value, last_merge_rows=(rows[0], rows[1]))

    def _with_target(self, read):
        """read(icp) on the current target, borrowed from the mapper: the handle is not closed here"""
        h = _vp()
        check(lib().slam_mapper_target(self.h, C.byref(h)))
        icp = object.__new__(Icp)
        icp.h = h.value
        try:
            return read(icp)
        finally:
            icp.h = None

    def target_index_info(self):
        def read(icp):
            info = icp.index_info()
            info["built_on_device"], info["build_host_ms"] = icp.build_info()
            return info
        return self._with_target(read)

    def target_model(self):
        """The current target's points as its index holds them: (ga[n,2] f32, nga[m,2] f32), each in original order."""
        return self._with_target(lambda icp: (icp.read_model(0), icp.read_model(1)))

    def target_index_blobs(self):
        """The current target's cell index and halo lists as they lie in HBM (Icp.index_blob 0 and 1)."""
        return self._with_target(lambda icp: (icp.index_blob(0), icp.index_blob(1)))

    def use_comm(self, comm):
        check(rccl_lib().slam_mapper_use_comm(self.h, comm.h))
        self._comm = comm


class GroundSegmentation(_Handle):
    """groundSegmentation-shaped handle (groundSegmentation.h:67-128) over the C-ABI."""
    _destroy = "slam_gseg_destroy"

    def __init__(self, **kw):
        self.params = _defaults(GsegParams, "slam_gseg_default_params", kw)
        h = _vp()
        check(lib().slam_gseg_create(C.byref(self.params), C.byref(h)))
        self.h = h.value

    def segment(self, xyz):
        """setupGroundSegmentation + segmentGround: one GSEG_* label per point."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = xyz.shape
        labels = np.zeros(max(n, 1), dtype=np.uint8)
        check(lib().slam_gseg_segment(self.h, _ptr(xyz), n, stride, _ptr(labels)))
        return labels[:n]

    def segment_dev(self, d_xyz, n, stride, d_labels, stream=None):
        check(lib().slam_gseg_segment_dev(self.h, d_xyz.ptr, int(n), int(stride), d_labels.ptr, _sp(stream)))

    def split_dev(self, d_xyz, n, stride, d_labels, d_ground, d_obstacle, d_counts, stream=None):
        check(lib().slam_gseg_split_dev(self.h, d_xyz.ptr, int(n), int(stride), d_labels.ptr, d_ground.ptr,
                                        d_obstacle.ptr, d_counts.ptr, _sp(stream)))

    def classify_ga(self, obstacle_xyz):
        """CCICP::classifyPoints over an obstacle cloud (host arrays): flags 1 GA / 0 NGA / 255 dropped."""
        xyz = np.ascontiguousarray(obstacle_xyz, dtype=np.float32)
        n, stride = xyz.shape
        if n == 0:
            return np.zeros(0, np.uint8)
        d_xyz = DeviceArray.from_host(xyz)
        d_f = DeviceArray((n,), np.uint8)
        check(lib().slam_gseg_classify_ga_dev(self.h, d_xyz.ptr, n, stride, d_f.ptr, None))
        synchronize()
        return d_f.download()

    def read_model(self):
        state = np.zeros(72 * 200, dtype=np.uint8)
        value = np.zeros(72 * 200)
        iters = np.zeros(72, dtype=np.int32)
        check(lib().slam_gseg_read_model(self.h, _ptr(state), _ptr(value), _ptr(iters)))
        return state, value, iters


class Ccicp(_Handle):
    """The CCICP facade steps either side of the ICP (icpTools.cpp:222-381, 611-634) over the C-ABI."""
    _destroy = "slam_ccicp_destroy"
    ICP_MAX_PTS = 20000  # icpTools.h:21

    def __init__(self):
        h = _vp()
        check(lib().slam_ccicp_create(C.byref(h)))
        self.h = h.value

    def voxel_downsample(self, xyz, flags=None, leaf=(0.5, 0.5, 2.0)):
        """pcl::VoxelGrid as setSceneCloud uses it; returns [n_out, 4] = centroid x,y,z, ground_adj."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = xyz.shape
        if n == 0:
            return np.zeros((0, 4), np.float32)
        d_xyz = DeviceArray.from_host(xyz)
        d_flag = DeviceArray.from_host(np.ascontiguousarray(flags, np.uint8)) if flags is not None else None
        d_out = DeviceArray((n, 4), np.float32)
        n_out = C.c_int(0)
        check(lib().slam_ccicp_voxel_downsample_dev(self.h, d_xyz.ptr, d_flag.ptr if d_flag else None, n, stride,
                                                    leaf[0], leaf[1], leaf[2], d_out.ptr, n, C.byref(n_out), None))
        return d_out.download()[:n_out.value]

    def bin_order(self, xyz, flags):
        """The cloud in classifyPoints order with its flags: [n_kept, 4]."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = xyz.shape
        if n == 0:
            return np.zeros((0, 4), np.float32)
        d_xyz = DeviceArray.from_host(xyz)
        d_flag = DeviceArray.from_host(np.ascontiguousarray(flags, np.uint8))
        d_out = DeviceArray((n, 4), np.float32)
        n_out = C.c_int(0)
        check(lib().slam_ccicp_bin_order_dev(self.h, d_xyz.ptr, d_flag.ptr, n, stride, d_out.ptr, C.byref(n_out), None))
        return d_out.download()[:n_out.value]

    def split(self, xyzg, pose_xy=None, crop_dist=75.0, cap=ICP_MAX_PTS):
        """doICPMatch marshalling: optional crop around pose_xy, then (ga_xy, nga_xy) f64 with the cap."""
        xyzg = np.ascontiguousarray(xyzg, dtype=np.float32)
        n, stride = xyzg.shape
        if n == 0:
            return np.zeros((0, 2)), np.zeros((0, 2))
        d_in = DeviceArray.from_host(xyzg)
        d_ga = DeviceArray((cap, 2), np.float64)
        d_nga = DeviceArray((cap, 2), np.float64)
        counts = (C.c_int * 2)()
        cx, cy = pose_xy if pose_xy is not None else (0.0, 0.0)
        check(lib().slam_ccicp_split_dev(self.h, d_in.ptr, n, stride, 1 if pose_xy is not None else 0, cx, cy,
                                         crop_dist, cap, d_ga.ptr, d_nga.ptr, counts, None))
        return d_ga.download()[:counts[0]], d_nga.download()[:counts[1]]

    def height(self, ground_xyz, pose7):
        """doHeightInterpolate: (z, n_corr, nn_idx[4])."""
        g = np.ascontiguousarray(ground_xyz, dtype=np.float32)
        n, stride = g.shape if g.ndim == 2 else (0, 3)
        pose = (C.c_double * 7)(*pose7)
        z = C.c_double(0.0)
        nc = C.c_int(0)
        idx = (C.c_int * 4)()
        d_g = DeviceArray.from_host(g) if n else None
        check(lib().slam_ccicp_height_dev(self.h, d_g.ptr if d_g else None, n, stride, pose, C.byref(z), C.byref(nc),
                                          idx, None))
        return z.value, nc.value, list(idx)


# ------------------------------------------------------------------ RCCL merge
_rccl = None


def rccl_lib():
    """Loads slam_amd/lib/libslam_mi355x_rccl.so (include/slam_mi355x_rccl.h)."""
    global _rccl
    if _rccl is not None:
        return _rccl
    lib()  # the core library first: the RCCL object links against it
    if not os.path.exists(RCCL_LIB_PATH):
        raise SlamError(E_UNSUPPORTED, "RCCL merge library not built: %s is missing" % RCCL_LIB_PATH)
    R = C.CDLL(RCCL_LIB_PATH, mode=C.RTLD_GLOBAL)
    _H.bind(R, RCCL_EXPORTS)
    _rccl = R
    return R


class Comm(_Handle):
    """One RCCL communicator per process/GPU.  `id_bytes` comes from Comm.unique_id()
    on rank 0 and is handed to the other ranks out of band (e.g. a torch.distributed
    broadcast or a file)."""
    _destroy, _library = "slam_comm_destroy", staticmethod(rccl_lib)
    ID_BYTES = _D["SLAM_COMM_ID_BYTES"]

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(Comm.ID_BYTES)
        check(rccl_lib().slam_comm_unique_id(buf))
        return buf.raw

    def __init__(self, id_bytes, rank, n_ranks):
        h = _vp()
        check(rccl_lib().slam_comm_create(id_bytes, int(rank), int(n_ranks), C.byref(h)))
        self.h = h.value

    @classmethod
    def host(cls, rank, n_ranks, allreduce):
        """slam_comm_create_host: a communicator over a host transport.  allreduce(array, op) reduces a numpy int32
        array in place over all ranks (op = COMM_SUM / COMM_MIN) -- e.g. a gloo all_reduce of torch.from_numpy(array)."""
        self = object.__new__(cls)

        def thunk(_ctx, buf, count, op):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)), op)
                return 0
            except Exception as ex:   # an exception must not unwind through the C frames
                import sys
                print("host all-reduce failed: %r" % (ex,), file=sys.stderr)
                return 1
        self._thunk = HOST_ALLREDUCE_FN(thunk)      # kept alive as long as the communicator
        h = _vp()
        check(rccl_lib().slam_comm_create_host(int(rank), int(n_ranks), self._thunk, None, C.byref(h)))
        self.h = h.value
        return self

    def info(self):
        r, n = C.c_int(), C.c_int()
        check(rccl_lib().slam_comm_info(self.h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def stats(self):
        """slam_comm_get_stats as a dict (waits for the timed all-reduces)."""
        st = CommStats()
        check(rccl_lib().slam_comm_get_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in CommStats._fields_}

    def stats_reset(self):
        check(rccl_lib().slam_comm_stats_reset(self.h))

    def allreduce_grid(self, grid, stream=None):
        check(rccl_lib().slam_grid_allreduce(grid.h, self.h, _sp(stream)))

    def allreduce_rows(self, grid, row_lo, row_hi, stream=None):
        check(rccl_lib().slam_grid_allreduce_rows(grid.h, self.h, int(row_lo), int(row_hi), _sp(stream)))

    def merge_begin(self, grid, stream=None):
        """Unites the ranks' device-tracked dirty rows (8-byte all-reduce) and sends them to the host; returns at once."""
        check(rccl_lib().slam_grid_merge_begin(grid.h, self.h, _sp(stream)))

    def merge_finish(self, grid, stream=None):
        """Waits for the united range, enqueues the all-reduce of those rows; returns (row_lo, row_hi)."""
        lo, hi = C.c_int(), C.c_int()
        check(rccl_lib().slam_grid_merge_finish(grid.h, self.h, _sp(stream), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def merge_async(self, grid, stream=None, then=MERGE_THEN_FINALIZE_RESET, done=None):
        """slam_grid_merge_async: the whole merge (+ what follows it on the stream) from the communicator's helper thread;
        returns a ticket at once.  Nothing else goes to `stream` / `grid` before ticket_wait(ticket)."""
        t = C.c_ulonglong()
        check(rccl_lib().slam_grid_merge_async(grid.h, self.h, _sp(stream), int(then), done.ptr if done is not None else None, C.byref(t)))
        return t.value

    def ticket_wait(self, ticket):
        """The status and united row range (row_lo, row_hi) of a merge posted with merge_async (waits for the helper thread
        to have enqueued it; raises SlamError with E_TIMEOUT / E_COMM when a rank is lost)."""
        lo, hi = C.c_int(), C.c_int()
        check(rccl_lib().slam_comm_ticket_wait(self.h, int(ticket), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def drain(self):
        check(rccl_lib().slam_comm_drain(self.h))

    def set_timeout(self, seconds):
        check(rccl_lib().slam_comm_set_timeout(self.h, float(seconds)))

    def check(self):
        check(rccl_lib().slam_comm_check(self.h))
