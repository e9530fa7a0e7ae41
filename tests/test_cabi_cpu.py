"""CPU-side checks of the C-ABI library: it loads, exports every symbol the
header declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    build.build()
    return api.lib()


def header_functions():
    txt = open(os.path.join(ROOT, "include", "slam_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(L):
    names = header_functions()
    assert len(names) >= 45
    for n in names:
        assert hasattr(L, n), "libslam_mi355x.so does not export %s" % n
    assert sorted(api.EXPORTS) == names


def test_version_and_defaults(L):
    assert b"gfx950" in L.slam_version()
    p = api.icp_default_params()
    # icp.cpp:27
    assert (p.max_iter, p.min_delta, p.mode) == (20, 1e-6, api.ICP_P2P)
    g = api.grid_default_params()
    # mls.h:161,165,188,189
    assert (g.max_range, g.occupancy_increment, g.occupancy_decrement, g.min_cluster_points) == \
        (75.0, 1.0, 0.3, 10)


def test_argument_errors_do_not_need_a_device(L):
    h = C.c_void_p()
    m = np.zeros((2, 2))
    # icp.cpp:38-43: fewer than 5 model points
    rc = L.slam_icp_create(m.ctypes.data_as(C.c_void_p), 2, m.ctypes.data_as(C.c_void_p), 2, None,
                           C.byref(h))
    assert rc == api.E_TOO_FEW_MODEL and b"at least 5 model points" in L.slam_last_error()
    assert L.slam_grid_create(0, 10, 0.1, None, C.byref(h)) == api.E_INVALID


def test_read_model_is_exported_and_checks_its_arguments(L):
    """slam_icp_read_model: declared, exported, bound with pointer signatures, and its argument errors need no device"""
    assert "slam_icp_read_model" in header_functions() and "slam_icp_read_model" in api.EXPORTS
    f = L.slam_icp_read_model
    assert f.argtypes is not None and len(f.argtypes) == 5
    n = C.c_int(-7)
    assert f(None, 0, None, 0, C.byref(n)) == api.E_INVALID and b"slam_icp_read_model" in L.slam_last_error()
    assert n.value == -7                                    # nothing written on a refused call
    assert callable(api.Icp.read_model) and callable(api.Mapper.target_model)


def _no_gpu():
    return api.device_count() == 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_compute_fails_loudly_without_gpu(L):
    with pytest.raises(api.SlamError) as e:
        api.Icp(np.random.randn(10, 2), np.random.randn(10, 2))
    assert e.value.code == api.E_NO_DEVICE and "no CPU path" in str(e.value)
    with pytest.raises(api.SlamError) as e:
        api.Grid(100, 100, 0.1)
    assert e.value.code == api.E_NO_DEVICE
    with pytest.raises(api.SlamError):
        api.DeviceArray((16,), np.float32)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "slam_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                for line in txt.splitlines():
                    if re.match(r"\s*(#\s*include|import|from)\b", line):
                        assert "oracle" not in line, "%s: %s" % (f, line)
                assert "CDLL" not in txt or f == "api.py", f


def test_device_memory_has_one_owner():
    """Handles hold device, pool and pinned memory through slam_amd/csrc/device_mem.hpp alone: a raw allocation call
    elsewhere is a buffer whose free somebody has to remember on every way out."""
    csrc = os.path.join(ROOT, "slam_amd", "csrc")
    raw = {"hipMalloc(": {"runtime.hip", "device_mem.hpp"}, "hipFree(": {"runtime.hip", "device_mem.hpp"},
           "hipHostMalloc(": {"runtime.hip", "device_mem.hpp"}, "hipHostFree(": {"runtime.hip", "device_mem.hpp"},
           "pool_alloc(": {"runtime.hip", "device_mem.hpp", "common.hpp"},
           "pool_free(": {"runtime.hip", "device_mem.hpp", "common.hpp"}, "struct DevBuf": set(), "struct GrowBuf": set()}
    files = sorted(os.listdir(csrc))
    assert "device_mem.hpp" in files and len(files) > 10
    for f in files:
        txt = open(os.path.join(csrc, f), errors="replace").read()
        for what, allowed in raw.items():
            assert what not in txt or f in allowed, "%s holds '%s'" % (f, what)


HEADERS = ("slam_mi355x.h", "slam_mi355x_rccl.h")


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_arities(name):
    """function -> number of parameters, by this file's own regex over the header (not by slam_amd/cdecl.py)"""
    protos = re.findall(r"\b(slam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text(name))
    return {n: 0 if a.strip() == "void" else a.count(",") + 1 for n, a in protos}


def test_python_binding_declares_pointer_signatures(L):
    """ctypes passes an undeclared Python int as a 32-bit C int: a device pointer handed to an entry point
    without argtypes would be truncated (a GPU fault, not an error code).  So every export of both libraries is
    declared, with as many arguments as its prototype has, and the mapping rules hold where each one applies.
    The RCCL library is not loaded here (ahead of torch's own ROCm libraries it ends the process in a double free at exit):
    its side is the table rccl_lib() binds from, and tests/test_multi_rank.py holds the loaded library to that table."""
    class Unloaded:
        def __getattr__(self, n):
            return self.__dict__.setdefault(n, type("F", (), {"argtypes": None, "restype": C.c_int})())

    R = Unloaded()
    api._H.bind(R, api.RCCL_EXPORTS)
    for lib_, exports, header in ((L, api.EXPORTS, HEADERS[0]), (R, api.RCCL_EXPORTS, HEADERS[1])):
        arity = header_arities(header)
        assert sorted(arity) == sorted(exports)
        for n in exports:
            f = getattr(lib_, n)
            assert f.argtypes is not None, n
            assert len(f.argtypes) == arity[n], (n, len(f.argtypes), arity[n])
    vp, i, f32, f64, P = C.c_void_p, C.c_int, C.c_float, C.c_double, C.POINTER
    expected = {
        "slam_grid_transform_cloud_dev": (i, [vp, i, i, vp, vp, vp, vp]),                       # R[9], t[3]
        "slam_icp_index_blob": (i, [vp, i, vp, C.c_size_t, vp]),                                # size_t, size_t *
        "slam_ccicp_voxel_downsample_dev": (i, [vp, vp, vp, i, i, f32, f32, f32, vp, i, vp, vp]),
        "slam_ccicp_select_dev": (i, [vp, vp, i, i, vp, C.c_uint, vp, vp, vp]),
        "slam_grid_total_updates": (i, [vp, vp]),                                               # uint64_t *
        "slam_comm_ticket_wait": (i, [vp, C.c_ulonglong, vp, vp]),
        "slam_grid_merge_async": (i, [vp, vp, vp, i, vp, vp]),                                  # unsigned long long *
        "slam_device_info": (i, [C.c_char_p, i, vp, vp]),
        "slam_vmap_save": (i, [vp, C.c_char_p]),                                                # const char *
        "slam_version": (C.c_char_p, []),
        "slam_icp_destroy": (None, [vp]),
        "slam_icp_set_min_delta": (i, [vp, f64]),
        "slam_pgo_optimize": (i, [vp, i, P(api.PgoResult), vp]),
        "slam_csm_match_post": (i, [vp, vp, i, vp, i, vp, vp, P(api.CsmResult), P(api._H.structs["slam_csm_posterior"])]),
        "slam_comm_get_stats": (i, [vp, P(api.CommStats)]),
        "slam_comm_create_host": (i, [i, i, api.HOST_ALLREDUCE_FN, vp, vp]),
        "slam_comm_unique_id": (i, [vp]),                                                       # char id[SLAM_COMM_ID_BYTES]
        "slam_device_synchronize": (i, []),
    }
    for n, (restype, argtypes) in expected.items():
        f = getattr(R if n in api.RCCL_EXPORTS else L, n)
        assert f.restype is restype and list(f.argtypes) == argtypes, (n, f.restype, f.argtypes)
    assert api.HOST_ALLREDUCE_FN._restype_ is i and api.HOST_ALLREDUCE_FN._argtypes_ == (vp, P(C.c_int32), C.c_size_t, i)
    # a struct position takes the struct by reference, an array of it and NULL, and nothing else
    assert L.slam_pgo_optimize(None, 1, C.byref(api.PgoResult()), None) == api.E_INVALID
    with pytest.raises(C.ArgumentError):
        L.slam_pgo_optimize(None, 1, C.byref(api.PgoParams()), None)
    with pytest.raises(C.ArgumentError):
        L.slam_pgo_optimize(None, 1, C.addressof(api.PgoResult()), None)


def header_structs(name):
    """struct -> [(C field name, is an array)], by this file's own regex"""
    out = {}
    for body, struct in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", header_text(name), flags=re.S):
        out[struct] = [(re.sub(r"\[.*", "", d).split()[-1], "[" in d) for decl in body.split(";") if decl.strip()
                       for d in decl.split(",")]
    return out


def test_python_structs_mirror_the_header(tmp_path):
    """Every struct of both headers, as ctypes has it after slam_amd/cdecl.py read the header, against the compiler: a C
    program prints sizeof and every field's offset, size and element count; ctypes must agree.  The field names are this
    file's own reading of the header; two are Python keywords and carry an underscore in Python."""
    import subprocess
    structs = {s: f for h in HEADERS for s, f in header_structs(h).items()}
    classes = dict({c: getattr(api, py) for py, c in api.STRUCTS.items()}, slam_csm_posterior=api.CsmPosterior)
    assert sorted(structs) == sorted(classes) == sorted(api._H.structs) and len(structs) == 36
    assert {"slam_pf_params", "slam_pf_motion", "slam_pf_state", "slam_gnav_params", "slam_gnav_state"} <= set(structs)
    # declarators that share a line (`int64_t W, S2;`) are read one by one
    assert [f for f, _ in structs["slam_pf_state"]] == [f for f, _ in api.PfState._fields_] and len(structs["slam_pf_state"]) == 17
    for py, c in api.STRUCTS.items():
        assert getattr(api, py) is api._H.structs[c]
    assert issubclass(api.CsmPosterior, api._H.structs["slam_csm_posterior"])
    trace = dict(api.PgoResult._fields_)["trace"]
    assert trace._type_ is api.PgoTrial and trace._length_ == api.PGO_TRACE == 64
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "slam_mi355x_rccl.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, is_array in fields:
            member = "((%s *)0)->%s" % (name, f)
            count = "sizeof(%s) / sizeof(%s[0])" % (member, member) if is_array else "(size_t)0"
            lines.append('printf(" %s=%%zu:%%zu:%%zu", offsetof(%s, %s), sizeof(%s), %s);' % (f, name, f, member, count))
        lines.append('printf("\\n");')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert len(out.strip().splitlines()) == len(structs)
    for line in out.strip().splitlines():
        parts = line.split()
        cls = classes[parts[0]]
        assert int(parts[1]) == C.sizeof(cls), (parts[0], parts[1], C.sizeof(cls))
        c_names = [p.split("=")[0] for p in parts[2:]]
        assert [f[:-1] if f in ("from_", "lambda_") else f for f, _ in cls._fields_] == c_names, parts[0]
        for (f, ctype), p in zip(cls._fields_, parts[2:]):
            off, size, count = (int(v) for v in p.split("=")[1].split(":"))
            d = getattr(cls, f)
            assert (d.offset, d.size, getattr(ctype, "_length_", 0)) == (off, size, count), (parts[0], f, p)


@pytest.mark.parametrize("text, named", [
    ("typedef struct slam_icp slam_icp_t;\nint slam_icp_frob(slam_icp_t *icp, widget_t *w);\n", "widget_t *w"),
    ("typedef struct {\n    int n; widget_t w;\n} slam_frob_params;\n", "widget_t w"),
    ("typedef struct {\n    int n; double trace[SLAM_FROB_TRACE];\n} slam_frob_result;\n", "SLAM_FROB_TRACE"),
    ("int slam_frob(int n);\nunion slam_frob_u { int a; float b; };\n", "union slam_frob_u"),
    ("int slam_frob(int n);\n#define SLAM_FROB(x) ((x) + 1)\n", "SLAM_FROB(x)"),
])
def test_the_header_reader_refuses_what_it_does_not_know(text, named):
    """An unknown parameter type, an unknown field type, an array bound that is neither a literal nor a defined constant,
    and declarations outside the dialect: an exception that names the text, never a function left unbound."""
    from slam_amd import cdecl
    with pytest.raises(cdecl.CDeclError) as e:
        cdecl.Header().parse(text)
    assert named in str(e.value)
    h = cdecl.Header()
    assert h.parse("#define SLAM_FROB_TRACE 4\ntypedef struct {\n    int n; double trace[SLAM_FROB_TRACE], one[2];\n} slam_frob_result;\n"
                   "int slam_frob(const slam_frob_result *r, double out[3]);\n") == ["slam_frob"]
    assert h.functions["slam_frob"] == (C.c_int, [C.POINTER(h.structs["slam_frob_result"]), C.c_void_p])
    assert [(f, getattr(t, "_length_", 0)) for f, t in h.structs["slam_frob_result"]._fields_] == [("n", 0), ("trace", 4), ("one", 2)]


def test_a_handle_closes_once_however_often_it_is_asked(L):
    """close() is safe twice and on an object whose constructor raised before the handle existed; `with` closes."""
    freed = []

    class FakeLibrary:
        slam_thing_destroy = staticmethod(freed.append)

    class Thing(api._Handle):
        _destroy, _library = "slam_thing_destroy", staticmethod(lambda: FakeLibrary)

    with Thing() as t:
        t.h = 1234
    assert freed == [1234] and t.h is None
    t.close()
    t.__del__()
    assert freed == [1234]
    for cls in (api.Icp, api.CorrelativeMatcher, api.PoseGraph, api.VoxelMap, api.Grid, api.DistanceField, api.KeyframeStore,
                api.MlsMap, api.Mapper, api.GroundSegmentation, api.Ccicp, api.Comm, api.Stream, api.Event):
        assert issubclass(cls, api._Handle) and cls._destroy in api.EXPORTS + api.RCCL_EXPORTS, cls
        assert "close" not in vars(cls) and "__del__" not in vars(cls), cls
    half = object.__new__(api.Grid)          # what a constructor that raised before the handle existed leaves behind
    half.close()
    half.close()
    if _no_gpu():
        with pytest.raises(api.SlamError) as e:
            half.__init__(100, 100, 0.1)
        assert e.value.code == api.E_NO_DEVICE and not getattr(half, "h", None)
        half.close()
        half.close()
        half.__del__()


