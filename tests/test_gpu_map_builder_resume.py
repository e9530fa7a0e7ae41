"""GlobalMapBuilder's save and resume (docs/VOXEL_MAP.md section 10.5) on the six-cloud sequence of
tests/vmap_oracle.py: a builder that adds three clouds, saves and is destroyed, and a fresh one that resumes and adds the
other three, against one builder that adds all six -- poses, counters, every reader of both maps and the last result, bit for
bit; the refusals; and slam_amd::GlobalMapBuilder (tests/cpp/map_builder_resume_test.cpp) against the Python twin: the same
three files byte for byte, and a resume from the Python twin's files to the same final state."""
import os
import signal
import subprocess

import numpy as np
import pytest

import vmap_oracle as V
from slam_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_SECONDS = 120       # the C++ program
TEST_SECONDS = 300
MODES = (dict(), dict(direct=True), dict(carve=True, direct=True))
EXTS = (".vmap", ".dmap", ".pose")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test here ends after TEST_SECONDS, and the session with it: nothing more is started on the GPU."""
    def expired(signum, frame):
        pytest.exit("GPU test exceeded %d s" % TEST_SECONDS, returncode=3)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def clouds():
    return [c for c, _ in V.builder_clouds()]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def readers(m):
    """every reader of a map as bytes"""
    out = [bits(a) for a in m.read()] + [bits(a) for a in m.read_sums()] + [bits(a) for a in m.read_carve()]
    lay = m.layout()
    if lay["distributions"]:
        out += [bits(a) for a in m.read_moments()]
        d = m.read_distributions()
        out += [bits(d[f]) for f in sorted(d)]
    i = m.info()
    return out + [(i["n_voxels"], i["n_points"], lay["leaf"], lay["carved"], lay["distributions"])]


def result_bits(r):
    return None if r is None else {k: bits(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}


def state(b, last):
    return dict(pose=bits(b.pose()), n=(b.n_clouds, b.n_accepted), vmap=readers(b.vmap), dmap=None if b.dmap is None else readers(b.dmap),
                map=bits(b.map()), last=result_bits(last))


def files(prefix, direct):
    return {e: open(prefix + e, "rb").read() for e in EXTS if direct or e != ".dmap"}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=("keyframe", "direct", "carve_direct"))
def test_resume_continues_with_the_same_bits(mode, clouds, tmp_path):
    whole = api.GlobalMapBuilder(**mode)
    for c in clouds:
        ok, last = whole.add_cloud(c)
        assert ok
    want = state(whole, last)
    prefix = str(tmp_path / "half")
    first = api.GlobalMapBuilder(**mode)
    for c in clouds[:3]:
        assert first.add_cloud(c)[0]
    first.save(prefix)
    half_pose = first.pose()
    first.close()
    assert sorted(os.listdir(str(tmp_path))) == sorted("half" + e for e in files(prefix, whole.direct))
    assert len(open(prefix + ".pose", "rb").read()) == 72

    second = api.GlobalMapBuilder(**mode)
    second.resume(prefix)
    assert (second.n_clouds, second.n_accepted) == (3, 3) and bits(second.pose()) == bits(half_pose)
    with pytest.raises(api.SlamError):            # it has taken up three clouds: a second resume is refused
        second.resume(prefix)
    for c in clouds[3:]:
        ok, last = second.add_cloud(c)
        assert ok
    got = state(second, last)
    for f in want:
        assert got[f] == want[f], f
    # and the two save the same files
    whole.save(str(tmp_path / "whole"))
    second.save(str(tmp_path / "second"))
    assert files(str(tmp_path / "whole"), whole.direct) == files(str(tmp_path / "second"), whole.direct)
    whole.close()
    second.close()


@pytest.mark.gpu
def test_resume_refusals(clouds, tmp_path):
    plain, direct = str(tmp_path / "plain"), str(tmp_path / "direct")
    b = api.GlobalMapBuilder()
    d = api.GlobalMapBuilder(direct=True)
    for c in clouds[:2]:
        assert b.add_cloud(c)[0] and d.add_cloud(c)[0]
    b.save(plain)
    d.save(direct)
    before = state(b, None)
    with pytest.raises(api.SlamError) as e:       # after a cloud was added
        b.resume(plain)
    assert e.value.code == api.E_INVALID and state(b, None) == before
    for kw, prefix in ((dict(leaf=0.25), plain), (dict(carve=True), plain), (dict(direct=True), plain), (dict(), direct),
                       (dict(direct=True, carve=True), direct)):
        fresh = api.GlobalMapBuilder(**kw)
        with pytest.raises(api.SlamError):
            fresh.resume(prefix)
        assert (fresh.n_clouds, fresh.vmap.info()["n_voxels"]) == (0, 0) and np.array_equal(fresh.pose(), np.eye(4, dtype=np.float32))
        assert fresh.add_cloud(clouds[0])[0]      # and it is still a working builder
        fresh.close()
    with pytest.raises(api.SlamError) as e:
        api.GlobalMapBuilder().resume(str(tmp_path / "absent"))
    assert e.value.code == api.E_IO
    b.close()
    d.close()


def compile_test(tmp):
    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe = os.path.join(tmp, "map_builder_resume_test")
    lib = os.path.join(ROOT, "slam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_builder_resume_test.cpp"), "-o", exe,
                           "-L" + lib, "-l:libslam_mi355x.so", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_builder_resume_test_compiles(tmp_path):
    """Not a GPU test: the program and the adapter header are valid C++ against the shipped library."""
    assert os.path.exists(compile_test(str(tmp_path)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (dict(), dict(carve=True, direct=True)), ids=("keyframe", "carve_direct"))
def test_cpp_twin_writes_the_same_files_and_resumes_from_pythons(mode, clouds, tmp_path):
    d = str(tmp_path)
    exe = compile_test(d)
    for i, c in enumerate(clouds):
        np.ascontiguousarray(c, np.float32).tofile(os.path.join(d, "cloud_%d.f32" % i))
    py = api.GlobalMapBuilder(**mode)
    for c in clouds[:3]:
        assert py.add_cloud(c)[0]
    py.save(os.path.join(d, "py_half"))
    for c in clouds[3:]:
        assert py.add_cloud(c)[0]
    py.save(os.path.join(d, "py_full"))
    # one run, under its own time limit; a fault ends it and the test with it
    r = subprocess.run([exe, d, str(int(py.carve)), str(int(py.direct))], timeout=RUN_SECONDS, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[-3:] == ["cloud 5 1", "saved 6 6", ""] and "resumed 3 3" in r.stdout
    assert "refused after clouds" in r.stdout and "refused another leaf" in r.stdout
    assert files(os.path.join(d, "cpp_half"), py.direct) == files(os.path.join(d, "py_half"), py.direct)
    assert files(os.path.join(d, "cpp_full"), py.direct) == files(os.path.join(d, "py_full"), py.direct)
    assert os.path.exists(os.path.join(d, "cpp_half.dmap")) == py.direct
    py.close()
