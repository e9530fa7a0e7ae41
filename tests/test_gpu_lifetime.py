"""Handle lifetime: every handle type of slam_amd.api created, used once and destroyed, over and over, must give its
device memory back.  Free device memory is read with hipMemGetInfo of the HIP runtime the library is linked to.

Three warm-up cycles fill the library's pool (common.hpp: pool blocks stay cached after a handle is gone).  S is what one
warm cycle's handles hold while they are all alive (free memory before the cycle minus free memory with every handle
still open).  After CYCLES = 40 further cycles free memory must be at least free_after_warmup - S: a buffer leaked in every
cycle that is 1 / 40 = 2.5 % or more of a cycle's memory crosses that bound.  Smaller per-cycle leaks are what the
source scan of tests/test_cabi_cpu.py and the owning type (slam_amd/csrc/device_mem.hpp) rule out by construction.
Every cycle's results equal the first cycle's bit for bit.

Measured on an MI355X when the test was written (before and after the handles moved to the owning type): S = 501 219 328
bytes, drift over the 40 cycles 0 bytes, run time 4 s (docs/NOTEBOOK.md, 2026-10-16)."""
import ctypes as C

import numpy as np
import pytest

from slam_amd import api, synth

pytestmark = pytest.mark.gpu

WARMUP, CYCLES = 3, 40


def hip_runtime():
    """The libamdhip64 this process has already mapped (the one libslam_mi355x.so resolved)."""
    api.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "the library is loaded but no libamdhip64 is mapped"
    rt = C.CDLL(paths[0])
    rt.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rt.hipMemGetInfo.restype = C.c_int
    return rt


def free_bytes(rt):
    api.synchronize()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module")
def inputs():
    m_ga, m_nga = synth.make_map(10000)
    batch = synth.make_batch(8, n_loop=64)
    cloud0, cloud1 = synth.make_cloud3d(0)[0].astype(np.float32), synth.make_cloud3d(1)[0].astype(np.float32)
    big = np.concatenate([cloud0 + np.float32(0.01 * k) for k in range(9)])  # more than 2^20 points: the pending store grows
    assert len(big) > 1 << 20
    return dict(m_ga=m_ga, m_nga=m_nga, batch=batch, cloud0=cloud0, cloud1=cloud1, big=big)


def cycle(inp, while_alive=None):
    """One of each handle: create, use once, (while_alive() with all of them open,) destroy.  Returns the results."""
    out, handles = [], []
    batch = inp["batch"]
    t_ga, t_nga = batch.scan(0)

    icp = api.Icp(inp["m_ga"], inp["m_nga"])
    handles.append(icp)
    R, t, res = icp.fit(t_ga, t_nga, batch.R[0], batch.t[0])
    out += [R, t, np.frombuffer(bytes(res), np.uint8)]

    grid = api.Grid(400, 400, 0.15, rolling=0, min_cluster_points=20)
    handles.append(grid)
    end = np.concatenate([t_ga, t_nga]).astype(np.float32)
    grid.raycast(np.zeros_like(end), end)
    grid.finalize()
    out += list(grid.read_counts())

    mls = api.MlsMap(300, 300, 0.5)
    handles.append(mls)
    mls.add_cloud(inp["cloud0"], pose=(0.0, 0.0))
    out += list(mls.segmented_clouds())
    cells = mls.read_cells(np.arange(0, 300 * 300, 97, dtype=np.int32))
    out += [cells[k] for k in sorted(cells)]
    mls.add_cloud(inp["big"])
    out.append(np.array([mls.info()["pending_points"]]))

    kf = api.KeyframeStore()
    handles.append(kf)
    a, b = kf.add_keyframe(inp["cloud0"]), kf.add_keyframe(inp["cloud1"])
    edge = kf.register_edges([(a, b, np.eye(4))])[0]
    out += [np.asarray(edge[k]) for k in sorted(edge)]

    seg = api.GroundSegmentation()
    handles.append(seg)
    out.append(seg.segment(inp["cloud0"]))

    cc = api.Ccicp()
    handles.append(cc)
    out.append(cc.voxel_downsample(inp["cloud0"]))

    mp = api.Mapper(inp["m_ga"], inp["m_nga"], grid=dict(rolling=1, min_cluster_points=20, max_range=27.0), max_scans=8,
                    max_points=8 * 1100, grid_size_x=400, grid_size_y=400, resolution=0.15)
    handles.append(mp)
    slot = mp.push(batch, window_xy=(batch.t[0, 0], batch.t[0, 1]))
    out += list(mp.wait(slot))
    mp.finish()
    out += list(mp.grid.read_counts())

    if while_alive is not None:
        while_alive()
    for h in handles:
        h.close()
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_handles_give_their_memory_back(inputs):
    rt = hip_runtime()
    first = cycle(inputs)
    for _ in range(WARMUP - 1):
        assert cycle(inputs) == first
    free_after_warmup = free_bytes(rt)
    alive = []
    assert cycle(inputs, while_alive=lambda: alive.append(free_bytes(rt))) == first
    S = free_after_warmup - alive[0]
    free_after_s = free_bytes(rt)
    for _ in range(CYCLES - 1):
        assert cycle(inputs) == first
    free_after = free_bytes(rt)
    print(f"lifetime: S = {S} bytes, free after warm-up {free_after_warmup}, after the measured cycle {free_after_s}, "
          f"after {CYCLES} cycles {free_after} (drift {free_after_warmup - free_after})")
    assert S > 0
    assert free_after >= free_after_warmup - S
