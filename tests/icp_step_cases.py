"""The inputs of the step certificate (host only): the smallest that still reach the edges of the registration kernels.  Each
case is a model, a batch and the fit's parameters; tests/test_icp_step_certificate.py proves on the CPU what each is for (and that
a swapped neighbour moves a row by at least 100 step tolerances on it), tests/test_gpu_icp_step_certificate.py runs every form
of the kernels on them."""
import functools

import numpy as np

import oracle_lib as O
from slam_amd import synth
from test_gpu_icp_list_pass import TIE_SIGN, corridor
from test_gpu_icp_ring_prune import room_batch, room_model


class Case:
    def __init__(self, name, m_ga, m_nga, batch, max_iter, min_delta=-1.0, indist=5.0, modes=("p2p", "p2l")):
        self.name, self.m_ga, self.m_nga, self.batch = name, m_ga, m_nga, batch
        self.max_iter, self.min_delta, self.indist, self.modes = max_iter, min_delta, indist, modes
        self._models = {}

    def model(self, mode):
        """the CPU oracle's model (normals for point-to-line), made once"""
        if mode not in self._models:
            self._models[mode] = O.IcpModel(self.m_ga, self.m_nga, normals_k=10) if mode == "p2l" else O.IcpModel(self.m_ga, self.m_nga)
        return self._models[mode]


OMODE = {"p2p": O.MODE_P2P, "p2l": O.MODE_P2L}


@functools.lru_cache(maxsize=None)
def _room():
    return room_model(np.random.RandomState(4242))


def _sample(m_ga, m_nga, sizes, rs, err=(0.3, 1.5), ga_share=None):
    """room_batch for any size: samples WITH replacement (a scan may be larger than the model) plus N(0, 0.01^2)"""
    pts, off, nga, Rs, ts = [], [0], [], [], []
    for k, n in enumerate(sizes):
        x, y, th = rs.uniform(-2, 2), rs.uniform(-2, 2), rs.uniform(-np.pi, np.pi)
        R, t = synth.pose_to_Rt(x, y, th)
        share = len(m_ga) / (len(m_ga) + len(m_nga)) if ga_share is None else ga_share[k]
        n_ga = int(n * share)
        for m, c in ((m_ga, n_ga), (m_nga, n - n_ga)):
            w = m[rs.choice(len(m), c)] + rs.normal(0.0, 0.01, (c, 2))
            pts.append((w - t) @ R)
        off.append(off[-1] + n)
        nga.append(n_ga)
        a = rs.uniform(0, 2 * np.pi)
        e_xy = rs.uniform(*err) * np.array([np.cos(a), np.sin(a)])
        e_th = rs.uniform(0.03, 0.06) * rs.choice([-1.0, 1.0]) * min(1.0, err[1])
        R0, t0 = synth.pose_to_Rt(x + e_xy[0], y + e_xy[1], th + e_th)
        Rs.append(R0.reshape(4))
        ts.append(t0)
    return synth.ScanBatch(np.ascontiguousarray(np.concatenate(pts)), np.array(off, np.int32), np.array(nga, np.int32),
                           np.array(Rs), np.array(ts), np.zeros((len(sizes), 3)))


@functools.lru_cache(maxsize=None)
def room():
    """the room of test_gpu_icp_ring_prune.py, scans of [300, 1081, 1081, 300] that start 0.3-1.5 m off: seed disks beyond
    3 x 3 cells, levels probed (reach_counts_fit proves it)"""
    m_ga, m_nga = _room()
    return Case("room", m_ga, m_nga, room_batch(m_ga, m_nga, [300, 1081, 1081, 300], np.random.RandomState(104)), 6)


@functools.lru_cache(maxsize=None)
def outliers():
    """the same room and scans, scans 0 and 2 with 10 % and 50 % of their points thrown up to 4 m away, and a gate of 0.7 m
    (indist is a squared distance: 0.49): the gate rejects some points of every scan in every step"""
    m_ga, m_nga = _room()
    b = room().batch
    rs = np.random.RandomState(77)
    pts = b.pts.copy()
    for s, frac in ((0, 0.1), (2, 0.5)):
        o, e = b.scan_off[s], b.scan_off[s + 1]
        k = rs.choice(np.arange(o, e), int(frac * (e - o)), replace=False)
        pts[k] += rs.uniform(-4.0, 4.0, (len(k), 2))
    return Case("outliers", m_ga, m_nga, synth.ScanBatch(pts, b.scan_off, b.scan_nga, b.R, b.t, b.true_poses), 6, indist=0.49)


@functools.lru_cache(maxsize=None)
def ties():
    """the dyadic corridor of test_gpu_icp_list_pass.py, three scans (an odd batch): eight queries stay at ONE float distance from
    two model points of different index in every step.  Point-to-point only: the point-to-line step leaves the axis at once."""
    m_ga, m_nga, b = corridor()
    q = b.scan(0)[1]
    batch = synth.ScanBatch(np.ascontiguousarray(np.concatenate([q, q, q])), np.arange(4, dtype=np.int32) * len(q), np.zeros(3, np.int32),
                            np.array([b.R[0]] * 3), np.array([b.t[0]] * 3), np.zeros((3, 3)))
    return Case("ties", m_ga, m_nga, batch, 5, modes=("p2p",))


N_TIE_QUERIES = len(TIE_SIGN)

RAGGED_SIZES = [5, 63, 64, 65, 513, 1081, 2600, 3, 200, 700, 6]


@functools.lru_cache(maxsize=None)
def ragged():
    """5 to 2600 points around the sizes of a wavefront, a pass and a team; a scan of 3 points (left alone), a scan without
    class-GA points and one without class-NGA points; eleven scans, an odd batch; starts 0.2-0.6 m off"""
    m_ga, m_nga = _room()
    share = [None] * len(RAGGED_SIZES)
    share[0] = 0.4                        # the 5-point scan: two and three points, on different walls
    share[8], share[9] = 0.0, 1.0         # an empty class GA, an empty class NGA
    share = [len(m_ga) / (len(m_ga) + len(m_nga)) if v is None else v for v in share]
    return Case("ragged", m_ga, m_nga, _sample(m_ga, m_nga, RAGGED_SIZES, np.random.RandomState(909), (0.2, 0.6), share), 4)


@functools.lru_cache(maxsize=None)
def small_class():
    """a model whose class GA has three points: the class is skipped (icpPointToPoint.cpp:59, :93), its queries pair with nothing"""
    m_ga, m_nga = _room()
    return Case("small_class", m_ga[[10, 400, 800]], m_nga, _sample(m_ga, m_nga, [64, 513, 300], np.random.RandomState(910), (0.2, 0.6)), 4)


@functools.lru_cache(maxsize=None)
def early(min_delta):
    """five scans that start 2 to 30 cm off and stop on min_delta after different numbers of steps (partners stopping apart)"""
    m_ga, m_nga = _room()
    b = _sample(m_ga, m_nga, [300, 1081, 700, 1081, 300], np.random.RandomState(911), (0.02, 0.021))
    for s, scale in enumerate([1.0, 15.0, 4.0, 1.0, 8.0]):        # the initial error, scaled per scan about the true pose
        b.t[s] = b.t[s] + (scale - 1.0) * np.array([0.014, -0.012])
    return Case("early_%g" % min_delta, m_ga, m_nga, b, 12, min_delta=min_delta)


def all_cases():
    return [room(), outliers(), ties(), ragged(), small_class(), early(1e-2), early(1e-4), early(1e-9)]


CASE_NAMES = ["room", "outliers", "ties", "ragged", "small_class", "early_0.01", "early_0.0001", "early_1e-09"]


def by_name(name):
    return {c.name: c for c in all_cases()}[name]
