"""slam_amd.api.MapLocalizer restated on tests/vmap_gicp_oracle.py's OracleDistMap.register (docs/VOXEL_MAP.md section 11.3),
and the two cases tests/test_map_localizer_cases.py (the restatement alone, no device) and tests/test_gpu_map_localizer.py (the
device against it) share.  The scene is section 9.5's: a 1 m map of clouds 0 .. 4 of vmap_oracle.builder_clouds() at the truth,
the source is cloud 5 through the store's filter at 0.30.  The restated levels are maps integrated directly at leaves 1, 2, 4
and 8: what slam_vmap_coarsen derives is held to them bit for bit elsewhere."""
import math

import numpy as np

import kf_edge_oracle as KE
import kf_gicp_oracle as KG
import vmap_gicp_oracle as VG
import vmap_oracle as V
from slam_amd import api

LEAF, STORE_LEAF = 1.0, 0.30
GATE_RATIO, N_YAW, MIN_PAIR_SHARE = 2.0, 8, 0.5
MAX_ITERATIONS, TRANSFORMATION_EPSILON = 100, 1e-6
# the single registration of docs/VOXEL_MAP.md section 9.5 from the fifth pose ends this far from the truth (mm, mrad)
RECORDED_MM, RECORDED_MRAD = 1.42, 0.031
CASE_A = dict(offset=(-9.7, -0.3, 2.78), levels=4, fan=N_YAW)      # a fan of 8 from 9.7 m and 2.78 rad off
CASE_B = dict(offset=(0.5, 0.3, 0.05), levels=3, fan=1)            # one start nearby
OUT = (api.KF_NO_CORRESPONDENCES, api.KF_DEGENERATE)


def planar(x, y, yaw):
    """GlobalMatcher.planar's matrix: cos and sin in double of the float angle, rounded to float"""
    c, s = np.float32(math.cos(float(np.float32(yaw)))), np.float32(math.sin(float(np.float32(yaw))))
    return np.array([[c, -s, 0, np.float32(x)], [s, c, 0, np.float32(y)], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)


def yaw_fan(x, y, yaw, n):
    """n planar starts at (x, y) with yaws (float)((double) yaw + 2 pi k / n)"""
    return [planar(x, y, np.float32(float(np.float32(yaw)) + 2.0 * math.pi * k / n)) for k in range(n)]


def scene():
    """(map clouds as [(cloud, T64)], the source cloud, its truth 4 x 4 f64 in the map's frame)"""
    clouds = V.builder_clouds(range(6))
    pose0 = clouds[0][1]
    parts = [(c, V.truth_in_first_frame(pose0, p)) for c, p in clouds[:5]]
    return parts, clouds[5][0], V.truth_in_first_frame(pose0, clouds[5][1])


def start_pose(case, truth):
    """(x, y, yaw) as float32 of the case's wrong pose: the truth plus the case's offset"""
    dx, dy, dth = case["offset"]
    return np.float32(truth[0, 3] + dx), np.float32(truth[1, 3] + dy), np.float32(math.atan2(truth[1, 0], truth[0, 0]) + dth)


def starts_of(case, truth):
    return yaw_fan(*start_pose(case, truth), case["fan"])


def pick(level0, n_source, max_score, min_pair_share=MIN_PAIR_SHARE):
    """The winner among the level-0 results (None for a start that is out): converged, fitness <= max_score and
    fitness_pairs >= min_pair_share n_source; the most fitness_pairs, then the lowest index.  -1: nobody."""
    best = -1
    for i, r in enumerate(level0):
        if r is None or r["state"] in OUT or not r["converged"] or not r["fitness"] <= max_score:
            continue
        if not r["fitness_pairs"] >= min_pair_share * n_source:
            continue
        if best < 0 or r["fitness_pairs"] > level0[best]["fitness_pairs"]:
            best = i
    return best


class OracleLocalizer:
    """The localiser on the restated maps.  `filter` stands for the store's voxel filter (the device's own where the device
    is held against this)."""

    def __init__(self, parts, levels, filter=None, leaf=LEAF):
        self.levels = []
        for k in range(levels):
            om = VG.OracleDistMap(math.ldexp(leaf, k))
            for c, T in parts:
                om.integrate(c, T[:3, :3], T[:3, 3])
            self.levels.append(om)
        self.filter = filter or V.cpu_filter(STORE_LEAF)
        self.kf_params = KE.default_params(leaf_size=STORE_LEAF, gate=2.0, transformation_epsilon=1e-6, fitness_epsilon=1e-6)
        self.gp = KG.default_gicp(max_iterations=MAX_ITERATIONS, transformation_epsilon=TRANSFORMATION_EPSILON)
        self.src = None

    def set_scan(self, cloud):
        self.src = KG.OracleCloud(self.filter(cloud), self.kf_params, self.gp)
        return len(self.src.xyz)

    def register(self, level, init):
        """one request at one level from the f32 `init`"""
        p = VG.default_gicp(gate=GATE_RATIO * self.levels[level].leaf, max_iterations=MAX_ITERATIONS, transformation_epsilon=TRANSFORMATION_EPSILON)
        return self.levels[level].register(self.src.xyz, self.src.cov, init, params=p, trace=MAX_ITERATIONS + 1)

    def localize(self, cloud, starts, max_score):
        """dict of found, index, transform, transform64, n_source and last[level][start] (None for a start that was out)"""
        n_source = self.set_scan(cloud)
        T = [np.array(s, np.float32).reshape(4, 4) for s in starts]
        alive = [True] * len(T)
        last = [[None] * len(T) for _ in self.levels]
        for k in range(len(self.levels) - 1, -1, -1):
            for i in range(len(T)):
                if not alive[i]:
                    continue
                r = last[k][i] = self.register(k, T[i])
                if r["state"] in OUT:
                    alive[i] = False
                else:
                    T[i] = r["transform"]
        w = pick(last[0], n_source, max_score)
        return dict(found=w >= 0, index=w, transform=last[0][w]["transform"] if w >= 0 else None,
                    transform64=last[0][w]["transform64"] if w >= 0 else None, n_source=n_source, last=last)
