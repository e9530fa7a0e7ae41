"""Inputs shared by tests/test_csm_post_oracle.py (the posterior's restatement alone) and tests/test_gpu_csm_post.py (the
device against it): the two scenes of docs/CSM.md section 6 and the parameter grid.  The scans, windows and edge cases
are those of tests/csm_cases.py."""
import numpy as np

from slam_amd import synth

MARGINS = (0, 16, 255)                      # only exact ties; the default; the whole volume (d <= S* <= 255 n_points)
SCENE_WINDOW = (20, 20, 10, 0.01)           # 41 x 41 x 21 candidates


def room_scene():
    """(m_ga, m_nga, t_ga, t_nga, R0, t0): the synth room, scan 32 of the 256-pose loop, started 0.5 m, -0.4 m, 0.03 rad off"""
    m_ga, m_nga = synth.make_map()
    t_ga, t_nga, pose = synth.make_scan(32, 256)
    R0, t0 = synth.pose_to_Rt(pose[0] + 0.5, pose[1] - 0.4, pose[2] + 0.03)
    return m_ga, m_nga, t_ga, t_nga, R0, t0


def corridor_scene():
    """Two straight walls y = +-1.5 m and nothing else: the score is flat along x.  The model reaches far beyond the window on
    both sides, so every shift along x within it scores alike."""
    def walls(x):
        return np.concatenate([np.stack([x, np.full(len(x), 1.5)], 1), np.stack([x, np.full(len(x), -1.5)], 1)])

    m_nga = walls(np.arange(-30.0, 30.0, 0.05))
    scan = walls(np.arange(-6.0, 6.0, 0.03))
    scan = scan + np.random.default_rng(3).normal(0, 0.01, scan.shape)
    c, s = np.cos(0.02), np.sin(0.02)
    return np.zeros((0, 2)), np.ascontiguousarray(m_nga), np.zeros((0, 2)), np.ascontiguousarray(scan), np.array([[c, -s], [s, c]]), np.array([0.3, 0.2])


def all_outside_scan():
    """17 x 17 x 1 candidates around a start far from every table: every score is 0"""
    import csm_cases as K
    ga, nga = K.scan_of(K.box_model(), 200, K.TRUE_POSE, 200)
    R0, t0 = K.pose_Rt(K.TRUE_POSE[0] + 100.0, K.TRUE_POSE[1] - 250.0, K.TRUE_POSE[2])
    return ga, nga, R0, t0
