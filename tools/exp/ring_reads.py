"""Model points the ring searches of the batch kernels evaluate on config 2, before and after the row chords, the probe and the
one-pass seeded form (icp_search.hpp) -- on the CPU, from the oracle's pose trace and tests/ring_restatement.py (numpy only):
the prediction that profiles/r08_ring_prune_ab.txt sets beside the measurement.

    python tools/exp/ring_reads.py [every]        every: count every n-th scan of the 256 (default 4)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle_lib as O
import ring_restatement as RR
from slam_amd import synth

S, ITERS, GATE = 256, 8, 25.0
every = int(sys.argv[1]) if len(sys.argv) > 1 else 4
m_ga, m_nga = synth.make_map(10000)
batch = synth.make_batch(S)
all_xy = np.concatenate([m_ga, m_nga]).astype(np.float32)
# plan_core (icp_build.hip) for a model whose index fits LDS: the pitch the benchmark reports
w, h = np.ptp(all_xy[:, 0]), np.ptp(all_xy[:, 1])
cell = 0.29947564005851746
info = dict(nx=int(np.floor(w / cell)) + 1, ny=int(np.floor(h / cell)) + 1, cell=cell)
L = RR.Lattice(info, all_xy)
idx = [RR.CellIndex(L, m_ga), RR.CellIndex(L, m_nga)]
print("lattice %d x %d cells of %.4f m" % (L.nx, L.ny, L.h))
model = O.IcpModel(m_ga, m_nga)
prm = O.icp_params(30, -1.0, 5.0, O.NN_KDTREE, O.MODE_P2P)

scans = list(range(0, S, every))
un = np.zeros((len(scans), 2))                  # iteration 0: points read per scan, old / new
big = np.zeros((len(scans), ITERS, 2))          # seeded, disk beyond 3 x 3: old / new
small = np.zeros(ITERS)
nq, nbig = np.zeros(ITERS), np.zeros(ITERS)
cu, cs = {}, {}
for a, s in enumerate(scans):
    ga, nga = batch.scan(s)
    _, _, tr, steps = model.fit(ga, nga, batch.R[s], batch.t[s], prm)
    poses = [(batch.R[s].reshape(2, 2), batch.t[s])] + [(tr[k, :4].reshape(2, 2), tr[k, 4:6]) for k in range(ITERS - 1)]
    for pts, ix in ((ga, idx[0]), (nga, idx[1])):
        if not len(pts):
            continue
        prev = None
        for it, (Rk, tk) in enumerate(poses):
            q = (pts @ Rk.T + tk).astype(np.float32)
            if it == 0:
                for v in q:
                    r0, d0 = RR.unseeded(ix, v, new=False, gate=GATE)
                    r1, d1 = RR.unseeded(ix, v, new=True, gate=GATE, count=cu)
                    assert d0 == d1 or min(d0, d1) >= GATE, (d0, d1)
                    un[a] += (r0, r1)
            else:
                for v, sd in zip(q, prev):
                    c = {}
                    r1, d1 = RR.seeded(ix, v, sd, new=True, gate=GATE, count=c)
                    nq[it] += 1
                    if "small" in c:
                        small[it] += r1
                        continue
                    r0, d0 = RR.seeded(ix, v, sd, new=False, gate=GATE)
                    assert d0 == d1, (d0, d1)
                    nbig[it] += 1
                    big[a, it] += (r0, r1)
                    for k_, v_ in c.items():
                        cs[k_] = cs.get(k_, 0) + v_
            prev = ix.nearest(q)
    print("scan %3d: iteration 0 reads %6d -> %6d, seeded beyond 3x3 (iterations 1-%d) %6d -> %6d" %
          (s, un[a, 0], un[a, 1], ITERS - 1, big[a, :, 0].sum(), big[a, :, 1].sum()), flush=True)

npts = float(np.diff(batch.scan_off)[scans].sum())
print("\niteration 0 (unseeded; passes 3 and 4 of a pair's team search like this in every ring iteration), %d scans:" % len(scans))
print("  points per query %.1f -> %.1f; mean scan %d -> %d (%.0f %% fewer); heaviest scan %d -> %d (%.0f %% fewer)" %
      (un[:, 0].sum() / npts, un[:, 1].sum() / npts, un[:, 0].mean(), un[:, 1].mean(), 100 * (1 - un[:, 1].mean() / un[:, 0].mean()),
       un[:, 0].max(), un[:, 1].max(), 100 * (1 - un[:, 1].max() / un[:, 0].max())))
print("  levels probed %d, rows clipped by their chord %d" % (cu.get("probed", 0), cu.get("clipped", 0)))
print("seeded search:")
for it in range(1, ITERS):
    print("  iteration %d: %4.1f %% of queries beyond 3 x 3 cells; they read %7d -> %7d points (%.0f %% fewer); the 3 x 3 path reads %d (%.1f per query)" %
          (it, 100 * nbig[it] / nq[it], big[:, it, 0].sum(), big[:, it, 1].sum(),
           100 * (1 - big[:, it, 1].sum() / max(big[:, it, 0].sum(), 1)), small[it], small[it] / max(nq[it] - nbig[it], 1)))
tot = big.sum(1)
print("  per scan over iterations 1-%d: heaviest %d -> %d, mean %d -> %d; one-pass searches %d of %d beyond 3 x 3" %
      (ITERS - 1, tot[:, 0].max(), tot[:, 1].max(), tot[:, 0].mean(), tot[:, 1].mean(), cs.get("onepass", 0), cs.get("big", 0)))
