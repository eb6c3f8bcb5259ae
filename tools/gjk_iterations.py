#!/usr/bin/env python3
"""Support evaluations of the exact route (gjk_distance, host compile) per pair class: the histogram DESIGN.md section 4 "Exact route"
quotes and kGjkMaxIt is derived from.  Inputs: tests/proximity_ref.sep_case_list (every gap, bands 1 cm and 5 cm) and, per scene, 200
states near the initial pose and 200 uniform ones, every candidate pair, no broad phase.  No GPU.   python tools/gjk_iterations.py"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import frames_ref as F  # noqa: E402
import proximity_ref as P  # noqa: E402
from conftest import SUPPORTED_ENVS, sample_states  # noqa: E402
from mopa_rl_amd import _lib  # noqa: E402
from mopa_rl_amd.scene import load_scene, planner_inputs  # noqa: E402
from oracle import oracle as O  # noqa: E402

BINS = (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 1 << 30)
hist, capped = {}, 0


def add(names, iters):
    global capped
    capped += int((iters < 0).sum())
    for n, it in zip(names, iters):
        if it != 0:
            hist.setdefault(n, []).append(abs(int(it)))


can = P.can_of(load_scene("sawyer_lift_obstacle"))
cs = P.sep_case_list(can)
types, recs = F.recs_of(cs)
for band in (0.01, 0.05):
    add([c.cls for c in cs], _lib.geom_sep_host(types, recs, band, mesh_verts=can, exact=True, return_iters=True)[1])
O.build()
for env in SUPPORTED_ENVS:
    pi = planner_inputs(env)
    m = pi.model
    orc = O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    qa = np.concatenate([sample_states(pi, 200, 3, "near")[0], sample_states(pi, 200, 4, "uniform")[0]])
    gpos, gmat = P.poses(pi, orc, qa, sample_states(pi, 1, 3)[1], len(qa))
    pg, gt = np.asarray(m.pair_geom).reshape(-1, 2), np.asarray(m.geom_type)
    size = np.where((gt == F.MESH)[:, None], 0.0, np.asarray(m.geom_size, dtype=np.float64))
    rec = np.concatenate([gpos, gmat, np.broadcast_to(size, (len(qa),) + size.shape)], axis=2)[:, pg].reshape(-1, 30)
    tp = np.broadcast_to(gt[pg].astype(np.int32), (len(qa), len(pg), 2)).reshape(-1, 2)
    names = [f"{F.NAMES[min(a, b)]}-{F.NAMES[max(a, b)]}" for a, b in tp]
    for band in (0.01, 0.05):
        add(names, _lib.geom_sep_host(tp, rec, band, mesh_verts=P.can_of(m), exact=True, return_iters=True)[1])
print(f"{'class':18s} {'n':>7s} {'median':>6s} {'max':>4s}   " + " ".join(f"<={b:<3d}" for b in BINS[:-1]) + " more")
top = 0
for cls, v in sorted(hist.items()):
    v = np.array(v)
    top = max(top, int(v.max()))
    counts, lo = [], 0
    for b in BINS:
        counts.append(int(((v > lo) & (v <= b)).sum()))
        lo = b
    print(f"{cls:18s} {len(v):7d} {int(np.median(v)):6d} {int(v.max()):4d}   " + " ".join(f"{c:5d}" for c in counts))
print(f"largest count {top}; twice that, rounded up to a multiple of 8: {-(-2 * top // 8) * 8}; runs ended by the cap: {capped}")
