#!/usr/bin/env python
"""Cost of the clearance report (K2, mopa_motion_clearance_batch) on Push: 4096 x 256 segments of planner length (the motion-report
bench's workload: a random direction of L1 length `range` from a valid state near the initial pose).  Five forms in alternated
windows of one process (device events around a window, one synchronise at its end):

    check_motion | motion_clearance(band = 0) | (band = 0.01) | (band = 0.05) | proximity(max_pairs=1, band = 0.05)

The last one runs k_proximity_rows over as many states as the segments expand into -- the states k / c along every segment, written
with torch -- which is the per-state kernel k_clearance_states is measured against: the clearance report at the same band minus
check_motion's share of the expansion is expected to cost no more per state.  ms per call (median [min .. max]), ns per expanded
state and the ratios.  Recorded, not bounded.

    timeout -k 10 900 python tools/motion_clearance_bench.py --out profiles/r32/motion_clearance_bench.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ENV = "SawyerPushObstacle-v0"
BANDS = (0.0, 0.01, 0.05)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from motion_report_bench import segments, window
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("motion_clearance_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E, S = args.envs, args.samples
    N = E * S
    a, b, row = segments(torch, bp, pi, N, dev)
    rows = row.repeat(E, 1).contiguous()
    first = bp.motion_clearance(a, b, rows, samples_per_env=S, band=BANDS[-1])
    c = first.n_states.long()
    T = int(c.sum())
    # as many states as the segments expand into, k / c along each (Push has no SO(2) coordinate: a plain lerp)
    seg = torch.repeat_interleave(torch.arange(N, device=dev), c)
    k = torch.arange(T, device=dev) - (torch.cumsum(c, 0) - c)[seg] + 1
    t = (k.double() / c[seg].double())[:, None]
    states = (a[seg] + (b[seg] - a[seg]) * t).contiguous()
    del seg, k, t
    forms = [("check_motion", lambda: bp.check_motion(a, b, rows, samples_per_env=S))]
    for band in BANDS:
        forms.append((f"motion_clearance(band={band})", lambda band=band: bp.motion_clearance(a, b, rows, samples_per_env=S, band=band)))
    forms.append((f"proximity(max_pairs=1, band={BANDS[-1]}), {T} states", lambda: bp.proximity(states, row, samples_per_env=T, band=BANDS[-1], max_pairs=1)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            times[name].append(window(torch, fn, args.reps))
    thr = pi.spec.contact_threshold
    v = forms[0][1]()
    torch.cuda.synchronize()
    assert torch.equal(v.bool(), first.clearance > thr), "clearance > contact_threshold is not check_motion's verdict"
    med = lambda x: f"{np.median(x):9.3f} [{min(x):.3f} .. {max(x):.3f}]"
    m = {name: float(np.median(x)) for name, x in times.items()}
    cm, prox = m[forms[0][0]], m[forms[-1][0]]
    lines = [f"K2 clearance report, {ENV}, {E} x {S} = {N} segments of L1 length range = {pi.spec.range} from valid states near the initial pose, "
             f"resolution 0.005: {T} expanded states ({T / N:.2f} per segment, max {int(c.max())});",
             f"{args.rounds} alternated rounds of {args.reps} calls per window (device events, one synchronise per window); ms per call: median [min .. max]", ""]
    for name, _ in forms:
        lines.append(f"    {name:58s}{med(times[name])}    {m[name] * 1e6 / T:8.2f} ns / state    x {m[name] / cm:7.3f} of check_motion    x {m[name] / prox:6.3f} of proximity")
    mc = m[forms[3][0]]
    lines += ["",
              f"    motion_clearance(band={BANDS[-1]}) / proximity(K = 1) over the same number of states: {mc / prox:.3f} (whole pipeline: count, scan, expand, "
              f"k_clearance_states, reduce); the expectation `no more than 1.1 x` is "
              f"{'met' if mc <= 1.1 * prox else 'NOT met'} by the whole pipeline",
              f"    segments with something within 5 cm: {int((first.k_min > 0).sum())} ({(first.k_min > 0).double().mean().item() * 100:.2f} %); "
              f"clearance <= contact_threshold: {int((first.clearance <= thr).sum())}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    scene.close()


if __name__ == "__main__":
    main()
