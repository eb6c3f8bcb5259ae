#!/usr/bin/env python
"""RRT* under the clearance objective (`plan_star_clearance`) next to path-length RRT* (`plan_star`) on Push: queries whose
straight line is blocked, at the benchmark's planner settings (max_path 256, max_iters + 1 nodes, goal bias 0.05, goal threshold 0),
in alternated windows of one process (device events around a window, one synchronise at its end), per band: ms per batch (median
[min .. max]), motion evaluations per query split into the first evaluation of an iteration, the parent walk and the rewire step,
the solved share (equal by the node-set invariance: asserted), and over the solved queries the mean clearance (`path_clearance` at
the band) and mean L1 length of both planners' paths.  The kernel counts motions, not states: the states per evaluation printed
here are those of the returned segments (`path_clearance(...).segments.n_states`), a proxy.  Recorded, not bounded.

The result goes to the next free profiles/rNN/star_clearance_bench.txt (or --out).

    python tools/star_clearance_bench.py --queries 512 --iters 500
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from simplify_bench import ENV, blocked_queries, window  # noqa: E402
from star_bench import PRM, next_free  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--bands", type=float, nargs="+", default=[0.01, 0.05])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1, help="batches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("star_clearance_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E = args.queries
    start, goal = blocked_queries(torch, bp, pi, E, dev)
    prm = dict(PRM, max_iters=args.iters)
    star = lambda: bp.plan_star(start, goal, want_info=True, **prm)
    med = lambda t: f"{np.median(t):10.3f} [{min(t):.3f} .. {max(t):.3f}]"
    mean = lambda t: float(t.double().mean()) if len(t) else float("nan")
    lines = [f"RRT* under the clearance objective next to path-length RRT*, {ENV}, {E} queries with a blocked straight line, {prm['max_iters']} iterations, "
             f"max_path {prm['max_path']}, seed {prm['seed']}, {prm['max_iters'] + 1} nodes, goal bias 0.05, goal threshold 0;",
             f"{args.rounds} alternated rounds of {args.reps} batches per window (device events, one synchronise per window); ms per batch: median [min .. max]", ""]
    for band in args.bands:
        clear = lambda: bp.plan_star_clearance(start, goal, band, want_info=True, **prm)
        star()
        clear()
        torch.cuda.synchronize()
        ts, tc = [], []
        for _ in range(args.rounds):
            ts.append(window(torch, star, args.reps))
            tc.append(window(torch, clear, args.reps))
        ps, pc = star(), clear()
        torch.cuda.synchronize()
        ok = pc[2] == 0
        assert torch.equal(ps[2], pc[2]), "the solved queries differ: the node-set invariance is broken"
        for col in (1, 4, 5):
            assert torch.equal(ps[4][:, col], pc[5][:, col]), f"info column {col} differs from plan_star's"
        rs, rc = bp.path_clearance(ps[0], ps[1], band), bp.path_clearance(pc[0], pc[1], band)
        torch.cuda.synchronize()
        assert torch.equal(rc.clearance[ok], pc[3][ok]), "clearance is not path_clearance's"
        info = pc[5].double()
        its = float(info[:, 0].mean())
        first = info[:, 2] - info[:, 8] - info[:, 9]
        lines += [f"band {band}",
                  f"    plan_star             (path length)   {med(ts)}",
                  f"    plan_star_clearance                   {med(tc)}",
                  f"    ratio of the medians                  {np.median(tc) / np.median(ts):10.3f}",
                  f"    solved share (both)                   {float(ok.double().mean()):.4f}",
                  f"    motion evaluations per query          {float(info[:, 2].mean()):.1f} = first {float(first.mean()):.1f} + parent walk (column 8) {float(info[:, 8].mean()):.1f}"
                  f" + rewire (column 9) {float(info[:, 9].mean()):.1f};  per iteration {float(info[:, 2].mean()) / its:.3f}, parent walk per appended node "
                  f"{float(info[:, 8].sum() / (info[:, 1] - 1).sum()):.3f};  path-length RRT*: {mean(ps[4][:, 2]):.1f} motion checks per query",
                  f"    rewires per query                     {float(info[:, 3].mean()):.2f} ({float(info[:, 10].mean()):.2f} raised a clearance), descendant updates {float(info[:, 6].mean()):.2f};"
                  f"  path-length RRT*: {mean(ps[4][:, 3]):.2f}",
                  f"    states per returned segment           {mean(rc.segments.n_states):.1f} (a proxy for the states of an evaluation: the kernel counts motions)",
                  f"    mean clearance, solved                plan_star {mean(rs.clearance[ok]):.6f}    plan_star_clearance {mean(pc[3][ok]):.6f}    "
                  f"(strictly higher on {int((pc[3][ok] > rs.clearance[ok]).sum())}, lower on {int((pc[3][ok] < rs.clearance[ok]).sum())} of {int(ok.sum())})",
                  f"    mean L1 length, solved                plan_star {mean(ps[3][ok]):.4f}    plan_star_clearance {mean(pc[4][ok]):.4f}",
                  f"    rows per solved path                  plan_star {mean(ps[1][ok]):.2f}    plan_star_clearance {mean(pc[1][ok]):.2f}", ""]
    text = "\n".join(lines)
    print(text)
    out = args.out or next_free("star_clearance_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(f"written to {out}")


if __name__ == "__main__":
    main()
