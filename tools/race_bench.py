#!/usr/bin/env python
"""K3 race (`plan_race`: `portfolio` seeded RRT-Connect members per query, DESIGN.md "K3 race") next to `plan` on the same queries in
the same session: the benchmark's planner queries (`bench.planner_queries`) at the benchmark's planner settings (2000 iterations,
4096 nodes per tree, max_path 256, seed 7), per scene.
  batched leg: E = 4096, portfolio 1 / 2 / 4 / 8
  lone leg:    E = 1 and E = 16, portfolio 1, 2, 4, ..., 256
Per leg, against `plan`: ms per launch (median [min .. max] over interleaved rounds: every round times every entry once, device
events around a window, one synchronise at its end), solved share, mean rows per solved path, and the members cut and checks spent
with and without `no_abort`.  No speed-up is promised: the table is the result.

The result goes to profiles/r19/race_bench.txt (or --out).

    python tools/race_bench.py [--scenes SawyerPushObstacle-v0,...] [--rounds 3]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from simplify_bench import window  # noqa: E402

PRM = dict(max_iters=2000, max_nodes=4096, max_path=256, seed=7)
SCENES = ["SawyerPushObstacle-v0", "SawyerLiftObstacle-v0", "SawyerAssemblyObstacle-v0"]       # (bench.planner_queries: the 7-joint arms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--batched", type=int, default=4096)
    ap.add_argument("--batched-portfolios", default="1,2,4,8")
    ap.add_argument("--lone", default="1,16")
    ap.add_argument("--lone-portfolios", default="1,2,4,8,16,32,64,128,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "race_bench.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("race_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    ints = lambda s: [int(x) for x in s.split(",") if x]
    med = lambda t: f"{np.median(t):9.3f} [{min(t):.3f} .. {max(t):.3f}]"
    lines = [f"K3 race next to plan: bench.planner_queries, {PRM['max_iters']} iterations, {PRM['max_nodes']} nodes per tree, max_path {PRM['max_path']}, "
             f"seed {PRM['seed']}; {args.rounds} interleaved rounds, one launch per window (device events); ms per launch: median [min .. max];",
             "cut = members stopped by the race word per query (mean), spent = checks of all members per query (mean): with the race word / with no_abort", ""]
    for env in [s for s in args.scenes.split(",") if s]:
        bench.ENV = env
        pi = planner_inputs(env)
        scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
        bp = BatchPlanner(scene)
        lines.append(f"== {env}")
        for E, ks in [(args.batched, ints(args.batched_portfolios))] + [(e, ints(args.lone_portfolios)) for e in ints(args.lone)]:
            start, goal = bench.planner_queries(torch, bp, pi, max(E, 16), dev)
            start, goal = start[:E].contiguous(), goal[:E].contiguous()
            entries = [("plan", lambda: bp.plan(start, goal, **PRM))]
            for k in ks:
                entries.append((f"race K={k}", lambda k=k: bp.plan_race(start, goal, portfolio=k, want_info=True, **PRM)))
                entries.append((f"race K={k} no_abort", lambda k=k: bp.plan_race(start, goal, portfolio=k, want_info=True, no_abort=True, **PRM)))
            res = {}
            for name, fn in entries:          # warm-up: scratch growth happens here
                res[name] = fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in entries}
            for _ in range(args.rounds):
                for name, fn in entries:
                    times[name].append(window(torch, fn, 1))
            lines.append(f"  E = {E}")
            for name, _ in entries:
                r = res[name]
                ok = r[2] == 0
                rows = float(r[1][ok].double().mean()) if bool(ok.any()) else float("nan")
                tail = ""
                if name != "plan":
                    info = r[6].double()
                    tail = f"   cut {float(info[:, 0].mean()):7.3f}   spent {float(info[:, 1].mean()):10.1f}   winner != 0: {float((r[4] > 0).double().mean()):.4f}"
                else:
                    tail = f"   checks {float(r[3].double().mean()):10.1f}"
                lines.append(f"    {name:22s} {med(times[name])}   solved {float(ok.double().mean()):.4f}   rows {rows:7.2f}{tail}")
        lines.append("")
        del bp, scene
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(f"written to {args.out}")


if __name__ == "__main__":
    main()
