#!/usr/bin/env python
"""RRT* (K3b, `plan_star`) next to RRT-Connect (`plan`) on Push: 4096 queries whose straight line is blocked, at the benchmark's
planner settings (2000 iterations, max_path 256; RRT-Connect with 4096 nodes per tree, RRT* with max_iters + 1 nodes), in
alternated windows of one process (device events around a window, one synchronise at its end): ms per batch (median [min ..
max]), solved share, mean L1 path length of the queries both solve, rows per path, and RRT*'s own counters.  No threshold is set:
RRT* spends its whole budget by construction, RRT-Connect stops at its first solution.

The result goes to the next free profiles/rNN/star_bench.txt (or --out).

    python tools/star_bench.py
"""
from __future__ import annotations

import argparse
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from simplify_bench import ENV, blocked_queries, window  # noqa: E402

PRM = dict(max_iters=2000, max_path=256, seed=7)


def next_free(name):
    """profiles/rNN/<name> of the newest round directory, or of a new one behind it when that file exists already"""
    base = os.path.join(ROOT, "profiles")
    nums = sorted(int(m.group(1)) for m in (re.fullmatch(r"r(\d+)", d) for d in os.listdir(base)) if m)
    n = nums[-1] if nums else 1
    if os.path.exists(os.path.join(base, f"r{n:02d}", name)):
        n += 1
    return os.path.join(base, f"r{n:02d}", name)


def l1_lengths(torch, path, plen, so2_cols):
    """L1 length of every path over its first plen rows (SO(2) columns the short way round); path [E, P, na]"""
    d = (path[:, 1:] - path[:, :-1]).abs()
    if len(so2_cols):
        w = d[:, :, so2_cols]
        d[:, :, so2_cols] = torch.where(w > math.pi, 2.0 * math.pi - w, w)
    seg = d.sum(dim=2)
    k = torch.arange(seg.shape[1], device=path.device)[None, :]
    return (seg * (k < (plen[:, None] - 1))).sum(dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=PRM["max_iters"])
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
        raise SystemExit("star_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E = args.queries
    start, goal = blocked_queries(torch, bp, pi, E, dev)
    prm = dict(PRM, max_iters=args.iters)
    connect = lambda: bp.plan(start, goal, max_nodes=4096, **prm)
    star = lambda: bp.plan_star(start, goal, want_info=True, **prm)
    connect()
    star()
    torch.cuda.synchronize()
    tc, ts = [], []
    for _ in range(args.rounds):
        tc.append(window(torch, connect, args.reps))
        ts.append(window(torch, star, args.reps))
    pc, ps = connect(), star()
    torch.cuda.synchronize()
    act = torch.as_tensor(np.asarray(scene.active_idx), dtype=torch.long, device=dev)
    m = pi.model
    so2 = [k for k, a in enumerate(scene.active_idx)
           if any(int(m.jnt_qposadr[j]) == int(a) and int(m.jnt_type[j]) == 3 and not bool(m.jnt_limited[j]) for j in range(len(m.jnt_type)))]
    okc, oks = pc[2] == 0, ps[2] == 0
    both = okc & oks
    lc = l1_lengths(torch, pc[0][:, :, act], pc[1], so2)
    ls = l1_lengths(torch, ps[0][:, :, act], ps[1], so2)
    assert torch.allclose(ls[oks], ps[3][oks], rtol=1e-9), "cost is not the L1 length of the returned rows"
    info = ps[4].double()
    med = lambda t: f"{np.median(t):10.3f} [{min(t):.3f} .. {max(t):.3f}]"
    mean = lambda t: float(t.double().mean()) if len(t) else float("nan")
    lines = [f"K3b RRT* next to RRT-Connect, {ENV}, {E} queries with a blocked straight line, {prm['max_iters']} iterations, max_path {prm['max_path']}, "
             f"seed {prm['seed']}; RRT-Connect: 4096 nodes per tree, RRT*: {prm['max_iters'] + 1} nodes, goal bias 0.05, goal threshold 0;",
             f"{args.rounds} alternated rounds of {args.reps} batches per window (device events, one synchronise per window); ms per batch: median [min .. max]", "",
             f"    plan        (RRT-Connect)     {med(tc)}",
             f"    plan_star   (RRT*)            {med(ts)}",
             f"    ratio of the medians          {np.median(ts) / np.median(tc):10.3f}", "",
             f"    solved share                  plan {float(okc.double().mean()):.4f}    plan_star {float(oks.double().mean()):.4f}    both {float(both.double().mean()):.4f}",
             f"    mean L1 length, both solve    plan {mean(lc[both]):.4f}    plan_star {mean(ls[both]):.4f}    ratio {mean(ls[both]) / mean(lc[both]):.4f}",
             f"    rows per solved path          plan {mean(pc[1][okc]):.2f} (max {int(pc[1].max())})    plan_star {mean(ps[1][oks]):.2f} (max {int(ps[1].max())})",
             f"    RRT* per query (means)        nodes {float(info[:, 1].mean()):.1f}, motion checks {float(info[:, 2].mean()):.1f}, rewires {float(info[:, 3].mean()):.2f}, "
             f"goal nodes {float(info[:, 4].mean()):.2f}, descendant updates {float(info[:, 6].mean()):.2f}, full-tree iterations {float(info[:, 7].mean()):.2f}", ""]
    text = "\n".join(lines)
    print(text)
    out = args.out or next_free("star_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(f"written to {out}")


if __name__ == "__main__":
    main()
