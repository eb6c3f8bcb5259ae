#!/usr/bin/env python
"""Cost and effect of smoothBSpline between shortcutPath and the vertex-reducing passes (K9) on Push: 4096 RRT-Connect queries
whose straight line is blocked, at the benchmark's planner settings (2000 iterations, 4096 nodes per tree, max_path 256).
`plan` alone, `plan(vertex_simplify=True, path_shortcut=True)` and the same with `path_smooth=True` in alternated windows of one
process (device events around a window, one synchronise at its end): ms per batch (median [min .. max]) and the ratios; per
solved path of the three forms: vertices, L1 length over the active coordinates, and waypoints of the densified trajectory
(`postprocess_paths`, what the rollout executes) -- mean and maximum; and the smoothing's own counters summed over the batch.
No threshold: the pass cuts corners, it is not expected to shorten paths.

`--baseline-root DIR`: a checkout of another commit with its library built (the parent of the change, say): a child process
imports mopa_rl_amd from there and times `plan` alone on the same queries, before this process touches the GPU.

    python tools/smooth_bench.py --baseline-root ../parent          (writes profiles/r16/smooth_bench.txt)
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = "SawyerPushObstacle-v0"
PRM = dict(max_iters=2000, max_nodes=4096, max_path=256, seed=7)


def blocked_queries(torch, bp, pi, E, device):
    """valid states near the initial pose (init_qpos + N(0, 0.3), clipped), paired; the first E pairs whose straight line fails
    the motion check -- the case in which the rollout calls the planner at all"""
    from mopa_rl_amd.scene import default_qpos
    g = torch.Generator(device=device)
    g.manual_seed(41)
    q0 = torch.tensor(default_qpos(ENV, pi.model), dtype=torch.float64, device=device)
    lo = torch.tensor(pi.jnt_minimum, dtype=torch.float64, device=device)
    hi = torch.tensor(pi.jnt_maximum, dtype=torch.float64, device=device)
    row = q0[None].contiguous()
    have_s, have_g, n = [], [], 0
    while n < E:
        N = 16 * E
        qa = torch.minimum(torch.maximum(q0[:7] + 0.3 * torch.randn(N, 7, generator=g, dtype=torch.float64, device=device), lo), hi).contiguous()
        good = qa[bp.is_valid(qa, row, samples_per_env=N).bool()]
        a, b = good[0:len(good) // 2 * 2:2].contiguous(), good[1:len(good) // 2 * 2:2].contiguous()
        blocked = ~bp.check_motion(a, b, row, samples_per_env=len(a)).bool()
        have_s.append(a[blocked])
        have_g.append(b[blocked])
        n += int(blocked.sum())
    start, goal = q0.repeat(E, 1), q0.repeat(E, 1)
    start[:, :7], goal[:, :7] = torch.cat(have_s)[:E], torch.cat(have_g)[:E]
    return start.contiguous(), goal.contiguous()


def window(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="batches per timed window")
    ap.add_argument("--package-root", default=os.path.dirname(HERE), help="the checkout mopa_rl_amd is imported from")
    ap.add_argument("--baseline-root", default=None, help="another checkout (library built) whose `plan` alone is timed in a child process")
    ap.add_argument("--plan-only", action="store_true", help="time `plan` alone and print one JSON line (what the child process runs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "r16", "smooth_bench.txt"))
    args = ap.parse_args()
    base = None
    if args.baseline_root and not args.plan_only:
        cmd = [sys.executable, os.path.abspath(__file__), "--plan-only", "--package-root", os.path.abspath(args.baseline_root),
               "--queries", str(args.queries), "--rounds", str(args.rounds), "--reps", str(args.reps)]
        env = {k: v for k, v in os.environ.items() if k != "MOPA_HIP_LIB"}
        base = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, env=env).stdout.strip().splitlines()[-1])
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E = args.queries
    start, goal = blocked_queries(torch, bp, pi, E, dev)
    plain = lambda: bp.plan(start, goal, **PRM)
    plain()
    torch.cuda.synchronize()
    if args.plan_only:
        t = [window(torch, plain, args.reps) for _ in range(args.rounds)]
        print(json.dumps({"ms": float(np.median(t)), "min": min(t), "max": max(t), "root": os.path.abspath(args.package_root)}))
        return
    forms = [("plan", plain),
             ("plan(vertex_simplify=True, path_shortcut=True)", lambda: bp.plan(start, goal, vertex_simplify=True, path_shortcut=True, **PRM)),
             ("plan(vertex_simplify=True, path_shortcut=True, path_smooth=True)",
              lambda: bp.plan(start, goal, vertex_simplify=True, path_shortcut=True, path_smooth=True, **PRM))]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for t, (_, fn) in zip(times, forms):
            t.append(window(torch, fn, args.reps))
    res = [fn() for _, fn in forms]
    raw = [t.clone() for t in res[0][:3]]
    info = bp.smooth_paths(raw[0], raw[1], raw[2], seed=PRM["seed"], passes=15, want_info=True)       # the third form's launch, with its counters
    assert torch.equal(raw[1], res[2][1]), "the two-step form differs from plan(...)"
    # what the rollout executes: the un-wrapped, densified trajectory of each solved query
    from mopa_rl_amd.batch import postprocess_paths
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    ro = BatchMoPARollout(make_env(ENV, 64, seed=12, max_episode_steps=1000), RolloutConfig.for_env(ENV))
    dense = []
    for p in res:
        _, ln, need = postprocess_paths(p[0].clone(), p[1], p[2], start, ro.n, ro.cfg.ac_scale, True, ro.limits, ro._valid)
        dense.append((ln, need))
    torch.cuda.synchronize()
    ok = (res[0][2] == 0)
    for p in res[1:]:
        assert torch.equal(res[0][2], p[2]) and torch.equal(res[0][3], p[3]), "a flag changed status or the planner's check counts"
    act = torch.tensor(np.asarray(scene.active_idx), dtype=torch.int64, device=dev)

    def l1(p):          # L1 length over the active coordinates (Push has no SO(2) coordinate)
        rows, n = p[0][:, :, act], p[1]
        step = (rows[:, 1:] - rows[:, :-1]).abs().sum(dim=2)
        live = torch.arange(step.shape[1], device=dev)[None] < (n[:, None] - 1)
        return (step * live).sum(dim=1)
    both = ok.clone()
    for _, need in dense:
        both &= ~need            # densified without the fallback planners in all three forms
    med = lambda t: f"{np.median(t):9.3f} [{min(t):.3f} .. {max(t):.3f}]"
    stat = lambda x: f"mean {x.double().mean():.3f}, max {float(x.double().max()):.3f}"
    w = max(len(name) for name, _ in forms) + 2
    lines = [f"K9 smoothBSpline, {ENV}, {E} RRT-Connect queries with a blocked straight line, {PRM['max_iters']} iterations, "
             f"{PRM['max_nodes']} nodes/tree, max_path {PRM['max_path']}, seed {PRM['seed']}: {int(ok.sum())} solved;",
             f"{args.rounds} alternated rounds of {args.reps} batches per window (device events, one synchronise per window); ms per batch: median [min .. max]", ""]
    for t, (name, _) in zip(times, forms):
        lines.append(f"    {name:<{w}}{med(t)}   ({np.median(t) / np.median(times[0]):.3f} x plan, {np.median(t) / np.median(times[1]):.3f} x shortcut + vertex passes)")
    if base is not None:
        lines.append(f"    {'plan, baseline checkout':<{w}}{base['ms']:9.3f} [{base['min']:.3f} .. {base['max']:.3f}]   (child process, before this one's runs; "
                     f"plan here: {np.median(times[0]) / base['ms']:.3f} x that)")
    lines.append("")
    for k, (name, _) in enumerate(forms):
        lines += [f"    {name}",
                  f"        vertices per solved path      {stat(res[k][1][ok])}",
                  f"        L1 length per solved path     {stat(l1(res[k])[ok])}",
                  f"        densified waypoints           {stat(dense[k][0][both])}   (needing a fallback plan: {int((ok & dense[k][1]).sum())})"]
    lines += [f"    ({int(both.sum())} queries densified without a fallback plan in all three forms)", ""]
    names = ("motion checks", "draws", "rounds", "shortcut splices", "capacity skips", "largest vertex count", "smoothing steps",
             "vertices moved", "idle midpoints dropped", "state checks")
    tot = info[ok].sum(dim=0).tolist()
    lines += ["    counters of the third form's launch, summed over the solved paths (largest vertex count: the maximum):"]
    lines += [f"        {n:<24}{(int(info[ok][:, 5].max()) if k == 5 else tot[k]):>12}" for k, n in enumerate(names)]
    lines.append("")
    ro.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
