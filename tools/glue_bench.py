#!/usr/bin/env python
"""glue_bodies (the manipulated object attached to the gripper, `Scene.glued`) next to the ordinary scene: `is_valid` at 4096 x 256
states on Push and Assembly and `plan` at 4096 queries on Push, in alternated windows of one process (device events around a window,
one synchronise at its end): ms per batch (median [min .. max]) and the valid / solved shares.  The object is parked between the
claws at the initial pose; both scenes ignore the object-gripper pairs on top of the env's own list.  The glued numbers include the
attach launch (and, for `plan`, the launch that writes the object's pose into the path rows).  No threshold is set: the glued scene
poses the object with every state (Assembly: 5 bodies, 19 geoms that the ordinary scene poses once per tile), runs the generic
kernels (never a baked one) and keeps every candidate pair of the object.

The result goes to --out, or, as with the other *_bench.py tools, to glue_bench.txt in the newest profiles/rNN directory -- in a new
directory behind it when that file exists already, so a recorded run (profiles/r21/glue_bench.txt) is never overwritten.

    python tools/glue_bench.py
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
from star_bench import next_free  # noqa: E402

CASES = {"SawyerPushObstacle-v0": ("clawGripper", "cube"), "SawyerAssemblyObstacle-v0": ("clawGripper", "furniture")}
PRM = dict(max_iters=2000, max_nodes=4096, max_path=256, seed=7)


def subtree(model, root):
    par = np.asarray(model.body_parent)
    s = np.zeros(len(par), dtype=bool)
    s[root] = True
    for b in range(root + 1, len(par)):
        s[b] = s[par[b]]
    return s


def make(env, _lib, default_qpos, planner_inputs):
    """(pi, unglued scene, glued scene, env row with the object parked between the claws)"""
    pi = planner_inputs(env)
    m = pi.model
    a, b = m.body_names.index(CASES[env][0]), m.body_names.index(CASES[env][1])
    grip, obj = subtree(m, a), subtree(m, b)
    gb = np.asarray(m.geom_body)
    ign = {(int(x), int(y)) for x, y in pi.ignored_contacts}
    for g1, g2 in np.asarray(m.pair_geom).reshape(-1, 2):
        if (grip[gb[g1]] and obj[gb[g2]]) or (grip[gb[g2]] and obj[gb[g1]]):
            i, j = int(m.geom_mjid[g1]), int(m.geom_mjid[g2])
            ign.add((min(i, j), max(i, j)))
    scene = _lib.Scene(m, pi.passive_joint_idx, sorted(ign), pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    row = default_qpos(env, m).copy()
    gpos, _ = scene.debug_fk(row)
    claws = [i for i in range(len(gb)) if grip[gb[i]] and gb[i] != a]
    adr = int(m.jnt_qposadr[m.body_jntadr[b]])
    row[adr:adr + 3] = gpos[claws].mean(axis=0)
    return pi, scene, scene.glued(a, b), row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1, help="batches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import default_qpos, planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("glue_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    med = lambda t: f"{np.median(t):10.3f} [{min(t):.3f} .. {max(t):.3f}]"
    E, S = args.envs, args.samples
    lines = [f"glue_bodies next to the ordinary scene; is_valid: {E} envs x {S} states (init pose + N(0, 0.3), clipped), plan: {args.queries} queries, "
             f"{PRM['max_iters']} iterations, {PRM['max_nodes']} nodes per tree, max_path {PRM['max_path']}, seed {PRM['seed']};",
             f"{args.rounds} alternated rounds of {args.reps} batches per window (device events, one synchronise per window); ms per batch: median [min .. max]", ""]
    for env in CASES:
        pi, scene, glued, row = make(env, _lib, default_qpos, planner_inputs)
        bu, bg = BatchPlanner(scene), BatchPlanner(glued)
        g = torch.Generator(device=dev)
        g.manual_seed(41)
        act = torch.as_tensor(np.asarray(scene.active_idx), dtype=torch.long, device=dev)
        q0 = torch.tensor(row, dtype=torch.float64, device=dev)
        lo = torch.tensor(pi.jnt_minimum, dtype=torch.float64, device=dev)
        hi = torch.tensor(pi.jnt_maximum, dtype=torch.float64, device=dev)
        qa = torch.minimum(torch.maximum(q0[act] + 0.3 * torch.randn(E * S, len(act), generator=g, dtype=torch.float64, device=dev), lo), hi).contiguous()
        rows = q0.repeat(E, 1).contiguous()
        out_u = torch.empty(E * S, dtype=torch.uint8, device=dev)
        out_g = torch.empty(E * S, dtype=torch.uint8, device=dev)
        fu = lambda: bu.is_valid(qa, rows, samples_per_env=S, out=out_u)
        fg = lambda: bg.is_valid(qa, rows, samples_per_env=S, out=out_g)
        fu(), fg()
        torch.cuda.synchronize()
        tu, tg = [], []
        for _ in range(args.rounds):
            tu.append(window(torch, fu, args.reps))
            tg.append(window(torch, fg, args.reps))
        lines += [f"{env}: is_valid, {E * S} states ({scene.valid_kernel(E * S)} / glued {glued.valid_kernel(E * S)}; pairs checked {scene.npair_checked} / glued {glued.npair_checked})",
                  f"    ordinary scene                {med(tu)}    valid share {float(out_u.double().mean()):.4f}",
                  f"    glued scene                   {med(tg)}    valid share {float(out_g.double().mean()):.4f}",
                  f"    ratio of the medians          {np.median(tg) / np.median(tu):10.3f}", ""]
        if env.startswith("SawyerPush"):
            Q = args.queries
            good = qa[out_g.bool() & out_u.bool()][:Q].contiguous()
            assert len(good) == Q, "not enough states that are valid in both scenes"
            start = q0.repeat(Q, 1).contiguous()
            goal = start.clone()
            goal[:, act] = good
            pu = lambda: bu.plan(start, goal, **PRM)
            pg = lambda: bg.plan(start, goal, **PRM)
            ru, rg = pu(), pg()
            torch.cuda.synchronize()
            tu, tg = [], []
            for _ in range(args.rounds):
                tu.append(window(torch, pu, args.reps))
                tg.append(window(torch, pg, args.reps))
            lines += [f"{env}: plan, {Q} queries from the initial pose to states valid in both scenes",
                      f"    ordinary scene                {med(tu)}    solved share {float((ru[2] == 0).double().mean()):.4f}    mean checks {float(ru[3].double().mean()):.1f}",
                      f"    glued scene                   {med(tg)}    solved share {float((rg[2] == 0).double().mean()):.4f}    mean checks {float(rg[3].double().mean()):.1f}",
                      f"    ratio of the medians          {np.median(tg) / np.median(tu):10.3f}", ""]
        scene.close()
    text = "\n".join(lines)
    print(text)
    out = args.out or next_free("glue_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(f"written to {out}")


if __name__ == "__main__":
    main()
