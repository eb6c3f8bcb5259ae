#!/usr/bin/env python
"""Time of the reuse_data relabelling on one recorded agent step of a Push rollout with planner paths (default 4096 envs,
max_reuse_data 15 and 30): the host loop `reuse_transitions` (its device-to-host copies of the record included; host clock
around calls that end in those copies) next to `reuse_transitions_device` (device events around a window of calls, one
synchronise at the window's end), alternated in one process.  Reports ms per call (median [min .. max]), the transitions kept
and the bytes the device form writes.

    python tools/reuse_bench.py --out profiles/r11/reuse_bench.txt
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENV = "SawyerPushObstacle-v0"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3, help="agent steps taken; the one with the most executed waypoints is relabelled")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2, help="host calls per timed window")
    ap.add_argument("--device-reps", type=int, default=50, help="device calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig

    if not torch.cuda.is_available():
        raise SystemExit("reuse_bench: no GPU (a CPU run measures nothing)")
    E = args.envs
    env = make_env(ENV, E, seed=12, max_episode_steps=1000)
    env.reset()
    ro = BatchMoPARollout(env, RolloutConfig.for_env(ENV, timelimit=0.15, max_nodes=512, max_path=128, num_trials=10))
    rng = np.random.default_rng(4)
    best = None
    for t in range(args.steps):
        ac = rng.uniform(-1, 1, size=(E, 7)) * rng.choice([0.6, 0.9, 1.0], size=(E, 1))
        out = ro.agent_step(torch.tensor(ac, device=env.device), record=True)
        n = int(out["record"]["n_exec"].sum())
        if best is None or n > best[0]:
            best = (n, out)
    n_wp, out = best
    rec = out["record"]
    _, L, D = rec["ob"].shape
    nex = rec["n_exec"].cpu().numpy()
    rec_bytes = sum(int(rec[k].numel()) * rec[k].element_size() for k in ("ob", "meta_rew", "done", "waypoint", "n_exec"))
    lines = [f"reuse_data relabelling, {ENV}, {E} envs, one recorded agent step: record [E, {L}, {D}] = {rec_bytes / 1e6:.1f} MB on the device,",
             f"{int((nex > 3).sum())} envs executed more than 3 waypoints ({n_wp} waypoints in all, longest path {int(nex.max())});",
             f"{args.rounds} alternated rounds; host: {args.host_reps} calls per window (host clock, the calls end in their own copies); device: "
             f"{args.device_reps} calls per window (device events, one synchronise at the end); ms per call: median [min .. max]", ""]
    for R in (15, 30):
        into = ro.reuse_transitions_device(out, max_reuse_data=R)
        host = lambda: ro.reuse_transitions(out, np.random.RandomState(0), max_reuse_data=R)
        dev = lambda: ro.reuse_transitions_device(out, max_reuse_data=R, into=into)
        n_host = len(host())            # warm-up of both forms
        for _ in range(3):
            dev()
        torch.cuda.synchronize()
        kept = int(into.count.cpu()[0])
        row_bytes = 2 * D * 8 + into.ac.shape[1] * 8 + 8 + 1 + 4 * 4
        th, td = [], []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.host_reps):
                host()
            th.append((time.perf_counter() - t0) * 1e3 / args.host_reps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.device_reps):
                dev()
            e1.record()
            e1.synchronize()
            td.append(e0.elapsed_time(e1) / args.device_reps)
        lines.append(f"max_reuse_data {R}:")
        lines.append(f"    host   reuse_transitions         {np.median(th):10.3f} [{min(th):.3f} .. {max(th):.3f}]   {n_host} transitions kept (RandomState(0) draws)")
        lines.append(f"    device reuse_transitions_device  {np.median(td):10.3f} [{min(td):.3f} .. {max(td):.3f}]   {kept} transitions kept (counter-RNG draws), "
                     f"{kept * row_bytes / 1e6:.2f} MB written ({row_bytes} B per row)")
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
