#!/usr/bin/env python
"""Time of the batched contact report next to the validity call it extends, per scene, on the headline batch (4096 x 256 states,
bench.py's generator): `contacts(cutoff=thr, K=16)`, its first stage alone (the min-depth launch on the full pair list) and
`is_valid(want_min_dist=True)` as the planner calls it -- in interleaved rounds (device events), median / min / max.
--frames: also `contacts(frames=True)` in the same rounds, frames on against off: both times and their ratio.
--manifold: also `contacts(manifold=True, max_points=P)` in the same rounds, against off and against frames on.

    python tools/contacts_bench.py --out profiles/r10/contacts_bench.txt
    python tools/contacts_bench.py --frames --out profiles/r25/contacts_frames_bench.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--max-contacts", type=int, default=16)
    ap.add_argument("--frames", action="store_true", help="also time contacts(frames=True): frames on against off")
    ap.add_argument("--manifold", action="store_true", help="also time contacts(manifold=True): manifold on against off (and against frames on)")
    ap.add_argument("--max-points", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import ENV_SPECS, planner_inputs

    dev = torch.device("cuda", 0)
    N = args.envs * args.samples
    lines = [f"contact report vs validity, {args.envs} x {args.samples} = {N} states per call, K = {args.max_contacts}, cutoff = contact_threshold;",
             f"{args.rounds} interleaved rounds of {args.reps} calls each, device events; ms per call: median [min .. max]", ""]
    for env in ENV_SPECS:
        pi = planner_inputs(env)
        sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=7)
        bp, bp_full = BatchPlanner(sc), BatchPlanner(sc.contact_scene())
        qa, rows = bench.make_inputs(torch, pi, args.envs, args.samples, 1234, dev, env=env)
        forms = {
            "is_valid(want_min_dist)": lambda: bp.is_valid(qa, rows, samples_per_env=args.samples, want_min_dist=True),
            "stage 1 (full pair list)": lambda: bp_full.is_valid(qa, rows, samples_per_env=args.samples, want_min_dist=True),
            "contacts": lambda: bp.contacts(qa, rows, samples_per_env=args.samples, max_contacts=args.max_contacts),
        }
        if args.frames:
            forms["contacts(frames=True)"] = lambda: bp.contacts(qa, rows, samples_per_env=args.samples, max_contacts=args.max_contacts, frames=True)
        if args.manifold:
            forms["contacts(manifold=True)"] = lambda: bp.contacts(qa, rows, samples_per_env=args.samples, max_contacts=args.max_contacts, manifold=True,
                                                                   max_points=args.max_points)
        for f in forms.values():           # warm-up: code objects, scratch buffers
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        rep = forms["contacts"]()
        frac = float((rep.count > 0).float().mean())
        mean_cnt = float(rep.count.float().mean())
        t = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append(f"{env}: {frac:.3f} of the states have a record, {mean_cnt:.2f} records per state")
        for k, v in t.items():
            lines.append(f"    {k:<26s} {med[k]:8.3f} [{min(v):.3f} .. {max(v):.3f}]")
        lines.append(f"    stage 2 (k_contact_rows) = contacts - stage 1: {med['contacts'] - med['stage 1 (full pair list)']:.3f} ms;  "
                     f"contacts / is_valid(want_min_dist) = {med['contacts'] / med['is_valid(want_min_dist)']:.2f}")
        if args.frames:
            on, off = med["contacts(frames=True)"], med["contacts"]
            lines.append(f"    frames on {on:.3f} ms against off {off:.3f} ms: k_contact_frames = {on - off:.3f} ms, on / off = {on / off:.3f}")
        if args.manifold:
            on, off = med["contacts(manifold=True)"], med["contacts"]
            lines.append(f"    manifold on (P = {args.max_points}) {on:.3f} ms against off {off:.3f} ms: k_contact_manifolds = {on - off:.3f} ms, on / off = {on / off:.3f}")
            if args.frames:
                fr = med["contacts(frames=True)"]
                lines.append(f"    manifold on against frames on {fr:.3f} ms: manifold / frames = {on / fr:.3f}")
        lines.append("")
        sc.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
