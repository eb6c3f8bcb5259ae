#!/usr/bin/env python
"""Cost of the proximity report (mopa_proximity_batch) next to is_valid and contacts on Push: 4096 x 256 states near the initial pose
(init_qpos + N(0, 0.3), clipped; valid and invalid ones alike).  Five forms in alternated windows of one process (device events
around a window, one synchronise at its end):

    is_valid | contacts(cutoff = contact_threshold) | proximity(band = 0) | proximity(band = 0.01) | proximity(band = 0.05)

ms per call (median [min .. max]) and each form's ratio to is_valid.  The figures are recorded, not bounded: the report gives every
state a wave of its own and runs no verdict early-out, and its cost grows with the band through the margin broad phase.

    python tools/proximity_bench.py --out profiles/r31/proximity_bench.txt

--exact adds an `exact` column: proximity(band, exact=True) at the bands above 0 joins the same alternated rounds, and each is reported
with its ratio to proximity(band) without the keyword (GJK on the shapes as they are against the inflated portal refinement).  Without the
flag the forms, the rounds and the output are what they were.

    python tools/proximity_bench.py --exact --out profiles/r39/proximity_bench.txt

--witness (implies --exact) adds a `witness` column: proximity(band, exact=True, witness=True) at the bands above 0 joins the same
alternated rounds, and each is reported with its ratio to proximity(band, exact=True) -- the cost of the tail kernel behind the report.

    python tools/proximity_bench.py --witness --out profiles/r42/proximity_bench.txt
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = "SawyerPushObstacle-v0"
BANDS = (0.0, 0.01, 0.05)


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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--max-pairs", type=int, default=8)
    ap.add_argument("--exact", action="store_true", help="add proximity(band, exact=True) to the rounds and its ratio to the inflated route")
    ap.add_argument("--witness", action="store_true", help="add proximity(band, exact=True, witness=True) and its ratio to exact=True alone (implies --exact)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.exact = args.exact or args.witness
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import default_qpos, planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("proximity_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E, S = args.envs, args.samples
    N = E * S
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    q0 = torch.tensor(default_qpos(ENV, pi.model), dtype=torch.float64, device=dev)
    lo = torch.tensor(pi.jnt_minimum, dtype=torch.float64, device=dev)
    hi = torch.tensor(pi.jnt_maximum, dtype=torch.float64, device=dev)
    act = torch.tensor(pi.ref_joint_pos_indexes, device=dev)
    q = torch.minimum(torch.maximum(q0[act] + 0.3 * torch.randn(N, len(pi.jnt_minimum), generator=g, dtype=torch.float64, device=dev), lo), hi).contiguous()
    rows = q0[None].repeat(E, 1).contiguous()
    forms = [("is_valid", lambda: bp.is_valid(q, rows, samples_per_env=S)),
             ("contacts(cutoff=threshold)", lambda: bp.contacts(q, rows, samples_per_env=S, max_contacts=args.max_pairs))]
    forms += [(f"proximity(band={b})", lambda b=b: bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs)) for b in BANDS]
    exact_bands = [b for b in BANDS if b > 0] if args.exact else []
    forms += [(f"proximity(band={b}, exact)", lambda b=b: bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs, exact=True))
              for b in exact_bands]
    witness_bands = exact_bands if args.witness else []
    forms += [(f"proximity(band={b}, witness)", lambda b=b: bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs, exact=True, witness=True))
              for b in witness_bands]
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            times[name].append(window(torch, fn, args.reps))
    valid = forms[0][1]().bool()
    reps = {b: bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs) for b in BANDS}
    torch.cuda.synchronize()
    for b in BANDS:
        assert torch.equal(valid, reps[b].clearance > pi.spec.contact_threshold), "the report's clearance disagrees with is_valid"
    med = lambda t: f"{np.median(t):9.3f} [{min(t):.3f} .. {max(t):.3f}]"
    base = float(np.median(times["is_valid"]))
    lines = [f"Proximity report, {ENV}, {E} x {S} = {N} states near the initial pose ({valid.double().mean().item() * 100:.1f} % valid), max_pairs = {args.max_pairs};",
             f"{args.rounds} alternated rounds of {args.reps} calls per window (device events, one synchronise per window); ms per call: median [min .. max]", ""]
    for name, _ in forms:
        lines.append(f"    {name:30s}{med(times[name])}    x {np.median(times[name]) / base:.2f} of is_valid")
    for b in exact_bands:
        r = np.array(times[f"proximity(band={b}, exact)"]) / np.array(times[f"proximity(band={b})"])
        lines.append(f"    exact / inflated at band {b}: x {np.median(times[f'proximity(band={b}, exact)']) / np.median(times[f'proximity(band={b})']):.3f}"
                     f"  (per round {r.min():.3f} .. {r.max():.3f})")
    for b in witness_bands:
        r = np.array(times[f"proximity(band={b}, witness)"]) / np.array(times[f"proximity(band={b}, exact)"])
        lines.append(f"    witness / exact at band {b}: x {np.median(times[f'proximity(band={b}, witness)']) / np.median(times[f'proximity(band={b}, exact)']):.3f}"
                     f"  (per round {r.min():.3f} .. {r.max():.3f})")
    lines.append("")
    for b in BANDS:
        c = reps[b].count
        lines.append(f"    band {b}: pairs in band per state: mean {c.double().mean().item():.2f}, max {int(c.max())};  states with none: {(c == 0).double().mean().item() * 100:.1f} %")
    for b in exact_bands:
        ex = bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs, exact=True)
        torch.cuda.synchronize()
        assert torch.equal(valid, ex.clearance > pi.spec.contact_threshold), "the exact report's clearance disagrees with is_valid"
        gain = ex.clearance - reps[b].clearance
        lines.append(f"    band {b}, exact: pairs in band per state: mean {ex.count.double().mean().item():.2f};  clearance above the inflated one: "
                     f"mean {gain.mean().item():.2e}, max {gain.max().item():.2e}, min {gain.min().item():.2e}")
    for b in witness_bands:
        ex = bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs, exact=True)
        wt = bp.proximity(q, rows, samples_per_env=S, band=b, max_pairs=args.max_pairs, exact=True, witness=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(ex, wt)), "witness=True changed the report's rows"
        used = wt.dist < 1.0e9
        sep = used & (wt.dist > 0)
        err = ((wt.p2 - wt.p1).norm(dim=2) - wt.dist)[sep].abs().max().item() if bool(sep.any()) else 0.0
        lines.append(f"    band {b}, witness: records {int(used.sum())}, of them separated {int(sep.sum())};  largest | |p2 - p1| - dist | over those: {err:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    scene.close()


if __name__ == "__main__":
    main()
