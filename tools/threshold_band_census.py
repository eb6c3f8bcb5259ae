#!/usr/bin/env python
"""Threshold-band census: how many verdicts hang on a pair class that DESIGN.md section 3 lists as a deviation from MuJoCo 2.0,
with the pair's distance within delta of the contact threshold -- the bound on disagreement with the reference that can be
produced without MuJoCo.

A state is EXPOSED at delta iff
  * no exact-class pair has dist <= thr                      (an exact class would decide "invalid" on both sides),
  * no deviating-class pair has dist <= thr - delta          (a deviation smaller than delta cannot lift it above thr),
  * some deviating-class pair has thr - delta < dist < thr + delta.
Exposed states split into "we say invalid" (a deviating pair in (thr - delta, thr]) and "we say valid".

`census` is the pure-numpy reduction over a contact report taken at cutoff = thr + max(deltas) (still negative: -1 mm on
Sawyer, -0.5 mm on Pusher); `main` runs it on the GPU over the seeded headline batch (bench.py's generator, 4096 x 256) and
over the waypoint rows of the solved paths of one 4096-query plan batch, all four scenes, and writes the table.

    python tools/threshold_band_census.py --out profiles/r10/threshold_band_census.txt
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DELTAS = (1e-6, 1e-5, 1e-4, 1e-3)


def census(count, pair, dist, deviating, thr, deltas=DELTAS, classes=None):
    """count [N], pair [N, K] (-1 = unused), dist [N, K]: a contact report whose cutoff is >= thr + max(deltas) wherever a
    band is to be seen; deviating [npair] bool (scene.deviating_pair_mask); thr: the contact threshold.
    Returns {"n", "truncated" (states with count > K: their lists are incomplete), "rows": [per delta: {"delta", "exposed" /
    "says_invalid" bool [N], "frac_exposed", "frac_invalid", "frac_valid", "by_class": {class: (frac_invalid, frac_valid)}}]}.
    classes (optional, [npair] labels: scene.pair_classes): a state counts for a class when a pair of that class lies in the band."""
    count = np.asarray(count)
    pair = np.asarray(pair, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    deviating = np.asarray(deviating, dtype=bool)
    N, K = pair.shape if pair.ndim == 2 else (len(count), 0)
    used = pair >= 0
    dev = np.zeros_like(used)
    dev[used] = deviating[pair[used]]
    exact = used & ~dev
    exact_bad = (exact & (dist <= thr)).any(axis=1) if K else np.zeros(N, dtype=bool)
    rows = []
    for delta in deltas:
        deep = (dev & (dist <= thr - delta)).any(axis=1) if K else np.zeros(N, dtype=bool)
        band = dev & (dist > thr - delta) & (dist < thr + delta)
        exposed = ~exact_bad & ~deep & band.any(axis=1) if K else np.zeros(N, dtype=bool)
        says_invalid = exposed & (band & (dist <= thr)).any(axis=1) if K else exposed
        row = {"delta": float(delta), "exposed": exposed, "says_invalid": says_invalid,
               "frac_exposed": float(exposed.mean()) if N else 0.0,
               "frac_invalid": float(says_invalid.mean()) if N else 0.0,
               "frac_valid": float((exposed & ~says_invalid).mean()) if N else 0.0, "by_class": {}}
        if classes is not None:
            cls = np.asarray(classes)
            for c in sorted(set(cls[deviating])):
                in_c = np.zeros_like(used)
                in_c[used] = cls[pair[used]] == c
                hit = exposed & (band & in_c).any(axis=1)
                row["by_class"][c] = (float((hit & says_invalid).mean()) if N else 0.0, float((hit & ~says_invalid).mean()) if N else 0.0)
        rows.append(row)
    return {"n": int(N), "truncated": int((count > K).sum()), "rows": rows}


def format_census(title, res):
    lines = [f"{title}: {res['n']} states, {res['truncated']} with more records than slots"]
    for r in res["rows"]:
        lines.append(f"  delta {r['delta']:.0e}: exposed {r['frac_exposed']:.3e}  (we say invalid {r['frac_invalid']:.3e}, valid {r['frac_valid']:.3e})")
        for c, (fi, fv) in r["by_class"].items():
            if fi or fv:
                lines.append(f"      {c:<20s} invalid {fi:.3e}  valid {fv:.3e}")
    return lines


def _queries(torch, bp, pi, E, device, seed=99):
    """start = the env's initial pose + N(0, 0.02) on the arm, goal = a valid state with |dq|_inf <= 0.5 (bench.py's recipe, any scene)"""
    from mopa_rl_amd.scene import default_qpos
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    idx = torch.tensor(pi.ref_joint_pos_indexes, device=device)
    na = len(idx)
    q0 = torch.tensor(default_qpos(pi.spec.env, pi.model), dtype=torch.float64, device=device)
    lo = torch.tensor(pi.jnt_minimum, dtype=torch.float64, device=device)
    hi = torch.tensor(pi.jnt_maximum, dtype=torch.float64, device=device)
    start = q0.repeat(E, 1)
    start[:, idx] += 0.02 * torch.randn(E, na, generator=g, dtype=torch.float64, device=device)
    C = 8
    cand = start[:, idx][:, None, :] + (torch.rand(E, C, na, generator=g, dtype=torch.float64, device=device) - 0.5)
    cand = torch.minimum(torch.maximum(cand, lo), hi).reshape(E * C, na).contiguous()
    ok = bp.is_valid(cand, start.contiguous(), samples_per_env=C).reshape(E, C).bool()
    pick = cand.reshape(E, C, na)[torch.arange(E, device=device), torch.argmax(ok.int(), dim=1)]
    goal = start.clone()
    goal[:, idx] = torch.where(ok.any(dim=1, keepdim=True), pick, start[:, idx])
    return start.contiguous(), goal.contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--max-contacts", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import ENV_SPECS, deviating_pair_mask, pair_classes, planner_inputs

    dev = torch.device("cuda", 0)
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    lib_hash = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    lines = [f"threshold-band census: seed {args.seed}, {args.envs} x {args.samples} states per scene, parent commit {commit}, libmopa_hip.so sha256 {lib_hash}",
             f"contact report at cutoff = thr + {max(DELTAS):g}, K = {args.max_contacts}; classes as in DESIGN.md section 3", ""]
    for env in ENV_SPECS:
        pi = planner_inputs(env)
        thr = pi.spec.contact_threshold
        deltas = DELTAS
        cutoff = thr + max(deltas)          # -1 mm on Sawyer, -0.5 mm on Pusher: still negative, so the report is exact
        sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, thr, range_=pi.spec.range, seed=7)
        bp = BatchPlanner(sc)
        devmask = deviating_pair_mask(pi.model, pi.ignored_contacts)
        cls = pair_classes(pi.model)
        # population 1: the seeded headline batch
        qa, rows = bench.make_inputs(torch, pi, args.envs, args.samples, args.seed, dev, env=env)
        rep = bp.contacts(qa, rows, samples_per_env=args.samples, cutoff=cutoff, max_contacts=args.max_contacts)
        torch.cuda.synchronize()
        res = census(rep.count.cpu().numpy(), rep.pair.cpu().numpy(), rep.dist.cpu().numpy(), devmask, thr, deltas, cls)
        lines += format_census(f"{env} (thr {thr:g}), headline batch", res)
        # population 2: waypoint rows of the solved paths of one plan batch
        start, goal = _queries(torch, bp, pi, args.envs, dev)
        path, plen, status, _ = bp.plan(start, goal, max_iters=2000, max_nodes=4096, max_path=256, seed=7)
        ok = status == 0
        keep = (torch.arange(path.shape[1], device=dev)[None, :] < plen[:, None]) & ok[:, None]
        wp = path[keep].contiguous()
        if len(wp):
            qa_w = wp[:, torch.tensor(pi.ref_joint_pos_indexes, device=dev)].contiguous()
            rep = bp.contacts(qa_w, wp, samples_per_env=1, cutoff=cutoff, max_contacts=args.max_contacts)
            torch.cuda.synchronize()
            res = census(rep.count.cpu().numpy(), rep.pair.cpu().numpy(), rep.dist.cpu().numpy(), devmask, thr, deltas, cls)
            lines += format_census(f"{env}, waypoints of {int(ok.sum())} solved paths of {args.envs} queries", res)
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
