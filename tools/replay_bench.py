#!/usr/bin/env python
"""Time of feeding and sampling the replay sink for one agent step (default 4096 envs, D = 40, A = 8): `append_step` with a
50 % `stepped` mask + `append_reuse` of a max_reuse_data = 15 batch ([E * 15] rows, a quarter of them counted) + `sample(256)`
of `DeviceReplayBuffer`, next to a plain-torch formulation of the same three steps written here (cumsum destinations,
index_copy_, torch.randint + index_select) that does not read back either.  Both forms are checked to leave the same ring,
then timed in alternated windows (device events around a window of iterations, one synchronise at its end); reports ms per
iteration (median [min .. max]) and the ratio.  `--launches` adds the kernel launches per iteration of each form, counted
in `rocprofv3 --kernel-trace --stats` runs of their own (fresh child processes, two lengths each; the difference cancels the
set-up's kernels).

    python tools/replay_bench.py --launches --out profiles/r12/replay_bench.txt
"""
from __future__ import annotations

import argparse
import csv
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class TorchRing:
    """The same ring in plain torch, without a read-back: row `capacity` is a sink for the rows that are not kept (index_copy_
    needs a destination for every source row); no oversize rule (a call keeps fewer rows than the ring holds here)."""

    def __init__(self, capacity, D, A, device, seed=0):
        import torch
        self.capacity, self.D, self.A, self.W = capacity, D, A, 2 * D + A + 4
        self.ring = torch.zeros(capacity + 1, self.W, dtype=torch.float32, device=device)
        self.total = torch.zeros((), dtype=torch.int64, device=device)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)

    def _append(self, keep, ob, ac, rew, done, intra, ob_next, ac_type):
        import torch
        f32 = torch.float32
        rows = torch.cat([ob.to(f32), ac[:, :self.A].to(f32), rew.to(f32)[:, None], done.to(f32)[:, None], intra.to(f32)[:, None],
                          ac_type.to(f32)[:, None], ob_next.to(f32)], dim=1)
        k = keep.to(torch.int64)
        incl = torch.cumsum(k, 0)
        dest = torch.where(keep, (self.total + incl - k) % self.capacity, torch.full_like(incl, self.capacity))
        self.ring.index_copy_(0, dest, rows)
        self.total = self.total + incl[-1]

    def append_step(self, out):
        self._append(out["stepped"], out["ob"], out["ac"], out["rew"], out["done"], out["intra_steps"], out["ob_next"], out["ac_type"])

    def append_reuse(self, rb):
        import torch
        keep = torch.arange(rb.cap, device=rb.count.device) < rb.count
        self._append(keep, rb.ob, rb.ac, rb.rew, rb.done, rb.intra_steps, rb.ob_next, rb.ac_type)

    def sample(self, B):
        import torch
        size = self.total.clamp(min=1, max=self.capacity)
        idx = torch.randint(0, 1 << 62, (B,), generator=self.gen, device=self.ring.device) % size
        return torch.index_select(self.ring, 0, idx), idx


def make_inputs(E, D, A, R, device, seed=0):
    import torch
    from mopa_rl_amd.rollout import ReuseBatch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    f64, i32 = torch.float64, torch.int32
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=f64, device=device)
    ri = lambda hi, n, dt: torch.randint(0, hi, (n,), generator=g, device=device).to(dt)
    step = {"ob": rn(E, D), "ac": rn(E, A), "rew": rn(E), "done": ri(2, E, torch.uint8), "intra_steps": ri(70, E, torch.int64), "ob_next": rn(E, D),
            "ac_type": ri(3, E, i32), "stepped": torch.rand(E, generator=g, device=device) < 0.5}
    n = E * R
    z = torch.zeros(n, dtype=i32, device=device)
    rb = ReuseBatch(count=torch.tensor([n // 4], dtype=torch.int64, device=device), env=z, start=z, goal=z, ob=rn(n, D), ac=rn(n, A), rew=rn(n),
                    done=ri(2, n, torch.uint8), intra_steps=ri(70, n, i32), ob_next=rn(n, D), ac_type=ri(3, n, i32))
    return step, rb


def build(form, args, device):
    from mopa_rl_amd.replay import DeviceReplayBuffer
    if form == "hip":
        buf = DeviceReplayBuffer(args.capacity, args.obs_dim, args.ac_dim, device)
        into = buf.empty_sample(args.batch)
        return buf, (lambda: buf.sample(args.batch, into=into))
    buf = TorchRing(args.capacity, args.obs_dim, args.ac_dim, device)
    return buf, (lambda: buf.sample(args.batch))


def iteration(buf, sample, step, rb):
    buf.append_step(step)
    buf.append_reuse(rb)
    sample()


def kernel_calls(form, iters, args):
    """kernel launches of a child process that runs `iters` iterations of one form, from rocprofv3's kernel_stats.csv"""
    work = tempfile.mkdtemp(prefix="replay_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "-o", "trace", "--", sys.executable, os.path.abspath(__file__),
               "--only", form, "--iters", str(iters), "--envs", str(args.envs), "--capacity", str(args.capacity), "--obs-dim", str(args.obs_dim),
               "--ac-dim", str(args.ac_dim), "--reuse", str(args.reuse), "--batch", str(args.batch)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
        calls, mine = 0, 0
        for d, _, files in os.walk(work):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    for r in csv.DictReader(open(os.path.join(d, f))):
                        calls += int(r["Calls"])
                        mine += int(r["Calls"]) if "k_replay_" in r["Name"] else 0
        if calls == 0:
            raise SystemExit("replay_bench: the kernel trace lists no kernel")
        return calls, mine
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--obs-dim", type=int, default=40)
    ap.add_argument("--ac-dim", type=int, default=8)
    ap.add_argument("--reuse", type=int, default=15, help="max_reuse_data: the relabelled batch has envs * reuse rows, a quarter of them counted")
    ap.add_argument("--capacity", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200, help="iterations per timed window")
    ap.add_argument("--launches", action="store_true", help="count kernel launches per iteration in rocprofv3 child runs")
    ap.add_argument("--only", choices=("hip", "torch"), default=None, help="(child of --launches) run one form for --iters iterations and exit")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("replay_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    E, D, A = args.envs, args.obs_dim, args.ac_dim
    step, rb = make_inputs(E, D, A, args.reuse, dev)
    if args.only:
        buf, sample = build(args.only, args, dev)
        for _ in range(args.iters):
            iteration(buf, sample, step, rb)
        torch.cuda.synchronize()
        return
    forms = {f: build(f, args, dev) for f in ("hip", "torch")}
    # the same ring from both forms (three iterations; the torch form's sink row aside), before anything is timed
    for _ in range(3):
        for buf, sample in forms.values():
            iteration(buf, sample, step, rb)
    torch.cuda.synchronize()
    hip, tor = forms["hip"][0], forms["torch"][0]
    kept = int(hip.state[0].item()) // 3
    if int(tor.total.item()) != 3 * kept or not torch.equal(hip.ring.view(torch.int32), tor.ring[:args.capacity].view(torch.int32)):
        raise SystemExit("replay_bench: the two forms leave different rings")
    times = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f, (buf, sample) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                iteration(buf, sample, step, rb)
            e1.record()
            e1.synchronize()
            times[f].append(e0.elapsed_time(e1) / args.reps)
    W = 2 * D + A + 4
    med = {f: float(np.median(t)) for f, t in times.items()}
    lines = [f"replay sink, one agent step's feeding and sampling: append_step ({E} envs, D = {D}, A = {A}, {int(step['stepped'].sum())} stepped) + append_reuse "
             f"({rb.cap} rows, count {int(rb.count[0])}) + sample({args.batch});",
             f"{kept} rows of {W} float32 appended per iteration ({kept * W * 4 / 1e6:.2f} MB), ring capacity {args.capacity}; both forms leave the same ring (checked);",
             f"{args.rounds} alternated rounds, {args.reps} iterations per window (device events, one synchronise at the window's end); ms per iteration: "
             "median [min .. max]", ""]
    names = {"hip": "DeviceReplayBuffer (mopa_replay_append / mopa_replay_sample)", "torch": "plain torch (cumsum, index_copy_, randint + index_select)"}
    for f in forms:
        lines.append(f"    {names[f]:62s} {med[f]:9.4f} [{min(times[f]):.4f} .. {max(times[f]):.4f}]")
    lines.append(f"    ratio torch / library: {med['torch'] / med['hip']:.2f}")
    if args.launches:
        lines.append("")
        lines.append("kernel launches per iteration (rocprofv3 --kernel-trace --stats, child runs of 10 and 30 iterations of one form each; difference / 20):")
        for f in forms:
            (c10, m10), (c30, m30) = kernel_calls(f, 10, args), kernel_calls(f, 30, args)
            lines.append(f"    {names[f]:62s} {(c30 - c10) / 20.0:6.2f} kernels, {(m30 - m10) / 20.0:.2f} of them k_replay_*")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
