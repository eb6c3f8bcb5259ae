#!/usr/bin/env python
"""Cost of the motion report (K2, mopa_motion_report_batch) next to check_motion on Push: 4096 x 256 segments of planner length
(a random direction of L1 length `range` from a valid state near the initial pose -- bench.py's A5 segments).  Four forms in
alternated windows of one process (device events around a window, one synchronise at its end):

    check_motion | motion_report(states=False) | motion_report(states=True) | motion_report(max_contacts=4)

ms per call (median [min .. max]) and each report's ratio to check_motion.  The ratio is recorded, not bounded: the report scans
the states of a segment in ascending order, so a segment blocked only at its end state costs all of its states where check_motion
stops after one.

`--baseline-lib PATH`: libmopa_hip.so built from another commit (the parent of the change, say).  Its mopa_check_motion_batch is
loaded next to this checkout's; both are called straight through the C ABI (same host path, one preallocated output) in the same
alternated windows on the same tensors -- the comparison that shows check_motion itself did not move.  The expanded path
synchronises the stream in every call, so host time per call is part of every figure here.

    python tools/motion_report_bench.py --baseline-lib ../parent/mopa_rl_amd/csrc/libmopa_hip.so --out profiles/r28/motion_report_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = "SawyerPushObstacle-v0"


def segments(torch, bp, pi, N, device):
    """N valid states near the initial pose (init_qpos + N(0, 0.3), clipped) and, from each, a segment of L1 length `range`"""
    from mopa_rl_amd.scene import default_qpos
    g = torch.Generator(device=device)
    g.manual_seed(2)
    q0 = torch.tensor(default_qpos(ENV, pi.model), dtype=torch.float64, device=device)
    lo = torch.tensor(pi.jnt_minimum, dtype=torch.float64, device=device)
    hi = torch.tensor(pi.jnt_maximum, dtype=torch.float64, device=device)
    na = len(pi.jnt_minimum)
    act = torch.tensor(pi.ref_joint_pos_indexes, device=device)
    row = q0[None].contiguous()
    have, n = [], 0
    while n < N:
        q = torch.minimum(torch.maximum(q0[act] + 0.3 * torch.randn(N, na, generator=g, dtype=torch.float64, device=device), lo), hi).contiguous()
        good = q[bp.is_valid(q, row, samples_per_env=N).bool()]
        have.append(good)
        n += len(good)
    a = torch.cat(have)[:N].contiguous()
    d = torch.randn(N, na, generator=g, dtype=torch.float64, device=device)
    d = d / d.abs().sum(dim=1, keepdim=True) * pi.spec.range
    b = torch.minimum(torch.maximum(a + d, lo), hi).contiguous()
    return a, b, row


def window(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def raw_check_motion(torch, L, h, a, b, row, S):
    """mopa_check_motion_batch of library L on scene handle h, straight through the C ABI into one preallocated output: the same
    host path for this checkout's library and for the baseline's, so that the two differ in the library alone"""
    vp = C.c_void_p
    valid = torch.empty(len(a), dtype=torch.uint8, device=a.device)
    ptr = lambda t: vp(t.data_ptr())

    def run():
        if L.mopa_check_motion_batch(h, ptr(a), ptr(b), ptr(row), len(a), S, ptr(valid), vp(torch.cuda.current_stream().cuda_stream)) != 0:
            raise SystemExit("motion_report_bench: mopa_check_motion_batch failed")
        return valid
    return run


def baseline_scene(path, _lib, pi):
    """another build of the library and its own scene from the same description"""
    L = C.CDLL(os.path.abspath(path))
    vp = C.c_void_p
    L.mopa_scene_create.argtypes = [C.POINTER(_lib.MopaSceneDesc), C.POINTER(vp)]
    L.mopa_scene_destroy.argtypes = [vp]
    L.mopa_scene_destroy.restype = None
    L.mopa_check_motion_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp]
    desc, keep, _, _ = _lib.scene_desc(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, pi.spec.range, 0.005, 0, 0)
    h = vp()
    if L.mopa_scene_create(C.byref(desc), C.byref(h)) != 0:
        raise SystemExit("motion_report_bench: the baseline library refused the scene")
    del keep
    return L, h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
    ap.add_argument("--baseline-lib", default=None, help="libmopa_hip.so of another commit: its check_motion joins the alternation")
    ap.add_argument("--baseline-first", action="store_true", help="the baseline's window runs before this library's (order effects of the alternation)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs

    if not torch.cuda.is_available():
        raise SystemExit("motion_report_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    pi = planner_inputs(ENV)
    scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    bp = BatchPlanner(scene)
    E, S = args.envs, args.samples
    N = E * S
    a, b, row = segments(torch, bp, pi, N, dev)
    rows = row.repeat(E, 1).contiguous()
    forms = [("check_motion", lambda: bp.check_motion(a, b, rows, samples_per_env=S)),
             ("motion_report(states=False)", lambda: bp.motion_report(a, b, rows, samples_per_env=S, states=False)),
             ("motion_report(states=True)", lambda: bp.motion_report(a, b, rows, samples_per_env=S, states=True)),
             ("motion_report(max_contacts=4)", lambda: bp.motion_report(a, b, rows, samples_per_env=S, max_contacts=4))]
    keep = None
    if args.baseline_lib:
        keep = baseline_scene(args.baseline_lib, _lib, pi)
        forms.insert(1, ("C ABI check_motion, this library", raw_check_motion(torch, _lib.lib(), scene.handle, a, b, rows, S)))
        forms.insert(1 if args.baseline_first else 2, ("C ABI check_motion, baseline lib", raw_check_motion(torch, keep[0], keep[1], a, b, rows, S)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            times[name].append(window(torch, fn, args.reps))
    v = forms[0][1]()
    rep = bp.motion_report(a, b, rows, samples_per_env=S, max_contacts=4)
    torch.cuda.synchronize()
    assert torch.equal(v, rep.valid), "the report's verdicts are not check_motion's"
    if args.baseline_lib:
        assert torch.equal(forms[1][1](), v) and torch.equal(forms[2][1](), v), "the baseline library's verdicts differ"
    fb, c = rep.first_bad, rep.n_states
    blocked = fb > 0
    med = lambda t: f"{np.median(t):9.3f} [{min(t):.3f} .. {max(t):.3f}]"
    base = float(np.median(times["check_motion"]))
    lines = [f"K2 motion report, {ENV}, {E} x {S} = {N} segments of L1 length range = {pi.spec.range} from valid states near the initial pose, "
             f"resolution 0.005; form: {scene.motion_kernel(N)};",
             f"{args.rounds} alternated rounds of {args.reps} calls per window (device events, one synchronise per window); ms per call: median [min .. max]", ""]
    for name, _ in forms:
        lines.append(f"    {name:34s}{med(times[name])}    x {np.median(times[name]) / base:.3f} of check_motion")
    lines += ["",
              f"    states per segment: mean {c.double().mean().item():.2f}, max {int(c.max())};  blocked segments: {int(blocked.sum())} ({blocked.double().mean().item() * 100:.2f} %), "
              f"of them at k = 1: {int((fb == 1).sum())}, only at the end state (c > 1): {int(((fb == c) & (fb > 1)).sum())}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if keep is not None:
        keep[0].mopa_scene_destroy(keep[1])
    scene.close()


if __name__ == "__main__":
    main()
