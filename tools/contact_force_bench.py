"""Cost of the contact-force readout (`BatchKinematicEnv.enable_contact_force`): ms per env.step of E envs with the readout off, on, and on
with the per-contact rows -- the three Sawyer scenes under tools/ct_bench.py's policy (random actions, maxcon 8) and PusherObstacle-v0
under tools/pusher_dyn_bench.py's (random actions, contacts on).  Per scene three envs with the same seed take the same actions (the
readout changes no state, so the three walk through the same states); the modes are timed as interleaved rounds, so that drift of the
device's clocks hits them alike.
   python tools/contact_force_bench.py [--envs 4096] [--steps 5] [--rounds 5] [--out profiles/r13/contact_force_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mopa_rl_amd.kinematic_env import make_env  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--scenes", default="SawyerPushObstacle-v0,SawyerLiftObstacle-v0,SawyerAssemblyObstacle-v0,PusherObstacle-v0")
ap.add_argument("--out", default="")
a = ap.parse_args()
E, dev = a.envs, torch.device("cuda:0")
MODES = ("off", "on", "on+rows")
lines = [f"contact-force readout: ms per env.step of {E} envs, {a.rounds} interleaved rounds of {a.steps} steps per mode "
         f"({torch.cuda.get_device_name(0)})",
         f"{'scene':28s} {'mode':8s} {'median':>8s} {'min':>8s} {'max':>8s}   rounds"]
for scene in a.scenes.split(","):
    pusher = scene == "PusherObstacle-v0"
    kw = dict(seed=0) if pusher else dict(seed=11, max_episode_steps=1 << 30, contact_options={"maxcon": 8, "maxpair": 8})
    envs = {}
    for mode in MODES:
        env = make_env(scene, E, device=dev, dynamics=True, contacts=True, **kw)
        if mode != "off":
            env.enable_contact_force(rows=(mode == "on+rows"))
        env.reset()
        envs[mode] = env
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    acts = (torch.rand(2 + a.rounds * a.steps, E, envs["off"].action_dim, generator=g, dtype=torch.float64, device=dev) * 2 - 1).contiguous()
    for env in envs.values():          # warm-up: the same two steps everywhere
        env.step(acts[0])
        env.step(acts[1])
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    for r in range(a.rounds):
        for mode in MODES:
            env = envs[mode]
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for t in range(a.steps):
                env.step(acts[2 + r * a.steps + t])
            ev1.record()
            torch.cuda.synchronize()
            ms[mode].append(ev0.elapsed_time(ev1) / a.steps)
    same = all(torch.equal(envs["off"].qpos, envs[m].qpos) for m in MODES[1:])
    for mode in MODES:
        v = ms[mode]
        lines.append(f"{scene:28s} {mode:8s} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}   " + " ".join(f"{x:.3f}" for x in v))
    f = envs["on+rows"]
    lines.append(f"{'':28s} states identical across the modes: {same}; mean contact_force {float(f.contact_force.mean()):.4g}, "
                 f"mean contacts {float(f.contact_count.double().mean()):.2f}")
    for env in envs.values():
        env.close()
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
