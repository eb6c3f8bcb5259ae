"""K8 (csrc/mopa_pusher_dyn.inc): PusherObstacle-v0 dynamics on the GPU against the sequential checker tests/pusher_dyn_ref.py
(bit for bit), plus what the physics has to do: a swept fingertip pushes the box."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ENV = "PusherObstacle-v0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def _contact_rows(env, ref, E, seed):
    """reset states of E envs; envs 0..7: the fingertip pressed 2 mm into the box; 8..15: the box pressed 2 mm into obstacle7;
    the rest as reset.  Small random velocities and integral terms."""
    rng = np.random.default_rng(seed)
    env.reset()
    qpos = env.qpos.cpu().numpy().copy()
    f = env.pdyn
    for e in range(16):
        q = qpos[e, f.qadr].copy()
        if e < 8:
            q[:4] = rng.uniform(-0.4, 0.4, size=4) + np.array([-0.6, 0.4, 0.3, 0.2])
            P = ref.kinematics(list(q))
            tip = (P[3][0] + P[3][2] * 0.11, P[3][1] + P[3][3] * 0.11)
            q[4], q[5] = tip[0] + P[3][2] * 0.018, tip[1] + P[3][3] * 0.018
        else:
            q[:4] = 0.0
            q[4], q[5] = -0.102, -0.12 + rng.uniform(-0.005, 0.005)
        qpos[e, f.qadr] = q
    qvel = rng.uniform(-0.05, 0.05, size=(E, 6))
    it = rng.uniform(-0.01, 0.01, size=(E, 4))
    return qpos, qvel, it


@pytest.mark.parametrize("contacts", [True, False])
@pytest.mark.parametrize("n", [1, 4, 100])
def test_raw_substeps_are_bit_identical_to_the_checker(torch_mod, contacts, n):
    torch = torch_mod
    from mopa_rl_amd.kinematic_env import make_env
    from pusher_dyn_ref import PusherRef
    E = 64
    env = make_env(ENV, E, dynamics=True, contacts=contacts, seed=3)
    ref = PusherRef(env.pdyn)
    qpos, qvel, it = _contact_rows(env, ref, E, seed=n)
    rng = np.random.default_rng(100 + n)
    prev = qpos[:, env.pdyn.qadr[:4]].copy()
    desired = prev + rng.uniform(-0.3, 0.3, size=(E, 4))
    env.qpos.copy_(torch.tensor(qpos, device="cuda"))
    env.qvel.copy_(torch.tensor(qvel, device="cuda"))
    env.i_term.copy_(torch.tensor(it, device="cuda"))
    stats = torch.zeros(E, dtype=torch.int32, device="cuda")
    env.set_pusher_stats(stats)
    env.pusher_substeps(torch.tensor(desired, device="cuda"), torch.tensor(prev, device="cuda"), n)
    torch.cuda.synchronize()
    gq, gv, gi = env.qpos.cpu().numpy(), env.qvel.cpu().numpy(), env.i_term.cpu().numpy()
    # every env for short runs; for 100 sub-steps the 16 set-up contacts and 8 others (the checker is plain Python)
    check = range(E) if n < 100 else list(range(16)) + list(range(40, 48))
    n_con = 0
    for e in check:
        if contacts and e < 16:
            P = ref.kinematics(list(qpos[e, env.pdyn.qadr]))
            n_con += len(ref.collide(P)) > 0
        row, v, i_ = ref.run_rows(qpos[e], qvel[e], it[e], desired[e], prev[e], n)
        assert np.array_equal(_bits(gq[e]), _bits(row)), (e, gq[e] - row)
        assert np.array_equal(_bits(gv[e]), _bits(v)), (e, gv[e] - v)
        assert np.array_equal(_bits(gi[e]), _bits(i_)), e
    if contacts:
        assert n_con == 16
    assert ref.dropped == 0 and int(stats.sum().item()) == 0
    env.set_pusher_stats(None)
    env.close()


def test_env_step_is_bit_identical_to_the_checker(torch_mod):
    """full env.steps (direct and planner actions, a move mask with a blocked and a sitting-out env, a partial reset): obs,
    reward, done, success and the carried state"""
    torch = torch_mod
    from mopa_rl_amd.kinematic_env import make_env
    from pusher_dyn_ref import PusherEnvRef
    E = 16
    env = make_env(ENV, E, dynamics=True, contacts=True, seed=4, max_episode_steps=3)
    ref = PusherEnvRef(env)
    qpos, _, _ = _contact_rows(env, ref.ref, 16, seed=9)
    env.reset()
    q = env.qpos.cpu().numpy()
    q[:4] = qpos[:4]            # four envs start with the fingertip in the box
    env.qpos.copy_(torch.tensor(q, device="cuda"))
    rng = np.random.default_rng(5)
    for t in range(4):
        if t == 2:
            mk = torch.tensor(np.arange(E) % 3 == 0, device="cuda")
            env.reset(mask=mk)
        ref.load(env)
        is_planner = t % 2 == 1
        act = rng.uniform(-0.2, 0.2, size=(E, 4)) if is_planner else rng.uniform(-1, 1, size=(E, 4))
        mm = np.ones(E, dtype=np.uint8)
        mm[1], mm[2] = 0, 2
        env._launch(torch.tensor(act, device="cuda").contiguous(), is_planner, torch.tensor(mm, device="cuda"))
        torch.cuda.synchronize()
        o, r, d, s = ref.step(act, is_planner, mm)
        assert np.array_equal(_bits(env.qpos.cpu().numpy()), _bits(ref.qpos)), t
        assert np.array_equal(_bits(env.qvel.cpu().numpy()), _bits(ref.qvel)), t
        assert np.array_equal(_bits(env.i_term.cpu().numpy()), _bits(ref.i_term)), t
        assert np.array_equal(_bits(env.prev_state.cpu().numpy()), _bits(ref.prev)), t
        live = mm != 2
        assert np.array_equal(_bits(env.obs.cpu().numpy()[live]), _bits(o[live])), t
        assert np.array_equal(_bits(env.reward.cpu().numpy()[live]), _bits(r[live])), t
        assert np.array_equal(env.done.cpu().numpy()[live], d[live]), t
        assert np.array_equal(env.success.cpu().numpy()[live], s[live]), t
        assert np.array_equal(env.ep_len.cpu().numpy(), ref.ep_len), t
    env.close()


def _sweep(torch, contacts):
    """the straight arm turned to -0.2 rad with the box 1 cm ahead of its distal links (radius 0.3 m, angle -0.1 rad), then six
    planner steps of +0.06 rad on joint0 that sweep the arm through the box's start position -> box start, box end, the deepest
    arm-box penetration seen after each env.step, dropped contacts"""
    from mopa_rl_amd.kinematic_env import make_env
    from pusher_dyn_ref import PusherRef
    E = 8
    env = make_env(ENV, E, dynamics=True, contacts=contacts, seed=1)
    env.reset()
    f = env.pdyn
    ref = PusherRef(f)
    qpos = env.qpos.cpu().numpy()
    qpos[:, f.qadr[:4]] = [-0.2, 0.0, 0.0, 0.0]
    box0 = np.array([0.3 * np.cos(-0.1), 0.3 * np.sin(-0.1)])
    qpos[:, f.qadr[4]], qpos[:, f.qadr[5]] = box0
    env.set_state(torch.tensor(qpos, device="cuda"))
    stats = torch.zeros(E, dtype=torch.int32, device="cuda")
    env.set_pusher_stats(stats)
    act = torch.zeros(E, 4, dtype=torch.float64, device="cuda")
    act[:, 0] = 0.06
    worst, drops = 0.0, 0
    for _ in range(6):
        env.step(act, is_planner=True)
        torch.cuda.synchronize()
        drops += int(stats.sum().item())
        for qn in env.qpos.cpu().numpy()[:, f.qadr]:
            cs = ref.collide(ref.kinematics(list(qn)))
            worst = min([worst] + [c["dist"] for c in cs if f.pair_names[c["pair"]][1] == "box"])
    box1 = env.qpos.cpu().numpy()[:, f.qadr[4:6]]
    env.set_pusher_stats(None)
    env.close()
    return box0, box1, worst, drops


def test_swept_arm_pushes_the_box(torch_mod):
    """fails where `dynamics=True` is refused for the Pusher: with contacts the box is carried along the sweep (> 5 mm towards
    +y) and never sinks more than 1 mm into the arm; without contacts the arm passes through and the box stays where it was."""
    torch = torch_mod
    box0, box1, worst, drops = _sweep(torch, True)
    dy = box1[:, 1] - box0[1]
    assert (dy > 0.005).all(), (box0, box1)
    assert worst > -0.001, worst
    assert drops == 0
    box0n, box1n, _, drops_n = _sweep(torch, False)
    assert np.array_equal(_bits(box1n), _bits(np.repeat(box0n[None], len(box1n), axis=0)))
    assert drops_n == 0


def test_chunked_walks_give_every_env_the_same_transitions(torch_mod):
    """BatchMoPARollout over the Pusher dynamics env: lock-step and asynchronous `walk_chunk` forms give every env the
    transitions (and waypoint records) of the run that walks every path to its end within its call"""
    torch = torch_mod
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    E, T = 24, 3
    rng = np.random.default_rng(11)
    AC = rng.uniform(-1, 1, size=(E, T, 4)) * rng.choice([0.5, 1.0], size=(E, T, 1))
    ACt = torch.tensor(AC, device="cuda")
    runs = {}
    for mode, chunk, asyn in (("whole", 0, False), ("chunk1", 1, True), ("chunk2_lockstep", 2, False)):
        # (episodes long enough that no env resets within the run: a reset's draws depend on which envs reset in a call)
        env = make_env(ENV, E, dynamics=True, contacts=True, seed=5, max_episode_steps=150)
        env.reset()
        ro = BatchMoPARollout(env, RolloutConfig.for_env(ENV, timelimit=0.1, max_nodes=512, max_path=64, num_trials=10, async_planner=asyn,
                                                         planner_first_iters=60, planner_min_job=1, walk_chunk=chunk))
        seq = [[] for _ in range(E)]
        calls = 0
        while min(len(q) for q in seq) < T:
            te = ro.t_env.clamp(max=T - 1)
            ac = ACt[torch.arange(E, device="cuda"), te].contiguous()
            out = ro.agent_step(ac, record=True)
            st = out["stepped"].cpu().numpy()
            rows = np.concatenate([out["rew"].cpu().numpy()[:, None], out["done"].cpu().numpy()[:, None].astype(np.float64),
                                   out["intra_steps"].cpu().numpy()[:, None].astype(np.float64),
                                   out["is_planner"].cpu().numpy()[:, None].astype(np.float64),
                                   env.qpos.cpu().numpy(), env.qvel.cpu().numpy(), env.i_term.cpu().numpy(), out["ac"].cpu().numpy(),
                                   out["ob"].cpu().numpy(), out["ob_next"].cpu().numpy()], axis=1)
            for e in np.where(st)[0]:
                if len(seq[e]) < T:
                    seq[e].append(rows[e])
            calls += 1
            assert calls < 300
        runs[mode] = np.array([np.array(q) for q in seq])
        env.close()
    a = runs["whole"]
    assert a[:, :, 3].sum() > 0 and a[:, :, 1].sum() == 0        # some transitions are planner paths; no episode ended
    for mode in ("chunk1", "chunk2_lockstep"):
        b = runs[mode]
        assert np.array_equal(_bits(a), _bits(b)), (mode, [(tuple(i), a[tuple(i)], b[tuple(i)]) for i in np.argwhere(_bits(a) != _bits(b))[:12]])
