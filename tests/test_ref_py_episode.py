"""What the evaluation-loop fixtures of tests/test_gpu_rollout.py hold (tests/golden/ref_py_episode_*.npz, written by
tools/gen_ref_py_golden.py `episode` from the reference's own `MoPARolloutRunner.run_episode`): a parity test is worth what its
fixture exercises, so the properties the GPU tests rely on -- unequal episode lengths (envs that sit out), episodes that end on
success before the time cap, both values of the discrete head, every branch of the step -- are asserted here, on the CPU, for
what the reference itself produced.  And the action `run_episode` gives a sitting-out env: its IK target must be finite."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
COUNTERS = ("mp", "rl", "interpolation", "mp_fail", "approximate", "invalid")


def _load(name):
    G = np.load(os.path.join(GOLD, name))
    cap = int(G["params"][4])                    # max_episode_steps
    return G, cap, dict(zip(COUNTERS, G["counters"].sum(0).tolist()))


def test_assembly_ik_episode_fixture_has_sit_outs_and_success_endings():
    G, cap, tot = _load("ref_py_episode_assembly_ik.npz")
    n, start = G["n_steps"], G["ep_len_start"]
    assert G["ac"].shape == (16, cap, 7) and cap == 14
    assert len(np.unique(n)) >= 3, n
    assert int((n <= n.max() - 3).sum()) >= 8, n                     # envs that sit out three or more calls of the batched loop
    assert start.any() and len(np.unique(start)) >= 3, start
    assert tot["interpolation"] > 0 and tot["rl"] > 0, tot
    # the loop's own `ep_len` starts at 0 whatever the env's counter says (rl/mopa_rollouts.py:415): the cap ends an episode at cap - start
    won = G["ep_success"] == 1
    assert np.array_equal(G["ep_len"][~won], (cap - start)[~won])
    # success endings before the cap, after several agent steps and after one
    early = won & (G["ep_len"] < cap - start)
    assert int(early.sum()) >= 2, G["ep_success"]
    assert (n[early] >= 3).any() and (n[early] == 1).any(), n[early]
    # ... one of them in the middle of a path: a planner step (with this action space two waypoints) that took one env step
    mid_path = early & (n == 1) & (G["counters"][:, COUNTERS.index("interpolation")] == 1) & (G["ep_len"] == 1)
    assert mid_path.any()
    # the episode of a winner ends with done = 1 on its last step, and the success reward is in it
    last = G["done"][np.arange(16), n - 1]
    assert (last == 1).all() and (G["rew"][np.arange(16), n - 1][won] > 100).all() and (G["ep_rew"][~won] < 100).all()
    # the time cap cuts a path between its waypoints as well (odd remaining length, planner steps of two env steps only)
    only_paths = (G["counters"][:, COUNTERS.index("rl")] == 0) & ~won
    assert (only_paths & (G["ep_len"] % 2 == 1)).any()


def test_assembly_ik_episode_fixture_never_plans_from_an_invalid_state(oracle_mod):
    """With `use_ik_target` a planner step's target IS the current state (rl/mopa_rollouts.py:483: target_qpos is never moved), so from
    a state in collision the invalid-target back-off divides 0 by 0.  The fixture keeps clear of that: every state a step starts
    from, and every state an episode ends in -- where the env then sits out --, passes the validity check."""
    from mopa_rl_amd.scene import planner_inputs
    G, cap, tot = _load("ref_py_episode_assembly_ik.npz")
    pi = planner_inputs("SawyerAssemblyObstacle-v0")
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    for e, n in enumerate(G["n_steps"]):
        for q in list(G["qpos_start"][e, :n]) + [G["qpos_final"][e]]:
            assert orc.is_valid(q)[0], e
    assert tot["invalid"] == 0 and tot["mp_fail"] == 0 and not G["pulled_back"].any()


def test_push_discrete_episode_fixture_takes_every_branch():
    G, cap, tot = _load("ref_py_episode_push_discrete.npz")
    assert G["ac"].shape == (16, cap, 7) and G["ac_type"].shape == (16, cap)
    n = G["n_steps"]
    used = np.arange(cap)[None, :] < n[:, None]
    assert set(np.unique(G["ac_type"][used])) == {0, 1}
    assert len(np.unique(n)) >= 4, n
    assert tot["rl"] > 0 and tot["interpolation"] > 0 and tot["mp_fail"] > 0 and tot["invalid"] > 0, tot
    # the head, not the magnitude, decided: small actions that went to the planner and large ones executed directly
    big = (np.abs(G["ac"]) > 0.7).any(axis=2)
    ty = G["ac_type"].astype(bool)
    assert (ty & ~big & used).any() and (~ty & big & used).any()


def test_sit_out_action_has_a_finite_ik_target():
    """`run_episode` hands finished envs `sit_out_action`'s neutral row; through the array-operation form of `k_ik_targets` its
    orientation target is the site's own [3, 0, 1, 1]-indexed quaternion (finite), the position target the site's position; the rows
    of the envs still in their episode are the policy's, untouched."""
    import torch
    from mopa_rl_amd.rollout import ik_targets_torch, sit_out_action
    g = torch.Generator().manual_seed(3)
    E = 6
    ac = torch.rand(E, 7, dtype=torch.float64, generator=g) * 2 - 1
    alive = torch.tensor([True, False, True, False, False, True])
    for use_ik in (False, True):
        got = sit_out_action(ac, alive, use_ik)
        assert got.dtype == torch.float64 and got.is_contiguous()
        assert torch.equal(got[alive], ac[alive])
        want = torch.zeros(7, dtype=torch.float64)
        if use_ik:
            want[3] = 1.0
        assert torch.equal(got[~alive], want.expand(int((~alive).sum()), 7))
    # float32 input (a policy network's output) comes out as float64 rows of the same values
    assert torch.equal(sit_out_action(ac.float(), alive, True)[alive], ac.float().double()[alive])
    # rotations about random axes as site orientations
    ax = torch.randn(E, 3, dtype=torch.float64, generator=g)
    ax = ax / ax.norm(dim=1, keepdim=True)
    ang = torch.rand(E, 1, 1, dtype=torch.float64, generator=g) * 3.0
    K = torch.zeros(E, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    site_mat = torch.eye(3, dtype=torch.float64) + torch.sin(ang) * K + (1 - torch.cos(ang)) * (K @ K)
    site_pos = torch.rand(E, 3, dtype=torch.float64, generator=g)
    cart, quat = ik_targets_torch(site_pos, site_mat, sit_out_action(ac, alive, True), 0.5, [-1.2, -1.2, 0.0], [1.2, 1.2, 2.0])
    assert bool(torch.isfinite(cart).all()) and bool(torch.isfinite(quat).all())
    assert torch.equal(cart[~alive], site_pos[~alive])
    # (w, x, y, y) of the site's unit quaternion: w^2 + x^2 + 2 y^2 <= 2, and not the zero quaternion
    nrm = quat[~alive].norm(dim=1)
    assert bool((nrm > 1e-3).all()) and bool((nrm <= 2 ** 0.5 + 1e-12).all())
    assert torch.equal(quat[~alive][:, 2], quat[~alive][:, 3])
