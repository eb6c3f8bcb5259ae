"""A10 against the reference's own `SACAgent.simple_interpolate` / `SACAgent.plan` (rl/sac_agent.py:198-318), run in the
build container on the Push scene with validity + RRT-Connect supplied by the CPU oracle (tests/golden/
ref_py_agent_push.npz, tools/gen_ref_py_golden.py).  The batched forms must return the same waypoints bit for bit, the
same lengths and the same success / interpolation / valid / exact flags.

CPU leg: the batched code on CPU tensors with the oracle as validity checker (pins the host logic).  GPU leg: the
product path -- HIP validity (K1), HIP RRT-Connect (K3) -- through BatchMoPARollout.plan."""
import os

import numpy as np
import pytest

from oracle_bp import OracleBP, bits as _bits

ENV = "SawyerPushObstacle-v0"
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_py_agent_push.npz"))


def _check_si(traj, tlen, success):
    K = len(G["cur"])
    for k in range(K):
        assert int(tlen[k]) == G["si_len"][k], k
        assert bool(success[k]) == bool(G["si_flags"][k, 0]), k
        assert np.array_equal(_bits(traj[k, :tlen[k]]), _bits(G["si_traj"][k, :G["si_len"][k]])), k
    assert 0 < G["si_flags"][:, 0].sum() < K


def test_simple_interpolate_batch_equals_reference_cpu(oracle_mod):
    import torch
    from mopa_rl_amd.agent_planning import JointLimits, max_interpolation_steps, simple_interpolate_batch
    from mopa_rl_amd.scene import planner_inputs, qpos_joint_arrays
    pi = planner_inputs(ENV)
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    idx, lo, hi, lim = qpos_joint_arrays(pi.model)
    jl = JointLimits(lo[idx], hi[idx], lim[idx], pi.spec.joint_margin)
    cur = jl.clip_state(torch.tensor(G["cur"]))
    tgt = torch.tensor(G["tgt"])
    traj, tlen, success, nst = simple_interpolate_batch(OracleBP(orc), cur, tgt, 0.05, pi.ref_joint_pos_indexes)
    _check_si(traj.numpy(), tlen.numpy(), success.numpy())
    # a fixed step budget (no host read-back of the step count) gives the same rows
    fixed = max_interpolation_steps(0.5, 0.05)
    assert fixed >= int(nst.max())
    traj2, tlen2, success2, _ = simple_interpolate_batch(OracleBP(orc), cur, tgt, 0.05, pi.ref_joint_pos_indexes, fixed_steps=fixed)
    _check_si(traj2.numpy(), tlen2.numpy(), success2.numpy())


@pytest.mark.gpu
def test_plan_batch_equals_reference_gpu():
    import torch
    from mopa_rl_amd.agent_planning import simple_interpolate_batch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    timelimit, max_nodes, max_path, seed, ac_scale = G["params"]
    K = len(G["cur"])
    env = make_env(ENV, K, seed=0)
    env.reset()
    ro = BatchMoPARollout(env, RolloutConfig(timelimit=float(timelimit), max_nodes=int(max_nodes), max_path=int(max_path), seed=int(seed)))
    cur, tgt = torch.tensor(G["cur"], device="cuda"), torch.tensor(G["tgt"], device="cuda")
    v = ro._valid(tgt).cpu().numpy()
    assert np.array_equal(v.astype(np.int64), G["tgt_valid"])
    traj, tlen, success, _ = simple_interpolate_batch(ro.bp, ro.clip_qpos(cur), tgt, float(ac_scale), ro.arm)
    _check_si(traj.cpu().numpy(), tlen.cpu().numpy(), success.cpu().numpy())
    ids = torch.arange(K, device="cuda")
    traj, lens, success, interpolation, valid, exact = ro.plan(cur, tgt, ids)
    traj, lens = traj.cpu().numpy(), lens.cpu().numpy()
    F = G["plan_flags"]
    for k in range(K):
        assert (bool(success[k]), bool(valid[k]), bool(exact[k])) == (bool(F[k, 0]), bool(F[k, 2]), bool(F[k, 3])), k
        if success[k]:
            assert bool(interpolation[k]) == bool(F[k, 1]), k
            assert lens[k] == G["plan_len"][k], k
            assert np.array_equal(_bits(traj[k, :lens[k]]), _bits(G["plan_traj"][k, :lens[k]])), k
    assert (F[:, 0] & (1 - F[:, 1])).sum() >= 5 and (F[:, 2] == 0).sum() >= 5      # RRT paths and invalid goals both present


@pytest.mark.gpu
def test_straight_line_precheck_library_form_equals_tensor_form():
    """`simple_interpolate_batch` with a fixed width runs as `mopa_interpolate_batch` (three launches of the library); without
    one as tensor operations around one validity launch (the form the reference-generated vectors above pin).  Same rows,
    lengths, verdicts and step counts, bit for bit, on lines that are short, long, blocked and free."""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.agent_planning import max_interpolation_steps, simple_interpolate_batch
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import default_qpos, planner_inputs
    env = "SawyerPushObstacle-v0"
    pi = planner_inputs(env)
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range)
    bp = BatchPlanner(sc)
    E = 1500
    rng = np.random.default_rng(3)
    cur = np.repeat(default_qpos(env, pi.model)[None], E, axis=0)
    cur[:, :7] += rng.normal(0, 0.05, size=(E, 7))
    tgt = cur.copy()
    tgt[:, :7] += rng.uniform(-0.5, 0.5, size=(E, 7)) * rng.choice([0.05, 0.3, 1.0], size=(E, 1))
    tgt[:, :7] = np.clip(tgt[:, :7], pi.jnt_minimum, pi.jnt_maximum)
    c, t = torch.tensor(cur, device="cuda"), torch.tensor(tgt, device="cuda")
    K = max_interpolation_steps(0.5, 0.05)
    a = simple_interpolate_batch(bp, c, t, 0.05, list(range(7)))
    b = simple_interpolate_batch(bp, c, t, 0.05, list(range(7)), fixed_steps=K)
    torch.cuda.synchronize()
    la, lb = a[1].cpu().numpy(), b[1].cpu().numpy()
    assert np.array_equal(la, lb) and np.array_equal(a[2].cpu().numpy(), b[2].cpu().numpy()) and np.array_equal(a[3].cpu().numpy(), b[3].cpu().numpy())
    ta, tb = a[0].cpu().numpy(), b[0].cpu().numpy()
    for e in range(E):
        assert np.array_equal(ta[e, :la[e]].view(np.uint64), tb[e, :lb[e]].view(np.uint64)), e
    ok = a[2].cpu().numpy()
    assert 0.1 * E < ok.sum() < 0.95 * E and a[3].max() > 8
