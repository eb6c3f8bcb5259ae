"""MoPA + IK on PusherObstacle-v0 (the reference's scripts/2d/mopa_ik.sh) on the GPU: K5 on the Pusher chain against the CPU oracle,
the position-only target kernel against its numpy form, the fused pre-step `displacement_pos` against the composition of the separate
launches, its argument checks, and the batched rollout against the reference's own runner (tests/golden/ref_py_rollout_pusher_ik.npz,
ref_py_episode_pusher_ik.npz; tools/gen_ref_py_golden.py `pusher_ik`)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = "PusherObstacle-v0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
# the script's own values (scripts/2d/mopa_ik.sh), which the fixtures were recorded with
SCRIPT = {"use_ik_target": True, "omega": 0.1, "action_range": 0.1}

# max |deviation| of a re-loaded agent step / of a free-running episode from the reference's, as measured on an MI355X by the two rollout
# tests below (which print it), and the asserted bounds: 4 x that.  A quantity that came out identical is asserted identical.
STEP_MEASURED = {"qpos": 2.220e-15, "rew": 0.0, "ob_next": 2.054e-15}
EPISODE_MEASURED = {"qpos_final": 3.109e-15, "ob": 2.554e-15, "rew": 0.0, "ep_rew": 0.0}
STEP_ATOL = {k: 4 * v for k, v in STEP_MEASURED.items()}
EPISODE_ATOL = {k: 4 * v for k, v in EPISODE_MEASURED.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def pusher():
    """the compiled Pusher model, its IK handle (site fingertip, the four robot joints), the oracle, and 65 start states -- one full
    wave and a one-lane tail --: 16 next to the seam of joint0, the others anywhere"""
    import torch
    from mopa_rl_amd.ik import BatchIK
    from mopa_rl_amd.kinematic_env import env_facts
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    O.build()
    pi = planner_inputs(ENV)
    m = pi.model
    ik = BatchIK(m, "fingertip", pi.spec.robot_joints, device=0)
    orc = O.OracleScene(m, [], [], 0.0)
    f = env_facts(ENV, m)
    rng = np.random.default_rng(17)
    E = 65
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (E, 1))
    q[:, 0] = rng.uniform(-3.0, 3.0, E)
    q[:16, 0] = rng.choice([-1.0, 1.0], 16) * rng.uniform(3.02, 3.13, 16)
    q[:, 1:4] = rng.uniform(-2.5, 2.5, (E, 3))
    q[:, 4:] += rng.uniform(-0.02, 0.02, (E, q.shape[1] - 4))
    dev = torch.device("cuda", 0)
    lo = torch.tensor(f.qpos_min[:4], dtype=torch.float64, device=dev)
    hi = torch.tensor(f.qpos_max[:4], dtype=torch.float64, device=dev)
    assert float(lo[0]) == -3.14 and float(hi[0]) == 3.14            # env/base.py:85-86: the unlimited joint0 carries +-3.14
    yield {"m": m, "ik": ik, "orc": orc, "q": q, "lo": lo, "hi": hi, "dev": dev, "rng": rng}
    ik.close()


def _site_np(P, q):
    """site positions of the rows of q from the GPU's own site-pose launch (the oracle pins it elsewhere)"""
    import torch
    pos, _ = P["ik"].site_pose(torch.tensor(q, device=P["dev"]))
    return pos.cpu().numpy()


def test_k5_on_the_pusher_chain_is_the_oracle_bit_for_bit(pusher):
    """Position-only solves of 65 problems on the planar 4-hinge chain (joint0 unlimited, the site on a jointless leaf body): targets
    already there, in reach and out of reach.  qpos, err_norm, steps and success are the CPU oracle's, bit for bit."""
    import torch
    P = pusher
    q, E = P["q"], len(P["q"])
    rng = np.random.default_rng(3)
    site = _site_np(P, q)
    tgt = site.copy()
    kind = np.arange(E) % 3
    tgt[kind == 0, :2] += rng.uniform(-0.004, 0.004, ((kind == 0).sum(), 2))
    tgt[kind == 1, :2] += rng.uniform(-0.06, 0.06, ((kind == 1).sum(), 2))
    ang = rng.uniform(-np.pi, np.pi, (kind == 2).sum())
    tgt[kind == 2, 0], tgt[kind == 2, 1] = 0.8 * np.cos(ang), 0.8 * np.sin(ang)
    qd = torch.tensor(q, device=P["dev"])
    res = P["ik"].solve(qd, torch.tensor(tgt, device=P["dev"]), None, max_steps=100, tol=1e-2)
    got_q, got_e, got_s, got_ok = res.qpos.cpu().numpy(), res.err_norm.cpu().numpy(), res.steps.cpu().numpy(), res.success.cpu().numpy()
    ik = P["ik"]
    for e in range(E):
        oq, oe, os_, ook = P["orc"].ik_solve(q[e], tgt[e], ik.joint_ids, ik.site_body, ik.site_off, max_steps=100, tol=1e-2)
        assert int(got_s[e]) == os_ and bool(got_ok[e]) == bool(ook), (e, int(got_s[e]), os_)
        assert np.array_equal(_bits(got_q[e]), _bits(oq)), e
        assert _bits(got_e[e]) == _bits(oe), e
    assert (got_s[kind == 0] == 0).all() and got_ok[kind == 1].all() and not got_ok[kind == 2].any() and (got_s == 99).any()


@pytest.mark.parametrize("n_cart", [2, 3])
def test_targets_pos_is_the_numpy_form_bit_for_bit(pusher, n_cart):
    import torch
    from mopa_rl_amd.rollout import ik_targets_pos_np
    P = pusher
    rng = np.random.default_rng(5 + n_cart)
    E = 65
    lo, hi = ((-0.41, -0.41), (0.41, 0.41)) if n_cart == 2 else ((-0.41, -0.41, 0.0), (0.41, 0.41, 0.05))
    site = rng.uniform(-0.45, 0.45, (E, 3))
    site[:, 2] = rng.uniform(-0.02, 0.07, E)
    big = rng.uniform(-1, 1, (E, 9))                  # the action sits in columns 2 .. of wider rows: ac_stride 9
    site[0, :2], big[0, 2:4] = (0.41, -0.41), (0.0, 0.0)         # exactly at the box
    site[1, :2], big[1, 2:4] = (0.31, 0.0), (1.0, 0.0)           # 0.31 + 0.1 * 1.0 = 0.41000000000000003: clipped
    site[2, :2], big[2, 2:4] = (0.44, -0.44), (1.0, -1.0)        # outside on both
    bd = torch.tensor(big, device=P["dev"])
    ac = bd[:, 2:2 + 4]
    assert ac.stride(0) == 9 and ac.stride(1) == 1
    got = P["ik"].targets_pos(torch.tensor(site, device=P["dev"]), ac, n_cart, 0.1, lo, hi).cpu().numpy()
    want = ik_targets_pos_np(site, big[:, 2:6], n_cart, 0.1, lo, hi)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[:, n_cart:]), _bits(site[:, n_cart:]))      # components at or above n_cart: the site's own
    assert (got[:, :2] == 0.41).any() and (got[:, :2] == -0.41).any() and (np.abs(got[:, :2]) < 0.41).any()


def _composition(P, qd, ac, n_cart, ar, wlo, whi):
    """site_pose -> targets_pos -> solve -> clamp -> sub, as separate launches"""
    import torch
    ik = P["ik"]
    site_pos, _ = ik.site_pose(qd)
    tgt = ik.targets_pos(site_pos, ac, n_cart, ar, wlo, whi)
    q2 = qd.clone()
    res = ik.solve(q2, tgt, None, max_steps=100, tol=1e-2)
    arm = torch.minimum(torch.maximum(q2[:, :4], P["lo"]), P["hi"])
    return arm - qd[:, :4], res, arm, q2


@pytest.mark.parametrize("E", [65, 1])
def test_displacement_pos_is_the_composition_of_the_separate_launches(pusher, E):
    """The fused pre-step against site_pose -> targets_pos -> solve -> clamp -> subtract: displacement, err_norm, steps and success
    bit for bit -- rows that stop at once, rows that converge, rows that run all 100 iterations, rows whose joint0 meets the +-3.14
    clip -- and the input qpos untouched.  (A world box wider than the env's, so that targets out of the arm's reach exist.)"""
    import torch
    P = pusher
    rng = np.random.default_rng(23)
    q = P["q"][:E] if E > 1 else P["q"][2:3]
    qd = torch.tensor(q, device=P["dev"])
    keep = qd.clone()
    ac = rng.uniform(-1, 1, (E, 2)) * np.array([0.004, 0.06, 1.0])[np.arange(E) % 3][:, None]
    if E == 1:
        ac[:] = (0.9, -0.8)
    acd = torch.tensor(ac, device=P["dev"])
    wlo, whi = (-0.9, -0.9), (0.9, 0.9)
    want, res, arm, q2 = _composition(P, qd, acd, 2, 1.0, wlo, whi)
    got, r = P["ik"].displacement_pos(qd, acd, 2, 1.0, wlo, whi, P["lo"], P["hi"], want_result=True)
    torch.cuda.synchronize()
    assert torch.equal(qd, keep), "displacement_pos wrote its input"
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))
    assert torch.equal(r.steps, res.steps) and torch.equal(r.success, res.success)
    assert np.array_equal(_bits(r.err_norm.cpu().numpy()), _bits(res.err_norm.cpu().numpy()))
    # without the optional outputs: the same displacement
    assert torch.equal(P["ik"].displacement_pos(qd, acd, 2, 1.0, wlo, whi, P["lo"], P["hi"]), got)
    st = res.steps.cpu().numpy()
    if E > 1:
        assert (st == 0).any() and (st == 99).any() and ((st > 0) & (st < 99)).any()
        assert bool((arm != q2[:, :4]).any()), "no row met the joint clip"
        # the env's own box (what the rollout passes), n_cart 3 as well: still the composition
        for n_cart, lo_w, hi_w in ((2, (-0.41, -0.41), (0.41, 0.41)), (3, (-0.41, -0.41, 0.0), (0.41, 0.41, 0.05))):
            ac3 = torch.tensor(rng.uniform(-1, 1, (E, 3)), device=P["dev"])
            w2, _, _, _ = _composition(P, qd, ac3, n_cart, 0.1, lo_w, hi_w)
            g2 = P["ik"].displacement_pos(qd, ac3, n_cart, 0.1, lo_w, hi_w, P["lo"], P["hi"])
            assert np.array_equal(_bits(g2.cpu().numpy()), _bits(w2.cpu().numpy())), n_cart
    else:
        assert int(st[0]) > 0


def test_argument_errors_are_status_codes_and_nothing_is_launched(pusher):
    import torch
    from mopa_rl_amd import _lib
    P = pusher
    L, h = _lib.lib(), P["ik"]._h
    E = 8
    dev = P["dev"]
    qd = torch.tensor(P["q"][:E], device=dev)
    ac = torch.zeros(E, 2, dtype=torch.float64, device=dev)
    site = torch.zeros(E, 3, dtype=torch.float64, device=dev)
    sentinel = -777.0
    cart = torch.full((E, 3), sentinel, dtype=torch.float64, device=dev)
    disp = torch.full((E, 4), sentinel, dtype=torch.float64, device=dev)
    lo, hi = (C.c_double * 3)(-0.41, -0.41, 0.0), (C.c_double * 3)(0.41, 0.41, 0.0)
    p = lambda t: t.data_ptr()

    def targets(E_=E, site_=p(site), ac_=p(ac), stride=2, n_cart=2, lo_=lo, hi_=hi, out=p(cart)):
        return L.mopa_ik_targets_pos_batch(h, E_, site_, ac_, stride, n_cart, 0.1, lo_, hi_, out, None)

    def displacement(E_=E, q_=p(qd), ac_=p(ac), stride=2, n_cart=2, lo_=lo, hi_=hi, max_steps=100, jlo=p(P["lo"]), jhi=p(P["hi"]), out=p(disp)):
        return L.mopa_ik_displacement_pos_batch(h, E_, q_, ac_, stride, n_cart, 0.1, lo_, hi_, max_steps, 1e-2, 2.0, 20.0, 3e-2, jlo, jhi, out,
                                                None, None, None, None)

    INVALID = 1
    for fn in (targets, displacement):
        assert fn(n_cart=1) == INVALID and fn(n_cart=4) == INVALID and fn(n_cart=0) == INVALID
        assert fn(E_=-1) == INVALID
        assert fn(stride=1) == INVALID and fn(n_cart=3, stride=2) == INVALID
        assert fn(ac_=None) == INVALID and fn(out=None) == INVALID and fn(lo_=None) == INVALID and fn(hi_=None) == INVALID
        assert _lib.lib().mopa_last_error()
    assert targets(site_=None) == INVALID
    assert displacement(q_=None) == INVALID and displacement(jlo=None) == INVALID and displacement(jhi=None) == INVALID
    assert displacement(max_steps=0) == INVALID
    torch.cuda.synchronize()
    assert bool((cart == sentinel).all()) and bool((disp == sentinel).all()), "a refused call launched"
    # E = 0 is fine and launches nothing; then the real thing
    assert targets(E_=0) == 0 and displacement(E_=0) == 0
    assert targets() == 0 and displacement() == 0
    torch.cuda.synchronize()
    assert bool((cart != sentinel).all()) and bool((disp != sentinel).all())
    # the Python wrappers refuse what the library would
    with pytest.raises(_lib.MopaError):
        P["ik"].targets_pos(site, ac, 4, 0.1, (0, 0, 0, 0), (1, 1, 1, 1))
    with pytest.raises(_lib.MopaError):
        P["ik"].displacement_pos(qd, ac[:, :1], 2, 0.1, (-1, -1), (1, 1), P["lo"], P["hi"])


def _make(G, E, **kw):
    from test_gpu_rollout import _make as make
    assert float(G["omega"]) == SCRIPT["omega"] and float(G["action_range"]) == SCRIPT["action_range"]
    return make(G, E, ENV, **SCRIPT, **kw)


def test_pusher_ik_agent_step_equals_reference_runner():
    """`agent_step` under scripts/2d/mopa_ik.sh's action space -- a 2-D Cartesian displacement of the fingertip, no quaternion,
    position-only IK, omega 0.1, action_range 0.1 -- against the reference's `MoPARolloutRunner.run` on PusherObstacle-v0
    (tests/golden/ref_py_rollout_pusher_ik.npz: 32 envs x 5 steps, each re-loaded from the fixture's state).  done, intra_steps and the
    six counters are identical; a planner step never moves `target_qpos` off `curr_qpos`, so it executes two zero-motion waypoints
    and `reuse_transitions` has nothing to relabel.  Joint states, rewards and observations: without a quaternion there is no
    float32 rotation matrix on the way, so they agree to the IK's round-off (Cholesky against LAPACK's LU), not Assembly's 1e-7.
    Measured max |deviation| on an MI355X:  qpos 2.220e-15   rew 0 (identical)   ob_next 2.054e-15;  asserted: 4 x that."""
    import torch
    from mopa_rl_amd.rollout import COUNTERS
    from test_gpu_rollout import _load_state
    G = np.load(os.path.join(GOLD, "ref_py_rollout_pusher_ik.npz"))
    E, T = G["ac"].shape[:2]
    env, ro = _make(G, E)
    assert ro.ac_dim == 2 and ro.cfg.ik_target == "fingertip" and ro.cfg.n_cart == 2
    dev_max = {"qpos": 0.0, "rew": 0.0, "ob_next": 0.0}
    flags_ok = True
    outs = []
    for t in range(T):
        _load_state(env, G["qpos_start"][:, t], G["ep_len_start"][:, t])
        before = {k: ro.counters[k].clone() for k in COUNTERS}
        ro.t = t
        out = ro.agent_step(torch.tensor(G["ac"][:, t], device=env.device), record=True)
        assert int(out["record"]["n_exec"].max()) <= 2 and ro.reuse_transitions(out, np.random.RandomState(0)) == []
        got_c = np.stack([(ro.counters[k] - before[k]).cpu().numpy() for k in COUNTERS], axis=1)
        ob_n, ob_n_want = out["ob_next"].cpu().numpy().copy(), G["ob_next"][:, t].copy()
        for a in (ob_n, ob_n_want):        # (the reset's joint / box velocities, which the kinematic env does not carry: see test_gpu_rollout.py)
            a[:, 10:16] = 0.0
        outs.append((env.qpos.cpu().numpy(), out["rew"].cpu().numpy(), ob_n, ob_n_want, out["done"].cpu().numpy().astype(np.int64),
                     out["intra_steps"].cpu().numpy(), got_c))
        dev_max["qpos"] = max(dev_max["qpos"], float(np.abs(outs[-1][0] - G["qpos_end"][:, t]).max()))
        dev_max["rew"] = max(dev_max["rew"], float(np.abs(outs[-1][1] - G["rew"][:, t]).max()))
        dev_max["ob_next"] = max(dev_max["ob_next"], float(np.abs(ob_n - ob_n_want).max()))
    print("agent_step, Pusher + IK: max |deviation| from the reference:", {k: f"{v:.3e}" for k, v in dev_max.items()})
    for t, (qpos, rew, ob_n, ob_n_want, done, intra, got_c) in enumerate(outs):
        assert np.array_equal(done, G["done"][:, t]), f"step {t}: done"
        assert np.array_equal(intra, G["intra"][:, t]), f"step {t}: intra_steps"
        assert np.array_equal(got_c, G["counters"][:, t]), f"step {t}: counters"
        np.testing.assert_allclose(qpos, G["qpos_end"][:, t], rtol=0, atol=STEP_ATOL["qpos"], err_msg=f"step {t}: qpos")
        np.testing.assert_allclose(rew, G["rew"][:, t], rtol=0, atol=STEP_ATOL["rew"], err_msg=f"step {t}: reward")
        np.testing.assert_allclose(ob_n, ob_n_want, rtol=0, atol=STEP_ATOL["ob_next"], err_msg=f"step {t}: ob_next")
    tot = dict(zip(COUNTERS, G["counters"].sum(axis=(0, 1))))
    assert tot["rl"] > 0 and tot["interpolation"] > 0, tot
    env.close(); ro.close()


def test_pusher_ik_run_episode_equals_reference_evaluation_loop():
    """`run_episode` under the same action space against the reference's own `run_episode` (tests/golden/ref_py_episode_pusher_ik.npz):
    24 envs, episode counters started at 0 / 3 / 6 / 9 so that the time cap ends them after 14, 11, 8 or 5 env steps, free-running.
    Identical: agent steps per episode, episode length, the six counters, the valid mask, done flags, success, and -- after the loop --
    the state every finished env was left in (an env that sits out gets an all-zero action: there is no quaternion to normalise).
    Measured max |deviation| on an MI355X:  qpos_final 3.109e-15   ob 2.554e-15   rew 0   ep_rew 0 (identical);  asserted: 4 x that."""
    import torch
    from mopa_rl_amd.rollout import COUNTERS
    from test_gpu_rollout import _episode_policy, _load_state
    G = np.load(os.path.join(GOLD, "ref_py_episode_pusher_ik.npz"))
    E, T = G["ac"].shape[:2]
    env, ro = _make(G, E)
    assert ro.ac_dim == 2
    _load_state(env, G["qpos_start"][:, 0], G["ep_len_start"])
    policy, calls = _episode_policy(G, env)
    rollout, info = ro.run_episode(policy, reset=False)
    n = G["n_steps"]
    valid = rollout["valid"].cpu().numpy().T
    Tn = valid.shape[1]
    ob = rollout["ob"].cpu().numpy().copy()
    ob_want, ob_final_want = G["ob"].copy(), G["ob_final"].copy()
    for a in (ob, ob_want, ob_final_want):           # (the reset's velocities again)
        a[..., 10:16] = 0.0
    same_shape = Tn == int(n.max()) and np.array_equal(valid, np.arange(Tn)[None, :] < n[:, None])
    # The reference's evaluation loop also parks every planner step's target in the four `-goal` indicator joints -- the translucent arm
    # its renderer draws (`env.visualize_goal_indicator`, rl/mopa_rollouts.py:514; qpos 4..7, passive, in no obs and no reward).  The
    # batched loop has no renderer and leaves them alone: the final joint state is compared without them.
    m = env.model
    shown = np.array([not m.jnt_names[j].endswith("-goal") for j in range(len(m.jnt_names))])[np.argsort(np.asarray(m.jnt_qposadr))]
    assert shown.sum() == 12 and not shown[4:8].any()
    q_final, q_final_want = rollout["qpos_final"].cpu().numpy()[:, shown], G["qpos_final"][:, shown]
    if same_shape:
        dev = {"qpos_final": np.abs(q_final - q_final_want).max(),
               "ob": max(np.abs(ob[:Tn].transpose(1, 0, 2)[valid] - ob_want[:, :Tn][valid]).max(), np.abs(ob[n, np.arange(E)] - ob_final_want).max()),
               "rew": np.abs(rollout["rew"].cpu().numpy().T[valid] - G["rew"][:, :Tn][valid]).max(),
               "ep_rew": np.abs(info["rew"].cpu().numpy() - G["ep_rew"]).max()}
        print("run_episode, Pusher + IK: max |deviation| from the reference:", {k: f"{v:.3e}" for k, v in dev.items()})
    assert np.array_equal(rollout["n_steps"].cpu().numpy(), n), "agent steps per episode"
    assert calls["t"] == int(n.max()) and same_shape
    assert len(set(n.tolist())) >= 3
    assert np.array_equal(info["len"].cpu().numpy(), G["ep_len"]), "episode length"
    assert np.array_equal(np.stack([info[k].cpu().numpy() for k in COUNTERS], axis=1), G["counters"]), "counters"
    assert np.array_equal(rollout["done"].cpu().numpy().T.astype(np.int64)[valid], G["done"][:, :Tn][valid]), "done flags"
    assert np.array_equal(info["success"].cpu().numpy().astype(np.int64), G["ep_success"]), "success"
    tol = EPISODE_ATOL
    np.testing.assert_allclose(q_final, q_final_want, rtol=0, atol=tol["qpos_final"], err_msg="final joint state")
    np.testing.assert_allclose(ob[:Tn].transpose(1, 0, 2)[valid], ob_want[:, :Tn][valid], rtol=0, atol=tol["ob"], err_msg="obs before each step")
    np.testing.assert_allclose(ob[n, np.arange(E)], ob_final_want, rtol=0, atol=tol["ob"], err_msg="final obs")
    np.testing.assert_allclose(rollout["rew"].cpu().numpy().T[valid], G["rew"][:, :Tn][valid], rtol=0, atol=tol["rew"], err_msg="per-step rewards")
    np.testing.assert_allclose(info["rew"].cpu().numpy(), G["ep_rew"], rtol=0, atol=tol["ep_rew"], err_msg="episode reward")
    # what the loop leaves behind: every env in the state its own episode ended in, finite, none waiting for a planner.  (No second
    # episode from a fresh reset on these actions: they were scripted for the fixture's states, and a planner step of this action
    # space from a state the planner calls invalid is undefined in the reference -- its back-off divides by |curr - target| = 0.)
    assert bool(torch.isfinite(env.qpos).all()) and bool(torch.isfinite(env.obs).all())
    for name, d in (("rollout", rollout), ("ep_info", info)):
        for k, v in d.items():
            assert bool(torch.isfinite(v.to(torch.float64)).all()), f"{name}[{k}]"
    assert torch.equal(env.qpos, rollout["qpos_final"]), "a sitting-out env left the state its episode ended in"
    assert torch.equal(env.obs, rollout["ob"][rollout["n_steps"], torch.arange(E, device=env.device)])
    assert not bool(ro.busy.any())
    env.close(); ro.close()


def test_pusher_ik_rollout_on_the_dynamics_env():
    """The K8 env (`dynamics=True, contacts=True`: PID loop, RK4, box contacts -- unpinned against MuJoCo like everything on K8) takes
    the same rollout: 64 envs, three `agent_step` calls with fixed actions.  Outputs are finite, every env's agent step lands in exactly
    one of the counters mp / rl / interpolation / mp_fail, and a second identical run gives the same bits."""
    import torch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import COUNTERS, BatchMoPARollout, RolloutConfig
    E, T = 64, 3
    rng = np.random.default_rng(31)
    AC = rng.uniform(-1, 1, size=(T, E, 2)) * rng.choice([0.05, 0.3, 1.0], size=(T, E, 1))
    runs = []
    for _ in range(2):
        env = make_env(ENV, E, dynamics=True, contacts=True, seed=6, max_episode_steps=150)
        env.reset()
        ro = BatchMoPARollout(env, RolloutConfig.for_env(ENV, timelimit=0.1, max_nodes=512, max_path=64, num_trials=10, **SCRIPT))
        assert ro.ac_dim == 2
        rows = []
        for t in range(T):
            out = ro.agent_step(torch.tensor(AC[t], device=env.device))
            for k in ("rew", "ob", "ob_next"):
                assert bool(torch.isfinite(out[k]).all()), (t, k)
            assert bool(torch.isfinite(env.qpos).all()) and bool(torch.isfinite(env.qvel).all())
            rows.append(np.concatenate([out["rew"].cpu().numpy()[:, None], out["done"].cpu().numpy()[:, None].astype(np.float64),
                                        out["intra_steps"].cpu().numpy()[:, None].astype(np.float64), env.qpos.cpu().numpy(),
                                        env.qvel.cpu().numpy(), out["ob_next"].cpu().numpy()], axis=1))
        cnt = {k: int(ro.counters[k].sum()) for k in COUNTERS}
        assert cnt["mp"] + cnt["rl"] + cnt["interpolation"] + cnt["mp_fail"] == E * T, cnt
        assert cnt["rl"] > 0
        runs.append((np.array(rows), cnt))
        env.close(); ro.close()
    assert runs[0][1] == runs[1][1]
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
