"""MoPA + IK on PusherObstacle-v0 (the reference's scripts/2d/mopa_ik.sh: a 2-D Cartesian action without a quaternion, position-only IK
of the `fingertip` site), the parts that need no GPU: the CPU oracle's IK on the Pusher chain against the reference's own
`qpos_from_site_pose` (tests/golden/ref_py_ik_pusher.npz, tools/gen_ref_py_golden.py `pusher_ik`), the config the reference builds, the
numpy form of the target rule, the neutral action of an env that sits out, the C ABI's new symbols, and what the recorded rollouts
contain."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENV = "PusherObstacle-v0"

# max |deviation| of the oracle's solve from the reference's on the 48 fixture problems, as measured by
# test_oracle_ik_on_the_pusher_chain_equals_reference (which prints it), and the asserted bound: 4 x that
MEASURED = {"qpos": 5.329e-15, "err_norm": 3.331e-16}
ATOL = {k: 4 * v for k, v in MEASURED.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pusher_ik_problem():
    from mopa_rl_amd.scene import ENV_SPECS, load_scene
    m = load_scene(ENV_SPECS[ENV].scene)
    si = m.site_name2id("fingertip")
    jids = [m.joint_name2id(j) for j in ENV_SPECS[ENV].robot_joints]
    return m, si, jids


def test_oracle_ik_on_the_pusher_chain_equals_reference(oracle_mod):
    """K5's checker on a chain no other test walks -- planar, 4 hinges, joint0 unlimited, the site on a jointless leaf body --
    against the REFERENCE'S OWN `qpos_from_site_pose(env, "fingertip", target_pos, target_quat=None, joint_names=robot_joints,
    max_steps=100, tol=1e-2)` on 48 problems: `steps` and `success` identical for all 48; joint vector and error norm to round-off
    (unpivoted Cholesky against LAPACK's LU).  Measured max |deviation|: qpos 5.329e-15, err_norm 3.331e-16; asserted: 4 x that."""
    G = np.load(os.path.join(GOLD, "ref_py_ik_pusher.npz"))
    m, si, jids = _pusher_ik_problem()
    orc = oracle_mod.OracleScene(m, [], [], 0.0)
    K = len(G["pusher_qpos"])
    assert K == 48
    dq = de = 0.0
    for k in range(K):
        q, en, st, su = orc.ik_solve(G["pusher_qpos"][k], G["pusher_target_pos"][k], jids, int(m.site_body[si]), m.site_pos[si],
                                     max_steps=100, tol=1e-2)
        assert st == G["pusher_steps"][k] and su == bool(G["pusher_success"][k]), (k, st, su)
        dq = max(dq, float(np.abs(q - G["pusher_qpos_out"][k]).max()))
        de = max(de, abs(en - float(G["pusher_err_norm"][k])))
    print(f"oracle IK on the Pusher chain: max |deviation| from the reference: qpos {dq:.3e}  err_norm {de:.3e}")
    assert dq <= ATOL["qpos"] and de <= ATOL["err_norm"], (dq, de)


def test_ik_fixture_covers_seam_starts_and_all_three_kinds_of_target():
    G = np.load(os.path.join(GOLD, "ref_py_ik_pusher.npz"))
    q0, kind, st, su = G["pusher_qpos"][:, 0], G["pusher_kind"], G["pusher_steps"], G["pusher_success"]
    near_seam = 3.14 - np.abs(q0) < 0.12
    assert near_seam.sum() >= 16 and (q0[near_seam] > 0).any() and (q0[near_seam] < 0).any()
    assert (st[kind == 0] == 0).all() and (su[kind == 0] == 1).all()               # already there
    assert (su[kind == 1] == 1).sum() >= 12 and (st[kind == 1] > 0).any()          # in reach (one start is too near a singular pose)
    assert (su[kind == 2] == 0).all() and (st[kind == 2] == 99).sum() >= 4         # out of reach: never converges, some run all 100 iterations
    assert ((st[kind == 2] > 0) & (st[kind == 2] < 99)).any()                      # ... and some give up on progress
    # only the four robot joints move
    assert np.array_equal(_bits(G["pusher_qpos_out"][:, 4:]), _bits(G["pusher_qpos"][:, 4:]))


def test_rollout_config_for_the_pusher_ik_script():
    from mopa_rl_amd.rollout import RolloutConfig
    from mopa_rl_amd.scene import ENV_SPECS
    sp = ENV_SPECS[ENV]
    c = RolloutConfig.for_env(ENV, use_ik_target=True)
    assert c.use_ik_target and c.ik_target == "fingertip"
    assert tuple(c.min_world_size) == (-0.41, -0.41) and tuple(c.max_world_size) == (0.41, 0.41)
    assert c.n_cart == 2 and not c.ik_has_quat
    # the Pusher defaults it already carried
    assert (c.ac_scale, c.action_range, c.range, c.simple_planner_range, c.step_size, c.joint_margin, c.contact_threshold) == (
        sp.ac_scale, sp.action_range, sp.range, sp.simple_planner_range, sp.step_size, sp.joint_margin, sp.contact_threshold)
    assert c.ac_scale == 0.1 and c.action_range == 1.0
    # the script's own values come as overrides, and an explicit override wins over the env's IK defaults
    s = RolloutConfig.for_env(ENV, use_ik_target=True, omega=0.1, action_range=0.1)
    assert (s.omega, s.action_range, s.ik_target) == (0.1, 0.1, "fingertip")
    assert RolloutConfig.for_env(ENV, use_ik_target=True, ik_target="other").ik_target == "other"
    # nothing changes for the configurations that existed
    p = RolloutConfig.for_env(ENV)
    assert not p.use_ik_target and p.ik_target == "grip_site" and p.n_cart == 3
    a = RolloutConfig.for_env("SawyerAssemblyObstacle-v0", use_ik_target=True)
    assert a.ik_target == "grip_site" and tuple(a.min_world_size) == (-1.2, -1.2, 0.0) and tuple(a.max_world_size) == (1.2, 1.2, 2.0)
    assert a.n_cart == 3 and a.ik_has_quat


def test_numpy_target_rule_on_edge_rows():
    """`ik_targets_pos_np` (the checker of the kernel) on rows chosen by hand: inside the box, exactly at it, outside it on either
    side, and a component at or above n_cart, which is the site's own whatever the action says."""
    from mopa_rl_amd.rollout import ik_targets_pos_np
    lo2, hi2 = (-0.41, -0.41), (0.41, 0.41)
    site = np.array([[0.1, -0.2, 0.02], [0.40, -0.40, 0.02], [0.31, 0.0, 0.02], [0.0, 0.0, 0.02], [0.41, -0.41, 0.02]])
    ac = np.array([[0.5, -0.5, 9.0], [1.0, -1.0, 9.0], [1.0, 0.0, 9.0], [-5.0, 5.0, 9.0], [0.0, 0.0, 9.0]])
    got = ik_targets_pos_np(site, ac, 2, 0.1, lo2, hi2)
    want = np.array([[0.1 + 0.1 * 0.5, -0.2 + 0.1 * -0.5, 0.02], [0.41, -0.41, 0.02], [0.41, 0.0, 0.02], [-0.41, 0.41, 0.02], [0.41, -0.41, 0.02]])
    assert np.array_equal(_bits(got), _bits(want))
    # a product, then a sum: 0.31 + 0.1 * 1.0 is 0.41000000000000003 before the clip
    assert 0.31 + 0.1 * 1.0 > 0.41
    # n_cart = 3: the third component follows the action and its own bounds
    lo3, hi3 = (-1.2, -1.2, 0.0), (1.2, 1.2, 2.0)
    got3 = ik_targets_pos_np(site, ac, 3, 0.1, lo3, hi3)
    assert np.array_equal(_bits(got3[:, 2]), _bits(np.full(5, 0.02 + 0.1 * 9.0)))
    assert np.array_equal(_bits(ik_targets_pos_np(site, -ac, 3, 0.1, lo3, hi3)[:, 2]), _bits(np.zeros(5)))      # below the floor
    # the reference's two statements, word for word (rl/mopa_rollouts.py:91-98, 684-690), on random rows
    rng = np.random.default_rng(0)
    S, A = rng.uniform(-0.45, 0.45, (64, 3)), rng.uniform(-1, 1, (64, 4))
    for e in range(64):
        cart = np.clip(S[e][:2] + 0.1 * A[e][:2], list(lo2), list(hi2))
        cart = np.concatenate((cart, np.array([S[e][2]])))
        assert np.array_equal(_bits(ik_targets_pos_np(S[e:e + 1], A[e:e + 1], 2, 0.1, lo2, hi2)[0]), _bits(cart))


def test_sit_out_action_without_a_quaternion_is_all_zeros():
    import torch
    from mopa_rl_amd.rollout import sit_out_action
    ac = torch.tensor([[0.3, -0.2], [0.5, 0.6], [-1.0, 1.0]], dtype=torch.float64)
    alive = torch.tensor([True, False, True])
    got = sit_out_action(ac, alive, True, has_quat=False)
    assert torch.equal(got, torch.tensor([[0.3, -0.2], [0.0, 0.0], [-1.0, 1.0]], dtype=torch.float64))
    # with a quaternion the neutral row still carries the identity rotation (and that stays the default)
    ac7 = torch.full((2, 7), 0.25, dtype=torch.float64)
    got7 = sit_out_action(ac7, torch.tensor([False, True]), True)
    assert torch.equal(got7[0], torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)) and torch.equal(got7[1], ac7[1])


def test_new_abi_symbols_are_declared_bound_and_check_their_arguments():
    from mopa_rl_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mopa_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for sym, nargs in (("mopa_ik_targets_pos_batch", 11), ("mopa_ik_displacement_pos_batch", 21)):
        assert re.search(r"\bint %s\s*\(" % sym, hdr), f"{sym} is not declared in include/mopa_hip.h"
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
        assert len(getattr(L, sym).argtypes) == nargs
    # a null handle is a status code (MOPA_ERR_INVALID_ARG), not a crash, and needs no device
    assert L.mopa_ik_targets_pos_batch(None, 4, None, None, 2, 2, 0.1, None, None, None, None) == 1
    assert L.mopa_ik_displacement_pos_batch(None, 4, None, None, 2, 2, 0.1, None, None, 100, 1e-2, 2.0, 20.0, 3e-2, None, None, None, None,
                                            None, None, None) == 1


def test_recorded_rollouts_contain_both_kinds_of_step_and_unequal_episodes():
    R = np.load(os.path.join(GOLD, "ref_py_rollout_pusher_ik.npz"))
    assert R["ac"].shape == (32, 5, 2) and float(R["omega"]) == 0.1 and float(R["action_range"]) == 0.1
    tot = dict(zip(("mp", "rl", "interpolation", "mp_fail", "approximate", "invalid"), R["counters"].sum(axis=(0, 1))))
    assert tot["rl"] > 0 and tot["interpolation"] > 0, tot
    # a planner step of this action space never leaves the current state: two zero-motion waypoints (intra_steps 1)
    planner = R["counters"][:, :, 2] == 1
    assert (R["intra"][planner] == 1).all() and np.array_equal(_bits(R["qpos_end"][planner][:, :4]), _bits(R["qpos_start"][planner][:, :4]))
    assert (R["intra"][~planner] == 0).all()
    Ep = np.load(os.path.join(GOLD, "ref_py_episode_pusher_ik.npz"))
    assert Ep["ac"].shape[0] == 24 and Ep["ac"].shape[2] == 2
    assert len(set(Ep["ep_len"].tolist())) >= 3 and len(set(Ep["n_steps"].tolist())) >= 3
    assert Ep["counters"][:, 1].sum() > 0 and Ep["counters"][:, 2].sum() > 0
