"""Contact-force readout, host side (no GPU): the C ABI entry, the row decode / sum of tests/contact_force_ref.py by hand, the envs
`enable_contact_force` refuses, and the K8 reference on the two committed contact states of tests/test_pusher_dyn_host.py."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two committed contact states of tests/test_pusher_dyn_host.py (dofs joint0..3, box_x, box_y)
Q_TIP_IN_BOX = [0.0, 0.0, 0.0, math.pi / 2, 0.3, 0.11 + 0.02 - 0.002]          # = [0, 0, 0, pi/2, 0.3, 0.128]: 2 contacts
Q_BOX_IN_OBSTACLE = [0.0, 0.0, 0.0, 0.0, -0.12 + 0.02 - 0.002, -0.12]          # = [0, 0, 0, 0, -0.102, -0.12]: 4 contacts


@pytest.fixture(scope="module")
def facts():
    from mopa_rl_amd.dynamics import pusher_dyn_facts
    from mopa_rl_amd.scene import ENV_SPECS, load_scene
    return pusher_dyn_facts(load_scene(ENV_SPECS["PusherObstacle-v0"].scene))


def test_abi_symbol_is_declared_and_bound():
    from mopa_rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    assert re.search(r"\bmopa_env_set_contact_force\s*\(", hdr)
    assert "mopa_env_set_contact_force" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    fn = getattr(L, "mopa_env_set_contact_force")
    assert len(fn.argtypes) == 6
    # a null env is a status code, not a crash
    assert fn(None, None, None, None, None, 0) == 1         # MOPA_ERR_INVALID_ARG


def test_decode_reproduces_fn_f1_f2_by_hand():
    """two pyramidal contacts with binary-exact edge forces: Fn = sum of the edges, F1 = mu (p0 - p1), F2 = mu (p2 - p3)"""
    from contact_force_ref import decode_pyramid, force_of_rows, pyramid_rows, row_sum
    p_a, mu_a = [1.0, 0.5, 0.25, 0.25], 0.5
    p_b, mu_b = [0.0, 2.0, 0.75, 0.125], 2.0
    assert decode_pyramid(p_a, mu_a) == (2.0, 0.25, 0.0)
    assert decode_pyramid(p_b, mu_b) == (2.875, -4.0, 1.25)
    rows = pyramid_rows([7, 3], [11, 12], [p_a, p_b], [mu_a, mu_b])
    assert rows.shape == (2, 8)
    assert list(rows[0]) == [7.0, 11.0, 2.0, 0.25, 0.0, 0.0, 0.0, 0.0]
    assert list(rows[1]) == [3.0, 12.0, 2.875, -4.0, 1.25, 0.0, 0.0, 0.0]
    assert row_sum(rows[0][2:]) == 2.25 and row_sum(rows[1][2:]) == 8.125          # |.|: the negative tangential force counts
    assert force_of_rows(rows) == 10.375
    assert force_of_rows(np.zeros((0, 8))) == 0.0
    # an elliptic row (condim 4, zero-padded) goes through the same sum
    assert row_sum([3.0, -1.0, 0.5, -0.25, 0.0, 0.0]) == 4.75


def test_sum_order_is_left_to_right():
    """the sum is the plain left-to-right chain: values chosen so that another association gives other bits"""
    from contact_force_ref import force_of_rows, row_sum
    f = [1.0, 2.0 ** -53, 2.0 ** -53, 0.0, 0.0, 0.0]
    assert row_sum(f) == 1.0 and (f[1] + f[2]) + f[0] != 1.0
    rows = np.zeros((3, 8))
    rows[:, 2] = [1.0, 2.0 ** -53, 2.0 ** -53]
    assert force_of_rows(rows) == 1.0


def test_enable_contact_force_refuses_envs_without_a_contact_solver():
    """kinematic, servo dynamics alone (K6) and the penalty-contact object: the option path decides before any device call"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.kinematic_env import BatchKinematicEnv
    for dynamics, dyn_lanes, what in ((False, 1, "kinematic"), (True, 1, "K6 / contacts='penalty'")):
        env = object.__new__(BatchKinematicEnv)
        env.pdyn, env.dynamics, env.dyn_lanes, env.ct, env._h, env._scene = None, dynamics, dyn_lanes, None, None, None
        env.contact_force = env.contact_force_total = env.contact_count = env.contact_rows = None
        assert not env.has_contact_solver(), what
        assert env.contact_maxcon == 0
        with pytest.raises(_lib.MopaError):
            env.enable_contact_force()
        with pytest.raises(_lib.MopaError):
            env.enable_contact_force(rows=True)
        env.disable_contact_force()         # off stays off, without a library call


@pytest.mark.parametrize("q,count", [(Q_TIP_IN_BOX, 2), (Q_BOX_IN_OBSTACLE, 4)])
def test_pusher_reference_on_the_committed_contact_states(facts, q, count):
    from contact_force_ref import PusherForceRef, force_of_rows
    ref = PusherForceRef(facts)
    # one forward pass at rest
    ref.forward(list(q), [0.0] * 6, [0.0] * 4)
    rows = ref.rows()
    assert rows.shape == (count, 8)
    assert force_of_rows(rows) > 0.0
    assert (rows[:, 2] >= 0.0).all() and (rows[:, 5:] == 0.0).all()
    assert (rows[:, 1] < 0.0).all()                                  # key: the signed distance of a penetrating contact
    C, F = ref.last
    assert [int(r) for r in rows[:, 0]] == [c["pair"] for c in C]
    # the normal force is the sum of the four edge forces, which are >= 0
    for r, fr in zip(rows, F):
        assert all(x >= 0.0 for x in fr) and abs(r[2] - sum(fr)) <= 4 * np.spacing(r[2])
    # ... and through the sub-step entry: the last forward pass of 3 sub-steps (its 4th RK4 stage) still has these contacts
    rows3, force3 = ref.readout(q, [0.0] * 6, [0.0] * 4, q[:4], q[:4], 3)
    assert rows3.shape == (count, 8) and force3 > 0.0 and (rows3[:, 2] >= 0.0).all()
    assert force3 == force_of_rows(rows3)


def test_forward_returns_what_the_caller_asked_for(facts):
    """the subclass changes nothing of the checker: qacc alone without `want`, the triple with it, same bits as PusherRef"""
    from contact_force_ref import PusherForceRef
    from pusher_dyn_ref import PusherRef
    a, b = PusherForceRef(facts), PusherRef(facts)
    qa = a.forward(list(Q_TIP_IN_BOX), [0.0] * 6, [0.0] * 4)
    assert isinstance(qa, list) and qa == b.forward(list(Q_TIP_IN_BOX), [0.0] * 6, [0.0] * 4)
    t = a.forward(list(Q_TIP_IN_BOX), [0.0] * 6, [0.0] * 4, want=True)
    assert len(t) == 3 and t[0] == qa and t[2] == b.forward(list(Q_TIP_IN_BOX), [0.0] * 6, [0.0] * 4, want=True)[2]
