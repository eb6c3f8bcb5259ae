"""The servo dynamics off the Sawyer, on the CPU: the oracle (oracle/mopa_oracle_dyn.inc) over the lumped DynFacts of random and directed
body trees (tests/random_dyn.py) against the independent Jacobian reference over the UN-lumped model (tests/dyn_ref.py), what the host
compiler of the dynamics tables (mopa_dyn_tables_host) accepts and refuses, and the energy bookkeeping of a free-swinging branching tree."""
import copy
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_ref  # noqa: E402
import random_dyn as RD  # noqa: E402

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_LIMIT = 1, 2, 4


@pytest.mark.parametrize("key", RD.ALL_CASES)
def test_oracle_matches_the_jacobian_reference_on_the_unlumped_model(oracle_mod, key):
    """M and the bias force at 6 states, with the bounds of test_oracle_dyn.py; M exactly symmetric; lumping conserves mass"""
    c = RD.case(key)
    m, d = c.model, c.dyn
    od = oracle_mod.OracleDyn(d)
    sub = dyn_ref.subtree_bodies(m, int(d.body[0]))
    assert sorted(sub) == sorted(c.tree) and abs(d.mass.sum() - m.body_mass[sub].sum()) < 1e-12
    assert d.gravity[0] != 0.0 and d.gravity[1] != 0.0 and d.gravity[2] == -9.81
    q, v = RD.states(c, 6, seed=3)
    for e in range(6):
        bias, M = od.forward(q[e], v[e])
        Mr, _ = dyn_ref.mass_matrix(m, q[e], list(d.body), d.armature)
        br = dyn_ref.bias_force(m, q[e], v[e], list(d.body), list(d.qadr), d.armature)
        assert np.array_equal(M, M.T)
        assert np.abs(M - Mr).max() < 1e-11 * max(1.0, np.abs(Mr).max()), (key, e, np.abs(M - Mr).max())
        assert np.abs(bias - br).max() < 2e-6 * max(1.0, np.abs(br).max()), (key, e, np.abs(bias - br).max())
        assert np.linalg.eigvalsh(M).min() > 0.0


def test_the_arm_is_a_real_permutation_of_the_dofs():
    """the arm starts at the root's dof and is not in dof order on the trees that have a choice; the other dofs are neither actuated nor
    gravity-compensated"""
    shuffled = 0
    for key in RD.ALL_CASES:
        c = RD.case(key)
        d, f = c.dyn, c.facts
        arm_dof = [int(np.where(d.qadr == a)[0][0]) for a in f.arm_qpos_idx]
        assert arm_dof[0] == 0 and len(set(arm_dof)) == len(arm_dof) <= 7
        assert list(np.where(d.actuated == 1)[0]) == sorted(arm_dof) == list(np.where(d.gravcomp == 1)[0])
        assert d.nd < 3 or len(arm_dof) < d.nd
        shuffled += int(arm_dof != sorted(arm_dof))
    assert shuffled >= len(RD.ALL_CASES) // 2


def test_tables_accept_every_tree_and_tell_the_directed_ones_apart():
    want = dict(chain9=0, slot_reuse=2, three_saves=3, star=1, one_hinge=0, one_slide=0)
    prints = {}
    for key in RD.ALL_CASES:
        c = RD.case(key)
        rc, text, fp, ns = RD.tables(c)
        assert rc == 0 and ns == c.n_save <= 3, (key, rc, text, ns)
        if key in want:
            assert ns == want[key], key
        if key in RD.DIRECTED:
            prints[key] = fp
    assert RD.case("welded_inside").n_save >= 1
    assert len(set(prints.values())) == len(RD.DIRECTED), prints
    assert RD.reuses_a_slot(RD.case("slot_reuse").dyn.parent) and RD.reuses_a_slot(RD.case("three_saves").dyn.parent)
    assert not RD.reuses_a_slot(RD.case("star").dyn.parent) and not RD.reuses_a_slot(RD.case("chain9").dyn.parent)


def test_random_trees_cover_the_shapes_the_sawyer_never_showed():
    cases = [RD.case(s) for s in RD.DYN_SEEDS]
    assert all(2 <= c.dyn.nd <= 9 and c.n_save <= 3 for c in cases)
    assert sum(RD.reuses_a_slot(c.dyn.parent) for c in cases) >= 3          # two bodies with the same save[] value
    assert {c.n_save for c in cases} >= {1, 2}
    assert any(len(c.tree) > c.dyn.nd for c in cases)                       # jointless bodies inside
    slide_with_children = 0
    for c in cases:
        d = c.dyn
        slide_with_children += int(any(d.jtype[p] == RD.JNT_SLIDE for p in d.parent if p >= 0))
    assert slide_with_children >= 1


# ---------------- energy bookkeeping on a tree that reuses a save slot ----------------
def _energy_run(oracle_mod, m, d, q0, n=200, timestep=None):
    """test_oracle_dyn.test_energy_bookkeeping_without_servo_or_damping: (e0, e1, final kinetic energy) of n free sub-steps from rest"""
    d2 = copy.copy(d)
    if timestep is not None:
        d2.timestep = float(timestep)
    d2.damping = np.zeros(d.nd)
    d2.actuated = np.zeros(d.nd, dtype=np.int32)
    d2.gravcomp = np.zeros(d.nd, dtype=np.int32)
    d2.limited = np.zeros(d.nd, dtype=np.int32)
    od2 = oracle_mod.OracleDyn(d2)
    g = np.asarray(d.gravity, dtype=np.float64)

    def energy(q, v):
        _, M = od2.forward(q, v)
        P, R = dyn_ref.fk(m, q)
        pe = 0.0
        for b in dyn_ref.subtree_bodies(m, int(d.body[0])):
            pe -= m.body_mass[b] * float(g @ (P[b] + R[b] @ m.body_ipos[b]))
        return 0.5 * v @ M @ v + pe

    q, v, lag = q0.copy(), np.zeros(d.nd), np.zeros(d.nd)
    e0 = energy(q, v)
    q, v, lag = od2.step(q, v, lag, np.zeros(d.nd), n=n)
    e1 = energy(q, v)
    return e0, e1, 0.5 * v @ od2.forward(q, v)[1] @ v


def test_energy_bookkeeping_on_the_slot_reusing_tree(oracle_mod):
    """No damping, no actuation, no gravity compensation, no joint stops: over 200 sub-steps (0.4 s) from rest the semi-implicit Euler
    step keeps the total energy to O(h) -- a wrong Coriolis or gravity term, or a child hung on the wrong parent's pose, drifts by the
    released energy itself.  Two statements:
      * the bound of test_oracle_dyn.py's Push run, in its own terms: |e1 - e0| < 2 % of the kinetic energy the fall released.  The Push
        arm, run here again, drifts by 0.0805 J with 63.8 J released (0.13 %), this tree by 0.0441 J with 9.41 J released (0.47 %: a
        quarter of the arm's length, so it swings faster per step).  Scaling the arm's drift by the ratio of the two INITIAL energies is
        not a usable bound: a potential energy has an arbitrary zero -- measured from the world's origin the arm starts at 285.5 J and
        this tree at -4.09 J, which would ask for 0.0012 J of a tree that sits 5 cm from the origin and for any figure one likes after
        moving the origin;
      * the drift is first order in h: with half the step over the same 0.4 s it halves (to within 30 %: the next order)."""
    from mopa_rl_amd.dynamics import dyn_facts
    from mopa_rl_amd.kinematic_env import env_facts
    from mopa_rl_amd.scene import ENV_SPECS, load_scene
    env = "SawyerPushObstacle-v0"
    pm = load_scene(ENV_SPECS[env].scene)
    pf = env_facts(env, pm)
    pq = np.array(pm.qpos0, dtype=np.float64)
    pq[pf.arm_qpos_idx] = ENV_SPECS[env].init_qpos
    p0, p1, pke = _energy_run(oracle_mod, pm, dyn_facts(pm, pf), pq)
    assert pke > 1.0 and abs(p1 - p0) < 0.02 * pke          # (the existing test's statement)
    c = RD.case("slot_reuse")
    e0, e1, ke = _energy_run(oracle_mod, c.model, c.dyn, RD.base_row(c))
    h0, h1, hke = _energy_run(oracle_mod, c.model, c.dyn, RD.base_row(c), n=400, timestep=0.5 * c.dyn.timestep)
    print(f"push: e0 {p0:.6g} drift {abs(p1 - p0):.3g} ke {pke:.4g}; slot_reuse: e0 {e0:.6g} drift {abs(e1 - e0):.3g} ke {ke:.4g}; "
          f"at h / 2: drift {abs(h1 - h0):.3g} ke {hke:.4g}")
    assert ke > 1.0                                         # it did fall
    assert abs(e1 - e0) < 0.02 * ke
    assert h0 == e0 and 0.35 < abs(h1 - h0) / abs(e1 - e0) < 0.65


# ---------------- limits and refusals of the host compiler ----------------
def _refused(case, df, code, text):
    rc, msg, _, _ = RD.tables(case, df)
    assert rc == code and text in msg, (rc, msg)


def test_a_tree_with_four_save_slots_is_refused():
    c = RD.case("four_saves")
    assert c.n_save == 4 and (253 + 19 * 4) * 64 * 8 > 160 * 1024 >= (253 + 19 * 3) * 64 * 8
    _refused(c, c.dyn, ERR_LIMIT, "dynamic tree too branchy for the LDS layout")


@pytest.mark.parametrize("nd", [0, 10])
def test_dof_counts_outside_1_to_9_are_refused(nd):
    c = RD.case("chain9")
    _refused(c, dataclasses.replace(c.dyn, nd=nd), ERR_LIMIT, "the dynamics kernel keeps 1 .. 9 dofs per env")


def test_a_parent_at_or_after_its_child_is_refused():
    c = RD.case("slot_reuse")
    for i, p in ((2, 2), (3, 5), (1, -2)):
        parent = c.dyn.parent.copy()
        parent[i] = p
        _refused(c, dataclasses.replace(c.dyn, parent=parent), ERR_INVALID_ARG, "dynamic bodies must list parents before children")


def test_a_massless_dof_is_refused():
    c = RD.case("star")
    mass = c.dyn.mass.copy()
    mass[3] = 0.0
    _refused(c, dataclasses.replace(c.dyn, mass=mass), ERR_INVALID_ARG, "every dynamic body needs mass")


def test_an_arm_address_that_is_no_dof_is_refused():
    """an arm dof's record points at the address of an unactuated dof (and says so): the env's arm joint has no dof left"""
    c = RD.case("chain9")
    d = c.dyn
    arm_dof = [int(np.where(d.qadr == a)[0][0]) for a in c.facts.arm_qpos_idx]
    free = [i for i in range(d.nd) if i not in arm_dof]
    assert free
    qadr, actuated = d.qadr.copy(), d.actuated.copy()
    qadr[arm_dof[1]], actuated[arm_dof[1]] = qadr[free[0]], 0
    _refused(c, dataclasses.replace(d, qadr=qadr, actuated=actuated), ERR_INVALID_ARG, "an arm joint is not among the dynamic dofs")
