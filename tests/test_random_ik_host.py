"""IK off the Sawyer, on the CPU: what the host compiler of the IK tables (mopa_ik_tables_host) refuses, and the oracle's solver
(oracle/mopa_oracle.c orc_ik_solve, the checker of k_ik_solve) against an independent restatement on the chains of tests/random_ik.py --
its first update against a finite-difference normal-equation solve over tests/dyn_ref.fk, the error it reports for a successful solve
against a recomputation by the same forward kinematics."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_ref  # noqa: E402
import random_ik as RI  # noqa: E402
import random_scenes as RS  # noqa: E402

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_LIMIT = 1, 2, 4
WORST_FIRST_UPDATE = 1.95e-9      # measured: test_first_update_is_the_damped_normal_equation_solve


def _tables(model, ids):
    """(return code, error text, nb) of mopa_ik_tables_host for the site "tip" of `model` with the movable joint ids `ids`"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.ik import ik_desc
    L = _lib.lib()
    desc, keep = ik_desc(model, "tip", [])
    arr = np.ascontiguousarray(ids, dtype=np.int32)
    desc.n_joints, desc.joint_ids = len(arr), arr.ctypes.data_as(C.POINTER(C.c_int32))
    fp, nb = C.c_uint64(0), C.c_int32(-1)
    rc = L.mopa_ik_tables_host(C.byref(desc), C.byref(fp), C.byref(nb))
    return rc, L.mopa_last_error().decode() if rc else "", nb.value


@pytest.mark.parametrize("name", list(RI.CHAINS))
def test_every_chain_compiles(name):
    c = RI.chain(name)
    rc, text, nb = _tables(c.model, RI.joint_ids(c))
    assert rc == 0 and nb == len(RI.site_chain(c)), (rc, text, nb)


def test_chains_are_what_they_are_for():
    m = RI.chain("eight").model
    assert len(RI.joint_ids(RI.chain("eight"))) == 8 and sorted(int(m.jnt_type[j]) for j in RI.joint_ids(RI.chain("eight"))).count(RS.JNT_SLIDE) == 2
    c = RI.chain("nine_of_which_eight")
    on = [b for b in RI.site_chain(c) if c.model.body_jntnum[b]]
    assert len(RI.site_chain(c)) == 11 and len(on) == 9 and len(RI.joint_ids(c)) == 8 and c.model.body_jntnum[RI.site_chain(c)[0]] == 0
    c = RI.chain("prefix")
    assert [int(c.model.body_jntnum[b]) for b in RI.site_chain(c)] == [0, 0, 1, 1, 1, 1]
    c = RI.chain("off_chain")
    on = {int(c.model.body_jntadr[b]) for b in RI.site_chain(c)}
    assert len(on) == 4 and len(set(RI.joint_ids(c)) - on) == 2
    c = RI.chain("none_on_chain")
    ch = RI.site_chain(c)
    assert len(ch) == 2 and c.model.jnt_type[c.model.body_jntadr[ch[0]]] == RS.JNT_FREE and c.model.body_jntnum[ch[1]] == 0


# ---------------- limits and refusals ----------------
def _refused(model, ids, code, text):
    rc, msg, _ = _tables(model, ids)
    assert rc == code and text in msg, (rc, msg)


def test_joint_counts_outside_1_to_8_are_refused():
    c = RI.chain("nine_of_which_eight")
    m = c.model
    nine = [int(m.body_jntadr[b]) for b in RI.site_chain(c) if m.body_jntnum[b]]
    assert len(nine) == 9
    _refused(m, nine, ERR_LIMIT, "IK supports 1..8 movable joints")
    _refused(m, [], ERR_LIMIT, "IK supports 1..8 movable joints")


def test_a_free_joint_among_the_movable_ones_is_refused():
    c = RI.chain("none_on_chain")
    m = c.model
    free = int(np.nonzero(np.asarray(m.jnt_type) == RS.JNT_FREE)[0][0])
    _refused(m, list(RI.joint_ids(c)) + [free], ERR_UNSUPPORTED, "IK joints must be hinge or slide")


def test_a_two_joint_body_on_the_chain_is_refused():
    nodes = [RS.node(-1), RS.node(0, (RS.JNT_HINGE, RS.JNT_HINGE)), RS.node(1)]
    m, _ = RS.build("two_joint_body", 307, nodes, n_static=2, n_free=0)
    ms = RI.with_site(m, len(m.body_parent) - 1)
    _refused(ms, [0, 1, 3], ERR_UNSUPPORTED, "IK: bodies on the site's chain may carry at most one joint")


def test_a_joint_id_of_njnt_is_refused():
    c = RI.chain("prefix")
    ids = list(RI.joint_ids(c))
    _refused(c.model, ids[:-1] + [len(c.model.jnt_type)], ERR_INVALID_ARG, "joint id out of range")
    _refused(c.model, [-1] + ids[1:], ERR_INVALID_ARG, "joint id out of range")


def test_a_joint_id_listed_twice_is_refused():
    """(it used to be accepted: the joint's first column stayed zero, and the solve was not the checker's, which gives both columns the joint)"""
    c = RI.chain("prefix")
    ids = list(RI.joint_ids(c))
    _refused(c.model, ids + [ids[1]], ERR_INVALID_ARG, "is listed twice")
    _refused(c.model, [ids[0], ids[0]], ERR_INVALID_ARG, "is listed twice")
    from mopa_rl_amd import _lib
    from mopa_rl_amd.ik import ik_desc
    desc, keep = ik_desc(c.model, "tip", c.joints + [c.joints[2]])
    h = C.c_void_p(1)
    assert _lib.lib().mopa_ik_create(C.byref(desc), C.byref(h)) == ERR_INVALID_ARG and not h.value      # before any device is looked for


# ---------------- the oracle's solver against an independent restatement ----------------
def _problems(oracle_mod, c, E):
    m = c.model
    orc = oracle_mod.OracleScene(m, c.pi.passive_joint_idx, c.pi.ignored_contacts, RS.CONTACT_THRESHOLD)
    q = RI.rows(c, E, seed=41)
    qt = RI.perturbed(c, q, seed=41)
    tgt = RI.far_targets(np.array([RI.site_pose_ref(c, row)[0] for row in qt]), seed=41)
    return orc, q, tgt


def _first_update_errors(oracle_mod, name):
    c = RI.chain(name)
    m = c.model
    ids = RI.joint_ids(c)
    adr = [int(m.jnt_qposadr[j]) for j in ids]
    b = int(m.site_body[0])
    orc, q, tgt = _problems(oracle_mod, c, RI.E_HOST)
    worst, moved = 0.0, 0
    for e in range(RI.E_HOST):
        oq, _, steps, ok = orc.ik_solve(q[e], tgt[e], ids, b, m.site_pos[0], max_steps=1, tol=1e-14)
        assert steps == 0
        site = lambda row: RI.site_pose_ref(c, row)[0]
        if ok:                  # (none_on_chain: an unmoved target is met exactly)
            assert np.linalg.norm(tgt[e] - site(q[e])) < 1e-14 and np.array_equal(oq, q[e])
            continue
        h = 1e-6
        J = np.zeros((3, len(ids)))
        for k, a in enumerate(adr):
            qp, qm = q[e].copy(), q[e].copy()
            qp[a] += h
            qm[a] -= h
            J[:, k] = (site(qp) - site(qm)) / (2 * h)
        err = tgt[e] - site(q[e])
        dq = np.linalg.solve(J.T @ J + 0.03 * np.eye(len(ids)), J.T @ err)
        un = np.linalg.norm(dq)
        if un == 0.0 or np.linalg.norm(err) / un > 20.0:          # the stall rule: no update
            dq = np.zeros(len(ids))
        elif un > 2.0:                                          # the cap
            dq = dq * (2.0 / un)
        got = oq[adr] - q[e, adr]
        worst = max(worst, float(np.abs(got - dq).max()))
        moved += int(np.abs(got).max() > 0)
        rest = np.ones(m.nq, dtype=bool)
        rest[adr] = False
        assert np.array_equal(oq[rest], q[e, rest])
    return worst, moved


@pytest.mark.parametrize("name", list(RI.CHAINS))
def test_first_update_is_the_damped_normal_equation_solve(oracle_mod, name):
    """max_steps=1: the update the oracle applies is (J^T J + 0.03 I)^-1 J^T e with the stall rule (|e| / |dq| > 20: none) and the cap
    (|dq| <= 2), J by central differences (h = 1e-6) of the site position of tests/dyn_ref.fk.  Worst absolute difference over the six
    chains, 40 problems each: 1.95e-9 (prefix; eight 7.8e-10, nine_of_which_eight 9.3e-10, off_chain 9.4e-10, one 1.5e-11); the bound is ten
    times that.  (A finite-difference J carries about eps |p| / h = 1e-10
    of round-off per entry.)"""
    worst, moved = _first_update_errors(oracle_mod, name)
    print(f"{name}: first update differs by {worst:.3g}")
    assert worst < 10 * WORST_FIRST_UPDATE, worst
    assert moved > 0 or name == "none_on_chain"
    assert moved == 0 or name != "none_on_chain"




@pytest.mark.parametrize("name", list(RI.CHAINS))
@pytest.mark.parametrize("tol", [1e-2, 1e-6])
def test_err_norm_of_a_successful_solve_is_the_distance_to_the_target(oracle_mod, name, tol):
    """successes only: a solve that runs out of steps reports the error before its last update"""
    c = RI.chain(name)
    m = c.model
    orc, q, tgt = _problems(oracle_mod, c, RI.E_HOST)
    n_ok = 0
    for e in range(RI.E_HOST):
        oq, en, steps, ok = orc.ik_solve(q[e], tgt[e], RI.joint_ids(c), int(m.site_body[0]), m.site_pos[0], max_steps=100, tol=tol)
        if ok:
            n_ok += 1
            assert en < tol and abs(en - np.linalg.norm(tgt[e] - RI.site_pose_ref(c, oq)[0])) < 1e-12
    assert n_ok > 0 or name == "none_on_chain"
