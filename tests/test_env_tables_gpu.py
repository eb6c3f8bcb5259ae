"""The shared body-walk compiler (csrc/mopa_model_host.hpp) feeds the env and IK walks a tree they have never seen: a push env and an
IK site on random_scenes.deep_branches (branch points at three depths), 65 envs -- one full wave plus one lane of the next --
against the CPU oracle, bit for bit."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_scenes as RS  # noqa: E402
from test_env_tables_host import DEEP_ENV, deep_facts, deep_site, env_tables  # noqa: E402

pytestmark = pytest.mark.gpu

E = 65


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the nearest double)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _quat2mat(q):
    """csrc/mopa_device.hpp quat2mat, operation for operation"""
    w, x, y, z = (float(v) for v in q)
    q00, q01, q02, q03 = w * w, w * x, w * y, w * z
    q11, q12, q13 = x * x, x * y, x * z
    q22, q23, q33 = y * y, y * z, z * z
    return [((q00 + q11) - q22) - q33, 2.0 * (q12 - q03), 2.0 * (q13 + q02),
            2.0 * (q12 + q03), ((q00 - q11) + q22) - q33, 2.0 * (q23 - q01),
            2.0 * (q13 - q02), 2.0 * (q23 + q01), ((q00 - q11) - q22) + q33]


@pytest.fixture(scope="module")
def deep(oracle_mod):
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    m, pi = RS.scene("deep_branches")
    orc = oracle_mod.OracleScene(m, pi.passive_joint_idx, pi.ignored_contacts, RS.CONTACT_THRESHOLD)
    rng = np.random.default_rng(36)
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (E, 1))
    for j, t in enumerate(m.jnt_type):
        a = int(m.jnt_qposadr[j])
        if t == RS.JNT_FREE:
            q[:, a:a + 3] += rng.uniform(-0.2, 0.2, (E, 3))
            quat = rng.normal(size=(E, 4))
            q[:, a + 3:a + 7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        else:
            lo, hi = (m.jnt_range[j] if m.jnt_limited[j] else (-3.14, 3.14))
            q[:, a] = rng.uniform(lo, hi, E)
    return m, orc, q, rng


def test_push_env_on_deep_branches_is_the_oracle_bit_for_bit(deep, oracle_mod):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr, _stream_handle
    from mopa_rl_amd.kinematic_env import env_desc
    m, orc, q, rng = deep
    f = deep_facts(m)
    assert len(f.grip_qpos_idx) == 0 and 1 <= len(f.arm_qpos_idx) <= 7
    cfg = dict(DEEP_ENV, max_episode_steps=3)          # (the third step ends the episode)
    desc, keep = env_desc(m, f, device=torch.cuda.current_device(), **cfg)
    t = env_tables(desc)
    assert t["n_save"] >= 2, t
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.mopa_env_create(C.byref(desc), C.byref(h)))
    try:
        ref = oracle_mod.OracleEnv(orc, f, E, **cfg)
        n_arm, obs_dim = len(f.arm_qpos_idx), L.mopa_env_obs_dim(h)
        assert obs_dim == ref.obs_dim == f.obs_dim - 4 and L.mopa_env_action_dim(h) == ref.action_dim == n_arm      # (no gripper: 2 + 2 entries less)
        dev, f64 = torch.device("cuda"), torch.float64
        qpos = torch.tensor(q, device=dev)
        prev, has_prev = torch.zeros(E, n_arm, dtype=f64, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)
        ep_len, obs = torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros(E, obs_dim, dtype=f64, device=dev)
        reward = torch.zeros(E, dtype=f64, device=dev)
        done, success = torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)

        def launch(action, is_planner):
            _lib.check(L.mopa_env_step_batch(h, E, _ptr(qpos), _ptr(prev), _ptr(has_prev), _ptr(ep_len), _ptr(action) if action is not None else None,
                                             int(is_planner), None, _ptr(obs), _ptr(reward), _ptr(done), _ptr(success), _stream_handle(None)))
            torch.cuda.synchronize()

        def same(what):
            assert np.array_equal(_bits(qpos.cpu().numpy()), _bits(ref.qpos)), f"{what}: qpos"
            assert np.array_equal(_bits(obs.cpu().numpy()), _bits(ref.obs)), f"{what}: obs"

        launch(None, False)
        ref.set_state(q)
        same("set_state")
        for k, is_planner in enumerate([False, False, False, True]):
            a = rng.uniform(-0.12, 0.12, (E, n_arm)) if is_planner else rng.uniform(-1.5, 1.5, (E, n_arm))
            launch(torch.tensor(a, device=dev), is_planner)
            ref.step(a, is_planner=is_planner)
            same(f"step {k}")
            assert np.array_equal(_bits(reward.cpu().numpy()), _bits(ref.reward)), f"step {k}: reward"
            assert np.array_equal(done.cpu().numpy(), ref.done), f"step {k}: done"
            assert np.array_equal(success.cpu().numpy(), ref.success), f"step {k}: success"
        assert ref.done.any() and not np.array_equal(ref.qpos, q)
    finally:
        L.mopa_env_destroy(h)


def test_ik_on_deep_branches_is_the_oracle_bit_for_bit(deep):
    import torch
    from mopa_rl_amd.ik import BatchIK
    m, orc, q, rng = deep
    ms, joints = deep_site(m)
    assert 3 <= len(joints) <= 8
    ik = BatchIK(ms, "tip", joints, device=torch.cuda.current_device())
    chain = []
    b = ik.site_body
    while b > 0:
        chain.append(b)
        b = int(m.body_parent[b])
    assert all(m.body_jntnum[c] <= 1 for c in chain) and sum(int(m.body_jntnum[c]) for c in chain) == len(joints)
    pos, mat = ik.site_pose(torch.tensor(q, device="cuda"))
    pos, mat = pos.cpu().numpy(), mat.cpu().numpy().reshape(E, 9)
    sl = _quat2mat(ms.site_quat[0])
    off = [float(v) for v in ik.site_off]
    for e in range(E):
        xpos, xquat = orc.fk_bodies(q[e])
        M = _quat2mat(xquat[ik.site_body])
        want_pos = [float(xpos[ik.site_body][r]) + _fma(M[3 * r + 2], off[2], _fma(M[3 * r + 1], off[1], M[3 * r] * off[0])) for r in range(3)]
        want_mat = [_fma(M[3 * r + 2], sl[6 + c], _fma(M[3 * r + 1], sl[3 + c], M[3 * r] * sl[c])) for r in range(3) for c in range(3)]
        assert np.array_equal(_bits(pos[e]), _bits(want_pos)), e
        assert np.array_equal(_bits(mat[e]), _bits(want_mat)), e
    # one solve: targets = the site of a perturbed pose, every third one pushed far away (the chain's slide reaches it, not in 6 steps)
    rng = np.random.default_rng(37)
    adrs = [int(m.jnt_qposadr[j]) for j in ik.joint_ids]
    qt = q.copy()
    qt[:, adrs] += rng.normal(0, 0.3, (E, len(adrs)))
    tgt, _ = ik.site_pose(torch.tensor(qt, device="cuda"))
    tgt = tgt.cpu().numpy()
    tgt[::3] += rng.normal(0, 1.5, (len(tgt[::3]), 3))
    res = ik.solve(torch.tensor(q, device="cuda"), torch.tensor(tgt, device="cuda"), None, max_steps=6, tol=1e-2)
    gq, ge, gs, gok = res.qpos.cpu().numpy(), res.err_norm.cpu().numpy(), res.steps.cpu().numpy(), res.success.cpu().numpy()
    n_ok = 0
    for e in range(E):
        oq, oe, os_, ook = orc.ik_solve(q[e], tgt[e], ik.joint_ids, ik.site_body, ik.site_off, max_steps=6, tol=1e-2)
        assert np.array_equal(_bits(gq[e]), _bits(oq)), (e, np.abs(gq[e] - oq).max())
        assert _bits(ge[e]) == _bits(oe) and gs[e] == os_ and bool(gok[e]) == ook, e
        n_ok += ook
    assert 0 < n_ok < E            # both outcomes occur
