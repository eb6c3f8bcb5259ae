"""The servo-dynamics kernels off the Sawyer (k_env_dyn, k_env_dyn4, the 16-lane mapping of the contact kernel) on the random and
directed body trees of tests/random_dyn.py -- slides with children, branches at several depths, 0 to 3 pose save slots and slots
with two writers, gravity with x and y components, an arm that is not in dof order -- through the C ABI (mopa_env_create ->
mopa_env_attach_dynamics -> forward / sub-steps / env.step), 200 envs (three full workgroups and a tail of 8), against
oracle/mopa_oracle_dyn.inc bit for bit."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_dyn as RD  # noqa: E402

pytestmark = pytest.mark.gpu

E = 200
FORMS = ["default", "wave"]      # the launch as it comes (the workgroup form, unless the tree shares a save slot), the single-wave form pinned


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def _form(monkeypatch, form):
    """the default launch, or the single-wave form pinned"""
    if form == "wave":
        monkeypatch.setenv("MOPA_DYN_KERNEL", "wave")
    else:
        monkeypatch.delenv("MOPA_DYN_KERNEL", raising=False)


class _Env:
    """an env with dynamics through the C ABI, its state in torch tensors"""

    def __init__(self, torch, case, df=None, lanes16=False, attach=True, **env):
        from mopa_rl_amd import _lib
        self.torch, self.L, self.case = torch, _lib.lib(), case
        self.nd, self.nq, self.n_arm = case.dyn.nd, case.model.nq, len(case.facts.arm_qpos_idx)
        edesc, ddesc, self.keep = RD.descs(case, df, device=torch.cuda.current_device(), **env)
        self.h = C.c_void_p()
        _lib.check(self.L.mopa_env_create(C.byref(edesc), C.byref(self.h)))
        self.ddesc = ddesc
        if attach:
            _lib.check(self.L.mopa_env_attach_dynamics(self.h, C.byref(ddesc)))
            assert self.L.mopa_env_dyn_dofs(self.h) == self.nd
        if lanes16:         # the empty contact stage BatchKinematicEnv attaches for dyn_lanes=16: no shapes, no pairs, no object
            cd = _lib.MopaCtDesc()
            cd.ns = cd.nf = cd.np = 0
            cd.obj_qadr = -1
            cd.maxcon, cd.maxpair, cd.iterations = 0, 1, 1
            cd.tolerance, cd.inv_scale = 0.0, 1.0
            cd.precull_every, cd.precull_margin, cd.warmstart = 15, 0.0, 0
            cd.near_every, cd.near_margin = 3, 0.0
            cd.noslip_iterations, cd.noslip_tolerance = 0, 0.0
            cd.solver, cd.limit_rows = 0, 0
            _lib.check(self.L.mopa_env_attach_contacts(self.h, C.byref(cd)))
            assert self.L.mopa_env_dyn_qvel_width(self.h) == self.nd
        dev, f64 = torch.device("cuda"), torch.float64
        self.obs_dim = self.L.mopa_env_obs_dim(self.h)
        self.qpos, self.qvel = torch.zeros(E, self.nq, dtype=f64, device=dev), torch.zeros(E, self.nd, dtype=f64, device=dev)
        self.bias_lag, self.prev_state = torch.zeros(E, self.nd, dtype=f64, device=dev), torch.zeros(E, self.n_arm, dtype=f64, device=dev)
        self.has_prev, self.ep_len = torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
        self.obs, self.reward = torch.zeros(E, self.obs_dim, dtype=f64, device=dev), torch.zeros(E, dtype=f64, device=dev)
        self.done, self.success = torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev)

    def close(self):
        if self.h.value:
            self.L.mopa_env_destroy(self.h)
            self.h = C.c_void_p()

    def load(self, q, v, lag=None):
        t = self.torch
        self.qpos.copy_(t.tensor(q, device="cuda"))
        self.qvel.copy_(t.tensor(v, device="cuda"))
        if lag is not None:
            self.bias_lag.copy_(t.tensor(lag, device="cuda"))

    def forward(self):
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import _ptr
        t = self.torch
        bias = t.zeros(E, self.nd, dtype=t.float64, device="cuda")
        M = t.zeros(E, self.nd * (self.nd + 1) // 2, dtype=t.float64, device="cuda")
        _lib.check(self.L.mopa_env_dyn_forward_batch(self.h, E, _ptr(self.qpos), _ptr(self.qvel), _ptr(bias), _ptr(M), None, None))
        t.cuda.synchronize()
        return bias.cpu().numpy(), M.cpu().numpy()

    def substeps(self, ctrl, n):
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import _ptr
        c = self.torch.tensor(ctrl, device="cuda")
        _lib.check(self.L.mopa_env_dyn_substeps_batch(self.h, E, _ptr(self.qpos), _ptr(self.qvel), _ptr(self.bias_lag), _ptr(c), int(n), None))
        self.torch.cuda.synchronize()

    def step(self, action, is_planner, move_mask=None, kinematic=False):
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import _ptr
        t = self.torch
        a = t.tensor(action, device="cuda") if action is not None else None
        mm = t.tensor(move_mask, device="cuda") if move_mask is not None else None
        ap, mp = (_ptr(a) if a is not None else None), (_ptr(mm) if mm is not None else None)
        if kinematic:
            _lib.check(self.L.mopa_env_step_batch(self.h, E, _ptr(self.qpos), _ptr(self.prev_state), _ptr(self.has_prev), _ptr(self.ep_len), ap,
                                                  int(is_planner), mp, _ptr(self.obs), _ptr(self.reward), _ptr(self.done), _ptr(self.success), None))
        else:
            _lib.check(self.L.mopa_env_step_dyn_batch(self.h, E, _ptr(self.qpos), _ptr(self.qvel), _ptr(self.bias_lag), _ptr(self.prev_state),
                                                      _ptr(self.has_prev), _ptr(self.ep_len), ap, int(is_planner), mp, _ptr(self.obs),
                                                      _ptr(self.reward), _ptr(self.done), _ptr(self.success), None))
        t.cuda.synchronize()

    def host(self, *names):
        return [getattr(self, n).cpu().numpy() for n in names]


@pytest.fixture
def envs():
    made = []
    yield made
    for e in made:
        e.close()


def _oracle_forward(oracle_mod, df, q, v):
    od = oracle_mod.OracleDyn(df)
    il = np.tril_indices(df.nd)
    out = [od.forward(q[e], v[e]) for e in range(len(q))]
    return np.array([b for b, _ in out]), np.array([M[il] for _, M in out])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", RD.ALL_CASES)
def test_forward_bias_and_inertia_bit_exact(oracle_mod, torch_mod, envs, monkeypatch, key, form):
    _form(monkeypatch, form)
    c = RD.case(key)
    env = _Env(torch_mod, c)
    envs.append(env)
    q, v = RD.states(c, E, seed=1)
    env.load(q, v)
    bias, M = env.forward()
    ob, oM = _oracle_forward(oracle_mod, c.dyn, q, v)
    bad = np.nonzero((_bits(bias) != _bits(ob)).any(axis=1) | (_bits(M) != _bits(oM)).any(axis=1))[0]
    assert len(bad) == 0, f"{key} / {form}: {len(bad)} of {E} envs differ from the oracle (first: env {bad[0]}; parent {list(c.dyn.parent)})"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("key", RD.ALL_CASES)
def test_substeps_bit_exact(oracle_mod, torch_mod, envs, monkeypatch, key, n, form):
    _form(monkeypatch, form)
    c = RD.case(key)
    d = c.dyn
    od = oracle_mod.OracleDyn(d)
    env = _Env(torch_mod, c)
    envs.append(env)
    q, v = RD.states(c, E, seed=10 + n)
    rng = np.random.default_rng(n)
    ctrl = q[:, d.qadr] + rng.uniform(-0.3, 0.3, size=(E, d.nd)) * np.where(d.jtype == RD.JNT_HINGE, 1.0, 0.05)
    lag0 = np.array([od.forward(q[e], v[e], want_M=False)[0] for e in range(E)])
    env.load(q, v, lag0)
    env.substeps(ctrl, n)
    gq, gv, gl = env.host("qpos", "qvel", "bias_lag")
    want = [od.step(q[e], v[e], lag0[e], ctrl[e], n) for e in range(E)]
    oq, ov, ol = (np.array([w[k] for w in want]) for k in range(3))
    for name, g, o in (("qpos", gq, oq), ("qvel", gv, ov), ("bias_lag", gl, ol)):
        bad = np.nonzero((_bits(g) != _bits(o)).any(axis=1))[0]
        assert len(bad) == 0, f"{key} / {form}, {n} sub-steps: {name} of {len(bad)} envs differs (first: env {bad[0]})"
    assert np.isfinite(oq).all() and np.isfinite(ov).all()
    lim = d.limited == 1
    if lim.any():           # the joint stops were exercised
        assert (((oq[:, d.qadr] == d.lo) | (oq[:, d.qadr] == d.hi)) & lim).any()


def test_trees_with_a_shared_save_slot_take_the_single_wave_form(torch_mod, envs, monkeypatch):
    """in the workgroup form four waves walk the chain on the same LDS columns with no barrier inside the pass: a slot with two writers is
    safe in one wave's walk only, so such a tree is launched in the single-wave form (the forward / sub-step / rollout tests above ran
    the workgroup form on these trees before that rule and found it bit-equal on this GPU: a margin in time, not a guarantee)"""
    shared = 0
    for key in RD.ALL_CASES:
        c = RD.case(key)
        env = _Env(torch_mod, c)
        envs.append(env)
        _form(monkeypatch, "default")
        assert env.L.mopa_env_dyn_waves(env.h) == (1 if RD.reuses_a_slot(c.dyn.parent) else 4), key
        _form(monkeypatch, "wave")
        assert env.L.mopa_env_dyn_waves(env.h) == 1, key
        shared += int(RD.reuses_a_slot(c.dyn.parent))
    assert 6 <= shared < len(RD.ALL_CASES)
    env = _Env(torch_mod, RD.case("star"), attach=False)
    envs.append(env)
    assert env.L.mopa_env_dyn_waves(env.h) == -1
    from mopa_rl_amd.kinematic_env import make_env
    _form(monkeypatch, "default")
    for name in ("SawyerPushObstacle-v0", "SawyerLiftObstacle-v0", "SawyerAssemblyObstacle-v0"):      # one slot, one writer
        sawyer = make_env(name, 8, dynamics=True)
        assert env.L.mopa_env_dyn_waves(sawyer._h) == 4, name
        sawyer.close()


STATE = ("qpos", "qvel", "bias_lag", "obs", "prev_state", "reward")
FLAGS = ("done", "success", "has_prev", "ep_len")


def _rollout(c, rng):
    """the calls of a rollout: two policy steps around a planner step and a planner step under a move mask (every value of it)"""
    n_arm = len(c.facts.arm_qpos_idx)
    mm = rng.integers(0, 4, size=E).astype(np.uint8)
    assert np.bincount(mm, minlength=4).min() >= 2
    return [(rng.uniform(-1.5, 1.5, (E, n_arm)), False, None), (rng.uniform(-0.08, 0.08, (E, n_arm)), True, None),
            (rng.uniform(-0.08, 0.08, (E, n_arm)), True, mm), (rng.uniform(-1.5, 1.5, (E, n_arm)), False, None)]


@pytest.mark.parametrize("key", RD.ROLLOUT_CASES)
def test_env_step_rollout_bit_identical_to_oracle(oracle_mod, torch_mod, envs, monkeypatch, key):
    _form(monkeypatch, "default")
    c = RD.case(key)
    cfg = dict(RD.ENV, max_episode_steps=3)
    ref = oracle_mod.OracleEnv(RD.oracle_scene(oracle_mod, c), c.facts, E, dyn=c.dyn, **cfg)
    env = _Env(torch_mod, c, max_episode_steps=3)
    envs.append(env)
    assert env.obs_dim == ref.obs_dim and env.L.mopa_env_action_dim(env.h) == ref.action_dim == env.n_arm
    q, _ = RD.states(c, E, seed=5, spread=0.5)
    ref.set_state(q)
    env.load(q, ref.qvel, ref.bias_lag)           # (at rest, the oracle's lagged bias: the forward launch has its own test)
    n_done = 0
    for t, (a, is_planner, mm) in enumerate(_rollout(c, np.random.default_rng(7))):
        env.step(a, is_planner, mm)
        ref.step(a, is_planner=is_planner, move_mask=mm, nthreads=8)
        for name in STATE:
            assert np.array_equal(_bits(env.host(name)[0]), _bits(getattr(ref, name))), f"{key}, step {t}: {name}"
        for name in FLAGS:
            assert np.array_equal(env.host(name)[0], getattr(ref, name)), f"{key}, step {t}: {name}"
        n_done += int(ref.done.sum())
    assert n_done > E // 2 and np.abs(ref.qvel).max() > 1e-3 and np.isfinite(ref.qpos).all()


@pytest.mark.parametrize("key", RD.ROLLOUT_CASES)
def test_16_lane_mapping_equals_the_lane_per_env_form(torch_mod, envs, monkeypatch, key):
    """the contact-free servo dynamics through the contact kernel's mapping (16 lanes per env, an empty contact stage), as
    test_gpu_dyn.test_contact_free_dynamics_in_the_16_lane_mapping_equals_k6 has it on the Sawyer"""
    _form(monkeypatch, "default")
    c = RD.case(key)
    a, b = _Env(torch_mod, c, max_episode_steps=3), _Env(torch_mod, c, lanes16=True, max_episode_steps=3)
    envs.extend([a, b])
    q, _ = RD.states(c, E, seed=6, spread=0.5)
    for env in (a, b):
        env.load(q, np.zeros((E, c.dyn.nd)))
    lag, _ = a.forward()
    for env in (a, b):
        env.load(q, np.zeros((E, c.dyn.nd)), lag)
    for t, (act, is_planner, mm) in enumerate(_rollout(c, np.random.default_rng(8))[:3]):
        for env in (a, b):
            env.step(act, is_planner, mm)
        for name in STATE + FLAGS:
            x, y = a.host(name)[0], b.host(name)[0]
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{key}, step {t}: {name}"
    assert np.abs(a.host("qvel")[0]).max() > 1e-3


def test_the_comparison_can_fail(oracle_mod, torch_mod, envs, monkeypatch):
    """the GPU gets three_saves with the mass of its deepest leaf times (1 + 1e-12), the oracle the unchanged facts: the diagonal of M
    differs in the rows of the leaf and of its ancestors, every entry of every other row is bit-equal, the bias differs at the leaf's dof.
    (A leaf's mass enters an ancestor's diagonal entry through m |a x r|^2, which an env may have near zero: "differs" is asked of most
    envs, "equal" of all.)"""
    _form(monkeypatch, "default")
    c = RD.case("three_saves")
    d = c.dyn
    depth = [0] * d.nd
    for i in range(1, d.nd):
        depth[i] = depth[d.parent[i]] + 1
    leaf = int(np.argmax(depth))
    assert leaf == 3 and not (d.parent == leaf).any()
    line = [leaf]
    while d.parent[line[-1]] >= 0:
        line.append(int(d.parent[line[-1]]))
    mass = d.mass.copy()
    mass[leaf] *= 1.0 + 1e-12
    assert mass[leaf] != d.mass[leaf]
    env = _Env(torch_mod, c, df=dataclasses.replace(d, mass=mass))
    envs.append(env)
    q, v = RD.states(c, E, seed=1)
    env.load(q, v)
    bias, M = env.forward()
    ob, oM = _oracle_forward(oracle_mod, d, q, v)
    rows, cols = np.tril_indices(d.nd)
    for i in range(d.nd):
        k = np.nonzero(rows == i)[0]
        if i in line:
            diag = int(np.nonzero((rows == i) & (cols == i))[0][0])
            assert (_bits(M[:, diag]) != _bits(oM[:, diag])).sum() > E // 2, i
        else:
            assert np.array_equal(_bits(M[:, k]), _bits(oM[:, k])), i
    assert (_bits(bias[:, leaf]) != _bits(ob[:, leaf])).sum() > E // 2
    assert np.abs(M - oM).max() < 1e-9 and np.abs(bias - ob).max() < 1e-9


def test_a_refused_tree_leaves_the_env_kinematic(oracle_mod, torch_mod, envs):
    """attach_dynamics commits last: after the refusal of four_saves the env is what it was, and steps kinematically as the oracle does"""
    c = RD.case("four_saves")
    env = _Env(torch_mod, c, attach=False, max_episode_steps=3)
    envs.append(env)
    rc = env.L.mopa_env_attach_dynamics(env.h, C.byref(env.ddesc))
    assert rc == 4 and "dynamic tree too branchy for the LDS layout" in env.L.mopa_last_error().decode()
    assert env.L.mopa_env_dyn_dofs(env.h) == -1
    ref = oracle_mod.OracleEnv(RD.oracle_scene(oracle_mod, c), c.facts, E, **dict(RD.ENV, max_episode_steps=3))
    q, _ = RD.states(c, E, seed=9, spread=0.5)
    env.load(q, np.zeros((E, c.dyn.nd)))
    env.step(None, False, kinematic=True)
    ref.set_state(q)
    rng = np.random.default_rng(3)
    for t, is_planner in enumerate([False, True, False]):
        a = rng.uniform(-0.12, 0.12, (E, env.n_arm)) if is_planner else rng.uniform(-1.5, 1.5, (E, env.n_arm))
        env.step(a, is_planner, kinematic=True)
        ref.step(a, is_planner=is_planner)
        for name in ("qpos", "obs", "reward"):
            assert np.array_equal(_bits(env.host(name)[0]), _bits(getattr(ref, name))), f"step {t}: {name}"
        assert np.array_equal(env.host("done")[0], ref.done) and np.array_equal(env.host("success")[0], ref.success)
    assert ref.done.all() and not np.array_equal(ref.qpos, q)
