"""Contact-force readout on the GPU (`BatchKinematicEnv.enable_contact_force`, C ABI `mopa_env_set_contact_force`): what the reference's
`env.get_contact_force()` reads after every env.step, from the last constraint solve of a launch of K7 (`k_env_dyn_ct`) and K8
(`k_pusher_dyn`), through env.step, the raw sub-step entry points and `BatchMoPARollout.run_episode`.

  K8  bit for bit against tests/contact_force_ref.py (the sequential checker with its constraint forces kept);
  K7  the contacts against the oracle's detection, the forces against tests/dyn_ref.py's independent solve of the same sub-step
      (bounds: profiles/r13/contact_force_parity.txt), the weight of the resting cube, the sum against the rows bit for bit, the
      states bit-identical with the readout on and off.
PARITY WITH MuJoCo IS UNPINNED, as for the solves the readout reads.  Every test prints the figures it asserts on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PUSH, LIFT, PUSHER = "SawyerPushObstacle-v0", "SawyerLiftObstacle-v0", "PusherObstacle-v0"

# the two committed contact states of tests/test_pusher_dyn_host.py (dofs joint0..3, box_x, box_y): fingertip 2 mm into the box
# (2 contacts), box 2 mm into obstacle7 (4 contacts)
Q_TIP_IN_BOX = [0.0, 0.0, 0.0, math.pi / 2, 0.3, 0.11 + 0.02 - 0.002]
Q_BOX_IN_OBSTACLE = [0.0, 0.0, 0.0, 0.0, -0.12 + 0.02 - 0.002, -0.12]
PUSHER_VEL = 0.05          # the velocity of the two moving variants (every dof; + for the first state, - for the second)

# the four object velocities (v 3, w 3) of tests/test_oracle_contact.py::test_spinning_sliding_object_step_equals_the_independent_qp
OBJ_VELS = ([0.0, 0.0, 0.0, 0.0, 0.0, 6.0], [0.25, -0.1, 0.0, 0.4, -0.3, 3.0], [1.5, 0.0, 0.0, 0.0, 0.0, 40.0], [0.0, 0.0, -0.05, 2.0, 1.0, -15.0])

# Bounds of the K7 forces against the independent solve: max |f_gpu - f_ref| / max |f_ref| per state, 10 x the largest value measured on
# an MI355X (profiles/r13/contact_force_parity.txt has every measurement): elliptic cones 1.101e-9 (Lift, the tumbling can; Push
# 6.065e-10), pyramidal cones 7.100e-15 (Newton; projected Gauss-Seidel 3.384e-15).  Hard cap 1e-3.
FORCE_BOUND = {"elliptic": 10 * 1.101e-9, "newton-pyramidal": 10 * 7.100e-15, "pgs": 10 * 7.100e-15}
FORCE_CAP = 1e-3
# Weight of the resting cube: 10 x the deviation of the independent solve's own normal forces from m g at the oracle's settled state
# (measured on the CPU: 2.040e-12, same file; the kernel's own rows: 2.021e-12)
WEIGHT_BOUND = 10 * 2.040e-12


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the gpu-marked tests need a HIP device"
    return torch


def _t(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


# ---- K8 -------------------------------------------------------------------------------------------------------------------------
def _pusher_case(torch):
    """E = 4: the two committed contact states at rest, and the same two moving"""
    from contact_force_ref import PusherForceRef
    from mopa_rl_amd.kinematic_env import make_env
    env = make_env(PUSHER, 4, dynamics=True, contacts=True, seed=3)
    f = env.pdyn
    q6 = np.array([Q_TIP_IN_BOX, Q_BOX_IN_OBSTACLE, Q_TIP_IN_BOX, Q_BOX_IN_OBSTACLE])
    qpos = np.tile(np.asarray(env.model.qpos0, dtype=np.float64), (4, 1))
    qpos[:, f.qadr] = q6
    qvel = np.zeros((4, 6))
    qvel[2], qvel[3] = PUSHER_VEL, -PUSHER_VEL
    return env, PusherForceRef(f), q6, qpos, qvel


def _pusher_load(torch, env, qpos, qvel):
    env.set_state(_t(torch, qpos))
    env.qvel.copy_(_t(torch, qvel))
    env.i_term.zero_()


def _pusher_check(env, ref, q6, qvel, n, need_contacts):
    rows_g, cnt_g = env.contact_rows.cpu().numpy(), env.contact_count.cpu().numpy()
    force_g, total_g = env.contact_force.cpu().numpy(), env.contact_force_total.cpu().numpy()
    counts = []
    for e in range(4):
        rows, force = ref.readout(q6[e], qvel[e], [0.0] * 4, q6[e][:4], q6[e][:4], n)
        counts.append(len(rows))
        print(f"K8 n={n} env {e}: contacts {len(rows)} (gpu {int(cnt_g[e])}), force ref {force!r} gpu {float(force_g[e])!r}")
        if need_contacts:
            assert len(rows) >= 1, f"env {e}: the reference itself has no contact -- the comparison would be empty"
        assert int(cnt_g[e]) == len(rows), e
        assert np.array_equal(_bits(rows_g[e, :len(rows)]), _bits(rows)), (e, rows_g[e, :len(rows)] - rows)
        assert np.array_equal(_bits(force_g[e]), _bits(force)), (e, force_g[e], force)
        assert np.array_equal(_bits(total_g[e]), _bits(0.0 + force)), e          # one launch since set_state zeroed the total
    return counts


def test_pusher_raw_substeps_bit_exact(torch_mod):
    torch = torch_mod
    env, ref, q6, qpos, qvel = _pusher_case(torch)
    env.enable_contact_force(rows=True)
    assert tuple(env.contact_rows.shape) == (4, env.pdyn.maxcon, 8)
    _pusher_load(torch, env, qpos, qvel)
    arm = _t(torch, q6[:, :4])
    env.pusher_substeps(arm, arm.clone(), 3)
    torch.cuda.synchronize()
    counts = _pusher_check(env, ref, q6, qvel, 3, need_contacts=True)
    assert counts[0] == 2 and counts[1] == 4
    # n = 0 launches nothing: every value stays
    before = env.contact_force.clone()
    env.pusher_substeps(arm, arm.clone(), 0)
    torch.cuda.synchronize()
    assert torch.equal(before, env.contact_force)
    env.close()


def test_pusher_env_step_bit_exact(torch_mod):
    """one env.step (zero action: desired = the arm's pose) = nsub sub-steps of the checker; the envs that sit the launch out or only
    record the command (move-mask bits) keep their previous values"""
    torch = torch_mod
    env, ref, q6, qpos, qvel = _pusher_case(torch)
    env.enable_contact_force(rows=True)
    _pusher_load(torch, env, qpos, qvel)
    env.step(torch.zeros(4, 4, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    _pusher_check(env, ref, q6, qvel, env.pdyn.nsub, need_contacts=False)
    # a second launch in which env 1 sits out (bit 1) and env 2 has its move flag clear: their values stay, the others' totals grow
    f0, t0, c0, r0 = (x.clone() for x in (env.contact_force, env.contact_force_total, env.contact_count, env.contact_rows))
    mm = torch.tensor([1, 2, 0, 1], dtype=torch.uint8, device="cuda")
    env._launch(torch.zeros(4, 4, dtype=torch.float64, device="cuda"), False, mm)
    torch.cuda.synchronize()
    for e in (1, 2):
        assert torch.equal(f0[e], env.contact_force[e]) and torch.equal(t0[e], env.contact_force_total[e])
        assert torch.equal(c0[e], env.contact_count[e]) and torch.equal(r0[e], env.contact_rows[e])
    for e in (0, 3):
        assert float(env.contact_force_total[e]) == float(t0[e]) + float(env.contact_force[e])
    # reset(mask) zeroes the three scalars of the reset envs only
    mk = torch.tensor([True, False, False, False], device="cuda")
    keep = env.contact_force_total.clone()
    env.reset(mask=mk)
    assert float(env.contact_force_total[0]) == 0.0 and float(env.contact_force[0]) == 0.0 and int(env.contact_count[0]) == 0
    assert torch.equal(keep[1:], env.contact_force_total[1:])
    env.disable_contact_force()
    assert env.contact_force is None
    env.step(torch.zeros(4, 4, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    env.close()


# ---- K7 -------------------------------------------------------------------------------------------------------------------------
_K7 = {}


def _k7_opts(form):
    base = dict(iterations=50, tolerance=0.0, warmstart=False, noslip_iterations=0, limit_rows=False)
    if form == "newton-pyramidal":
        base.update(solver="newton", cone="pyramidal")
    elif form == "pgs":
        base.update(solver="pgs", cone="pyramidal", iterations=3000)
    return base


def _k7_case(torch, env_name, form):
    """E = 8, prepared as tests/test_oracle_contact.py::test_spinning_sliding_object_step_equals_the_independent_qp: the object settled for
    150 oracle sub-steps, then the four object velocities of that test, two envs each; ONE raw sub-step with the readout on and
    the same launch with it off.  The oracle's contacts and the independent solve's forces are computed once per case."""
    key = (env_name, form)
    if key in _K7:
        return _K7[key]
    import dyn_ref
    from contact_force_ref import decode_pyramid
    from mopa_rl_amd.kinematic_env import make_env
    from oracle import oracle as O
    E = 8
    env = make_env(env_name, E, dynamics=True, contacts=True, contact_options=_k7_opts(form), seed=3)
    m, d, ct = env.model, env.dyn, env.ct
    od = O.OracleDyn(d, ct=ct)
    nd = d.nd
    q = np.asarray(env.init_qpos_row, dtype=np.float64).copy()
    v = np.zeros(od.nv)
    lag = od.forward(q, v[:nd], want_M=False)[0]
    ctrl = q[d.qadr].copy()
    q, v, lag = od.step(q, v, lag, ctrl, n=150)
    con = od.contacts(q)
    pair_of = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(ct.pr_f, ct.pr_s))}
    con_pairs = [pair_of[(int(r[7]), int(r[8]))] for r in con]
    ident = [(p, int(r[9])) for p, r in zip(con_pairs, con)]
    qvel = np.tile(v, (E, 1))
    for e in range(E):
        qvel[e, nd:] = OBJ_VELS[e // 2]
    # the independent solve, per velocity case: {(pair, feature): force entries in the contact frame}
    ref_f = []
    for vel in OBJ_VELS:
        v2 = v.copy()
        v2[nd:] = vel
        _, fr = dyn_ref.contact_step_reference(m, d, ct, con, q, v2, lag, ctrl, cone="elliptic" if form == "elliptic" else "pyramidal")
        fr = np.asarray(fr).reshape(-1, 4)
        assert len(fr) == len(con)
        if form != "elliptic":          # per pyramid edge (t1 +, t1 -, t2 +, t2 -): decoded by the same formula as the kernel's rows
            fr = np.array([decode_pyramid([float(x) for x in p4], float(ct.pr_par[p][0])) for p4, p in zip(fr, con_pairs)])
        ref_f.append({k: f for k, f in zip(ident, fr)})

    def load():
        env.qpos.copy_(_t(torch, np.tile(q, (E, 1))))
        env.qvel.copy_(_t(torch, qvel))
        env.bias_lag.copy_(_t(torch, np.tile(lag, (E, 1))))

    ctrl_t = _t(torch, np.tile(ctrl, (E, 1)))
    out = {}
    for mode in ("on", "off"):
        load()
        if mode == "on":
            env.enable_contact_force(rows=True)
        else:
            env.disable_contact_force()
        env.dyn_substeps(ctrl_t, 1)
        torch.cuda.synchronize()
        out[mode] = [x.cpu().numpy().copy() for x in (env.qpos, env.qvel, env.bias_lag)]
        if mode == "on":
            out["rows"], out["count"] = env.contact_rows.cpu().numpy().copy(), env.contact_count.cpu().numpy().copy()
            out["force"], out["total"] = env.contact_force.cpu().numpy().copy(), env.contact_force_total.cpu().numpy().copy()
    out.update(con=con, ident=ident, ref_f=ref_f, maxcon=int(ct.maxcon), dims=[int(ct.pr_par[p][8]) for p in con_pairs])
    env.close()
    _K7[key] = out
    return out


@pytest.mark.parametrize("env_name", [PUSH, LIFT])
def test_k7_contacts_sum_and_states(torch_mod, env_name):
    """count and the set of (pair, feature) per env = the oracle's detection at the state the sub-step starts from; contact_force = the
    host's sum over the returned rows, bit for bit; qpos / qvel / bias_lag bit-identical with the readout on and off"""
    from contact_force_ref import force_of_rows
    c = _k7_case(torch_mod, env_name, "elliptic")
    assert len(c["con"]) >= 3                      # (asserted by the CPU test for these states: no env is empty)
    assert tuple(c["rows"].shape) == (8, c["maxcon"], 8)
    for e in range(8):
        n = int(c["count"][e])
        assert n == len(c["con"]), (e, n, len(c["con"]))
        got = {(int(r[0]), int(r[1])) for r in c["rows"][e, :n]}
        assert len(got) == n and got == set(c["ident"]), (e, got, c["ident"])
        host = force_of_rows(c["rows"][e, :n])
        print(f"K7 {env_name} env {e}: {n} contacts, force {float(c['force'][e])!r}")
        assert host > 0.0 and np.array_equal(_bits(c["force"][e]), _bits(host)), (e, c["force"][e], host)
        assert np.array_equal(_bits(c["total"][e]), _bits(0.0 + host)), e
        # condim-4 contacts: f4, f5 are padding
        assert (c["rows"][e, :n, 6:] == 0.0).all()
    for a, b, what in zip(c["on"], c["off"], ("qpos", "qvel", "bias_lag")):
        assert np.array_equal(_bits(a), _bits(b)), what


@pytest.mark.parametrize("env_name,form", [(PUSH, "elliptic"), (LIFT, "elliptic"), (PUSH, "newton-pyramidal"), (PUSH, "pgs")])
def test_k7_forces_equal_the_independent_solve(torch_mod, env_name, form):
    """rows matched by (pair, feature) against tests/dyn_ref.contact_step_reference's forces of the same sub-step (elliptic: the
    contact's four solver forces; pyramidal: its edge forces decoded by the rows' formula).  The solve stops on its own criterion,
    so agreement is not exact: the bound is 10 x the largest deviation measured (FORCE_BOUND), never above 1e-3 -- a wrong row
    order or a missing mu is an O(1) error."""
    c = _k7_case(torch_mod, env_name, form)
    worst, torsion = 0.0, 0
    for k in range(4):
        ref = c["ref_f"][k]
        fmax = max(np.abs(f).max() for f in ref.values())
        assert fmax > 0.0
        for e in (2 * k, 2 * k + 1):
            n = int(c["count"][e])
            assert n == len(ref)
            dev = 0.0
            for r in c["rows"][e, :n]:
                f_ref = ref[(int(r[0]), int(r[1]))]
                dev = max(dev, float(np.abs(r[2:2 + len(f_ref)] - f_ref).max()))
            print(f"K7 {env_name} {form} velocity case {k} env {e}: max|f_gpu - f_ref| / max|f_ref| = {dev / fmax:.3e} (max|f_ref| {fmax:.4g})")
            worst = max(worst, dev / fmax)
        if form == "elliptic":
            n = int(c["count"][2 * k])
            torsion += int(np.abs(c["rows"][2 * k, :n, 5]).max() > 1e-6)
    print(f"K7 {env_name} {form}: worst {worst:.3e}")
    bound = FORCE_BOUND[form]
    assert bound is not None and bound <= FORCE_CAP
    assert worst <= bound, (worst, bound)
    if form == "elliptic":
        assert all(d == 4 for d in c["dims"])
        assert torsion >= 3, torsion          # the torsional row carries force: condim 4 is really exercised


def _push_env(torch, E=8, **kw):
    from mopa_rl_amd.kinematic_env import make_env
    return make_env(PUSH, E, dynamics=True, contacts=True, seed=5, **kw)


def test_k7_weight_of_the_resting_cube(torch_mod):
    """Push, default options, 4 env.steps with the zero action from reset: the normal forces of the cube's contacts add up to its weight"""
    torch = torch_mod
    env = _push_env(torch)
    env.enable_contact_force(rows=True)
    env.reset()
    act = torch.zeros(8, env.action_dim, dtype=torch.float64, device="cuda")
    for _ in range(4):
        env.step(act)
    torch.cuda.synchronize()
    ct, nd = env.ct, env.dyn.nd
    on_obj = np.array([(ct.sh_body[int(a)] == nd) or (ct.sh_body[int(b)] == nd) for a, b in zip(ct.pr_f, ct.pr_s)])
    W = float(ct.obj_mass) * 9.81
    rows, cnt = env.contact_rows.cpu().numpy(), env.contact_count.cpu().numpy()
    for e in range(8):
        r = rows[e, :int(cnt[e])]
        r = r[on_obj[r[:, 0].astype(int)]]
        fn = float(r[:, 2].sum())
        print(f"K7 resting cube env {e}: {len(r)} cube contacts, sum f0 = {fn!r}, m g = {W!r}, relative deviation {abs(fn - W) / W:.3e}")
        assert len(r) >= 3 and (r[:, 2] > 0.0).all()
        assert abs(fn - W) <= WEIGHT_BOUND * W, (e, fn, W)
    env.close()


def test_k7_two_runs_and_two_streams_write_the_same_bytes(torch_mod):
    torch = torch_mod
    env = _push_env(torch)
    env.enable_contact_force(rows=True)
    env.reset()
    state = [x.clone() for x in (env.qpos, env.qvel, env.bias_lag, env.prev_state, env.has_prev, env.ep_len)]
    rng = np.random.default_rng(2)
    act = _t(torch, rng.uniform(-1, 1, size=(8, env.action_dim)))
    side = torch.cuda.Stream()
    outs = []
    for stream in (None, None, side):
        for dst, src in zip((env.qpos, env.qvel, env.bias_lag, env.prev_state, env.has_prev, env.ep_len), state):
            dst.copy_(src)
        for t in (env.contact_force, env.contact_force_total, env.contact_count, env.contact_rows):
            t.zero_()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        env.step(act, stream=stream)
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        outs.append([x.cpu().numpy().copy() for x in (env.contact_force, env.contact_force_total, env.contact_rows, env.qpos, env.qvel)]
                    + [env.contact_count.cpu().numpy().copy()])
    assert (outs[0][0] > 0.0).all()
    for o in outs[1:]:
        for a, b in zip(outs[0][:5], o[:5]):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(outs[0][5], o[5])
    env.close()


def test_abi_refuses_what_it_cannot_serve(torch_mod):
    """status codes, not crashes: rows with K below maxcon, force NULL with another pointer set, envs without a solver-backed stage;
    the contact-free 16-lane form accepts the call and reports zeros"""
    torch = torch_mod
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    from mopa_rl_amd.kinematic_env import make_env
    L = _lib.lib()
    env = _push_env(torch, E=4)
    K = env.ct.maxcon
    buf = torch.zeros(4 * K * 8, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert L.mopa_env_set_contact_force(env._h, _ptr(buf), None, _ptr(buf), None, K - 1) == 1
    assert L.mopa_env_set_contact_force(env._h, None, _ptr(buf), None, None, 0) == 1
    assert L.mopa_env_set_contact_force(env._h, None, None, None, _ptr(cnt), 0) == 1
    assert L.mopa_env_set_contact_force(env._h, _ptr(buf), None, None, None, 0) == 0          # force alone
    assert L.mopa_env_set_contact_force(env._h, None, None, None, None, 0) == 0               # off
    env.close()
    for kw in ({}, {"dynamics": True}, {"dynamics": True, "contacts": "penalty"}):
        e = make_env(PUSH, 4, **kw)
        f = torch.zeros(4, dtype=torch.float64, device="cuda")
        assert L.mopa_env_set_contact_force(e._h, _ptr(f), None, None, None, 0) == 1, kw
        with pytest.raises(_lib.MopaError):
            e.enable_contact_force()
        e.close()
    e = make_env(PUSH, 4, dynamics=True, dyn_lanes=16, seed=1)
    e.enable_contact_force(rows=True)
    e.reset()
    e.contact_force.fill_(7.0)
    e.contact_count.fill_(7)
    e.step(torch.zeros(4, e.action_dim, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert float(e.contact_force.abs().max()) == 0.0 and int(e.contact_count.abs().max()) == 0
    e.close()


# ---- rollout --------------------------------------------------------------------------------------------------------------------
def _episode(torch, env_name, env_kw, cfg_kw, prepare=None):
    """run_episode with a fixed scripted policy; every stepping launch of the env is logged (move mask, contact_force, done)"""
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    E = 4
    env = make_env(env_name, E, seed=7, max_episode_steps=4, **env_kw)
    env.reset()
    if prepare is not None:
        prepare(env)
    ro = BatchMoPARollout(env, RolloutConfig.for_env(env_name, **cfg_kw))
    rng = np.random.default_rng(13)
    AC = rng.uniform(-1, 1, size=(8, E, ro.ac_dim))
    AC[:, :2] *= 0.9 * ro.cfg.omega          # envs 0, 1: every entry below omega -> direct steps; envs 2, 3: mostly planner steps
    ACt = _t(torch, AC)
    log, calls = [], {"t": 0}
    orig = env._launch

    def launch(action, is_planner, move_mask, stream=None):
        orig(action, is_planner, move_mask, stream)
        if action is not None and env.contact_force is not None:
            mm = np.ones(E, dtype=np.uint8) if move_mask is None else move_mask.cpu().numpy().copy()
            log.append((mm, env.contact_force.cpu().numpy().copy(), env.done.cpu().numpy().copy()))

    env._launch = launch

    def policy(ob, is_train=True, random_exploration=False):
        t = calls["t"]
        calls["t"] += 1
        return ACt[min(t, len(AC) - 1)].clone()

    rollout, info = ro.run_episode(policy, reset=False)
    torch.cuda.synchronize()
    return env, ro, log, info


def _episode_check(torch, env, log, info):
    E = 4
    want, alive, nstep = np.zeros(E), np.ones(E, dtype=bool), np.zeros(E, dtype=int)
    for mm, force, done in log:
        for e in range(E):
            if not alive[e] or (mm[e] & 2):
                continue
            if mm[e] & 1:          # the env ran its sub-steps in this launch: `contact_force += env.get_contact_force()`
                want[e] = want[e] + float(force[e])
                nstep[e] += 1
            if done[e]:
                alive[e] = False
    got = info["contact_force"].cpu().numpy()
    ln = info["len"].cpu().numpy()
    total = float(env.contact_force_total.max())
    # a step's force is (total after) - (total before) of the env's device-side accumulator: every add rounds to half an ulp of the
    # running total, at most two roundings per launch and one per difference -- bounded by 4 x launches x 2^-53 x the largest total
    tol = 4 * max(len(log), 1) * 2.0 ** -53 * total
    print(f"episode: contact_force {got}, sum of env.contact_force over the step launches {want}, len {ln}, tol {tol:.3e}")
    assert (nstep >= 1).all()
    assert np.abs(got - want).max() <= tol, (got, want, tol)
    avg = info["avg_conntact_force"].cpu().numpy()
    assert np.array_equal(_bits(avg), _bits(got / ln.astype(np.float64)))
    return want


def test_run_episode_reports_contact_force_k7(torch_mod):
    torch = torch_mod
    env, ro, log, info = _episode(torch, PUSH, dict(dynamics=True, contacts=True),
                                  dict(timelimit=0.1, max_nodes=512, max_path=64, num_trials=10))
    assert env.contact_force is not None               # the rollout enabled the readout
    want = _episode_check(torch, env, log, info)
    assert (want > 0.0).all()                          # the cube rests on the table in every env
    # agent_step reports the force of the step
    out = ro.agent_step(torch.zeros(4, ro.ac_dim, dtype=torch.float64, device="cuda"))
    assert "contact_force" in out and tuple(out["contact_force"].shape) == (4,)
    assert bool((out["contact_force"][out["stepped"].bool()] > 0).all())
    env.close()
    ro.close()


def test_run_episode_reports_contact_force_k8(torch_mod):
    torch = torch_mod

    def prepare(env):          # envs 0 / 1 start from the two committed contact states
        q = env.qpos.cpu().numpy().copy()
        q[0, env.pdyn.qadr], q[1, env.pdyn.qadr] = Q_TIP_IN_BOX, Q_BOX_IN_OBSTACLE
        env.set_state(_t(torch, q))

    env, ro, log, info = _episode(torch, PUSHER, dict(dynamics=True, contacts=True),
                                  dict(timelimit=0.1, max_nodes=512, max_path=64, num_trials=10), prepare)
    want = _episode_check(torch, env, log, info)
    assert want[0] > 0.0 and want[1] > 0.0
    env.close()
    ro.close()


def test_run_episode_on_a_kinematic_env_has_no_contact_force(torch_mod):
    torch = torch_mod
    env, ro, log, info = _episode(torch, PUSH, {}, dict(timelimit=0.1, max_nodes=512, max_path=64, num_trials=10))
    assert "contact_force" not in info and "avg_conntact_force" not in info
    assert env.contact_force is None
    out = ro.agent_step(torch.zeros(4, ro.ac_dim, dtype=torch.float64, device="cuda"))
    assert "contact_force" not in out
    env.close()
    ro.close()
