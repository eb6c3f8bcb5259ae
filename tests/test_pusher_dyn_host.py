"""K8 host side (no GPU): the facts `dynamics.pusher_dyn_facts` compiles from the committed Pusher scene, the sequential checker
tests/pusher_dyn_ref.py (its PID against the reference's own `_step`, its contact-free trajectory against an independent RK4,
hand-built contacts), and the C ABI of the new entry points."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def model():
    from mopa_rl_amd.scene import ENV_SPECS, load_scene
    return load_scene(ENV_SPECS["PusherObstacle-v0"].scene)


@pytest.fixture(scope="module")
def facts(model):
    from mopa_rl_amd.dynamics import pusher_dyn_facts
    return pusher_dyn_facts(model)


ARM = ["link0", "link1", "link2", "link3", "fingertip0", "fingertip1", "fingertip2"]
OBST = [f"obstacle{k}_geom" for k in range(1, 8)]


def _expected_pairs():
    """the compiled candidates that touch a simulated body and can meet in z: non-adjacent arm capsules, arm x box, arm x
    obstacles, box x obstacles (body3 / fingertip are one weld, body2 / fingertip adjacent through it)"""
    out = [("link0", g) for g in ["link2", "link3", "fingertip0", "fingertip1", "fingertip2", "box"] + OBST]
    out += [("link1", g) for g in ["link3", "fingertip0", "fingertip1", "fingertip2", "box"] + OBST]
    for a in ARM[2:]:
        out += [(a, g) for g in ["box"] + OBST]
    out += [("box", g) for g in OBST]
    return out


def test_facts_tree_actuators_and_substeps(facts, model):
    f = facts
    assert f.dof_names == ("joint0", "joint1", "joint2", "joint3", "box_x", "box_y")
    jn = list(model.jnt_names)
    assert list(f.qadr) == [int(model.jnt_qposadr[jn.index(n)]) for n in f.dof_names]
    assert list(f.act_kind) == [2] * 4 and list(f.gear) == [10.0] * 4 and list(f.kv) == [1.0] * 4
    assert list(f.ctrl_lo) == [-1.0] * 4 and list(f.ctrl_hi) == [1.0] * 4
    assert list(f.damping) == [1.0] * 6 and list(f.armature) == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0]      # pusher_gripper.xml:9, :109-110
    assert list(f.limited) == [0, 1, 1, 1, 1, 1]
    assert list(f.lo[1:]) == [-3.0, -3.0, -3.0, -0.4, -0.4] and list(f.hi[1:]) == [3.0, 3.0, 3.0, 0.4, 0.4]
    assert f.integrator == "RK4" and f.timestep == 0.01 and f.frame_dt == 1.0
    assert int(1.0 / 0.01) == 100 and f.nsub == 100
    assert (f.kp, f.kd, f.ki, f.alpha) == (150.0, 20.0, 0.1, 0.95)
    assert f.iterations == 100 and f.tolerance == 1e-8 and f.maxcon == 16
    # masses from the compiled scene: body3 carries the welded fingertip
    nb = list(model.body_names)
    assert f.mass[0] == model.body_mass[nb.index("body0")]
    assert math.isclose(f.mass[3], model.body_mass[nb.index("body3")] + model.body_mass[nb.index("fingertip")], rel_tol=1e-15)
    assert f.box_mass == model.body_mass[nb.index("box")]


def test_contact_pair_list_is_pinned(facts):
    assert facts.pair_names == _expected_pairs()
    assert len(facts.pairs) == 72 and facts.pairs.shape[1] == 20
    from mopa_rl_amd.dynamics import PAIR_BOX_BOX, PAIR_CAPSULE_BOX, PAIR_CAPSULE_CAPSULE
    for (a, b), r in zip(facts.pair_names, facts.pairs):
        want = PAIR_BOX_BOX if a == "box" else (PAIR_CAPSULE_BOX if (b == "box" or b in OBST) else PAIR_CAPSULE_CAPSULE)
        assert int(r[0]) == want
        assert r[13] == 1.0                 # friction: max of the two geoms' (1 everywhere in this scene)


def test_dropped_pairs_never_meet_in_z(facts, model):
    """a compiled candidate is left out only when no simulated body is in it, or when its geoms' z-extents -- fixed, since all
    motion is planar -- cannot overlap; both proven here from the compiled scene itself"""
    names = [model.all_geom_names[int(i)] for i in model.geom_mjid]
    nb = list(model.body_names)

    def zrange(g):
        b, z = int(model.geom_body[g]), float(model.geom_pos[g][2])
        while b > 0:
            z += float(model.body_pos[b][2])
            b = int(model.body_parent[b])
        t, s = int(model.geom_type[g]), model.geom_size[g]
        half = {3: s[0], 5: s[1], 6: s[2]}[t]          # capsule in the plane: radius; cylinder: half-height; box: half z
        return z - half, z + half

    kept = set(facts.pair_names)
    n = 0
    for a, b in model.pair_geom:
        na, nb_ = names[int(a)], names[int(b)]
        if (na, nb_) in kept or (nb_, na) in kept:
            continue
        n += 1
        za, zb = zrange(int(a)), zrange(int(b))
        sim = {nb.index(x) for x in ("body0", "body1", "body2", "body3", "fingertip", "box")}
        on_sim = int(model.geom_body[int(a)]) in sim or int(model.geom_body[int(b)]) in sim
        assert (not on_sim) or za[1] <= zb[0] or zb[1] <= za[0], (na, nb_, za, zb)
    assert n == len(facts.dropped_pairs) == 15


def test_pid_reproduces_the_reference_step_bit_for_bit(facts):
    """tests/golden/ref_py_pusher_pid.npz: the reference's own `_step` + `_get_control` over a scripted sim (tools/gen_ref_py_golden.py
    pusher_pid).  The checker's PID, driven by the same desired-state rule and the same scripted update, gives every ctrl,
    prev_state and i_term bit for bit."""
    from pusher_dyn_ref import PusherRef
    g = np.load(os.path.join(GOLDEN, "ref_py_pusher_pid.npz"))
    ref = PusherRef(facts)
    adr = [int(a) for a in g["arm_qpos_idx"]]
    prev = None
    it = [0.0] * 4
    for t in range(len(g["action"])):
        q = [float(x) for x in g["qpos0"][t][adr]]
        v = [float(x) for x in g["qvel0"][t][adr]]
        if g["reset_prev"][t]:
            prev = None
        is_planner = bool(g["is_planner"][t])
        if not is_planner or prev is None:
            prev = list(q)
        desired = [prev[j] + float(g["action"][t][j]) for j in range(4)]
        tv0 = [((desired[j] - prev[j]) / facts.frame_dt) * 0.0 for j in range(4)]
        for k in range(g["ctrl"].shape[1]):
            ctrl = ref.pid(q, v, it, desired, prev, tv0)
            assert np.array_equal(np.array(ctrl).view(np.uint64), g["ctrl"][t][k].view(np.uint64)), (t, k)
            v = [0.02 * c for c in ctrl]
            q = [q[j] + 0.01 * v[j] for j in range(4)]
        prev = desired
        assert np.array_equal(np.array(prev).view(np.uint64), g["prev_state"][t].view(np.uint64)), t
        assert np.array_equal(np.array(it).view(np.uint64), g["i_term"][t].view(np.uint64)), t


def test_contact_free_arm_matches_an_independent_rk4(model):
    """contacts off, the box at rest: one env.step of the checker against RK4 over tests/dyn_ref.py's mass matrix / bias force
    (the general 3-D tree), with the same PID and actuator law"""
    from dyn_ref import bias_force, mass_matrix
    from mopa_rl_amd.dynamics import pusher_dyn_facts
    from pusher_dyn_ref import PusherRef
    f = pusher_dyn_facts(model, contacts=False)
    ref = PusherRef(f)
    nb = list(model.body_names)
    bodies = [nb.index(x) for x in ("body0", "body1", "body2", "body3")]
    arm_ad = [int(a) for a in f.qadr[:4]]
    rng = np.random.default_rng(0)
    q0 = np.array(model.qpos0, dtype=np.float64)
    q0[arm_ad] = rng.uniform(-0.5, 0.5, size=4)
    v0 = rng.uniform(-0.1, 0.1, size=4)
    prev = q0[arm_ad].copy()
    desired = prev + np.array([0.3, -0.2, 0.25, -0.1])
    # the checker
    row, v, _ = ref.run_rows(q0, np.concatenate([v0, [0.0, 0.0]]), np.zeros(4), desired, prev, f.nsub)
    # independent: numpy RK4, same PID / actuator law, M and bias from dyn_ref (3-D rigid-body formulas)
    arm = np.asarray(f.armature[:4])

    def acc(q, qd, ctrl):
        row_ = q0.copy()
        row_[arm_ad] = q
        M, _ = mass_matrix(model, row_, bodies, arm)
        c = bias_force(model, row_, qd, bodies, arm_ad, arm)
        u = np.clip(ctrl, -1.0, 1.0)
        tau = 10.0 * (1.0 * u - 10.0 * qd) - 1.0 * qd - c
        return np.linalg.solve(M, tau)

    q, qd, it = q0[arm_ad].copy(), v0.copy(), np.zeros(4)
    h = 0.01
    for _ in range(f.nsub):
        it = 0.95 * it + 0.1 * (prev - q)
        ctrl = 150.0 * (desired - q) + 20.0 * (0.0 - qd) + it
        k1v, k1a = qd, acc(q, qd, ctrl)
        k2v, k2a = qd + 0.5 * h * k1a, acc(q + 0.5 * h * k1v, qd + 0.5 * h * k1a, ctrl)
        k3v, k3a = qd + 0.5 * h * k2a, acc(q + 0.5 * h * k2v, qd + 0.5 * h * k2a, ctrl)
        k4v, k4a = qd + h * k3a, acc(q + h * k3v, qd + h * k3a, ctrl)
        q = q + h / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v)
        qd = qd + h / 6.0 * (k1a + 2 * k2a + 2 * k3a + k4a)
    assert np.abs(row[arm_ad] - q).max() <= 1e-10, row[arm_ad] - q
    assert np.abs(np.asarray(v[:4]) - qd).max() <= 1e-10
    assert list(row[[int(a) for a in f.qadr[4:]]]) == list(q0[[int(a) for a in f.qadr[4:]]])


def _forward_contacts(facts, q):
    from pusher_dyn_ref import PusherRef
    ref = PusherRef(facts)
    qa, C, F = ref.forward(list(q), [0.0] * 6, [0.0] * 4, want=True)
    return ref, C, F


def test_fingertip_pressed_into_the_box(facts):
    """joint3 at pi/2: the fingertip body sits at (0.3, 0.11) pointing +y, so fingertip0 lies along x (0.27 .. 0.33) at y = 0.11;
    the box centred at x = 0.3 with its -y face 2 mm inside that capsule.  The capsule lies along the face: two points (the box's
    two -y corners; the capsule's ends are beyond them), normal -y (from the box to the fingertip), depth 2 mm, midway between
    the surfaces; pyramid forces >= 0 and the box is pushed along +y."""
    q = [0.0, 0.0, 0.0, math.pi / 2, 0.3, 0.11 + 0.02 - 0.002]
    ref, C, F = _forward_contacts(facts, q)
    assert {facts.pair_names[c["pair"]] for c in C} == {("fingertip0", "box")}
    assert len(C) == 2
    for c in C:
        assert abs(c["n"][1] + 1.0) < 1e-12 and abs(c["n"][0]) < 1e-12
        assert abs(c["dist"] + 0.002) < 1e-12
        assert abs(c["pos"][1] - (0.11 + 0.01 - 0.001)) < 1e-12
    assert sorted(round(c["pos"][0], 12) for c in C) == [0.29, 0.31]
    assert all(x >= 0.0 for fr in F for x in fr) and sum(sum(fr) for fr in F) > 0.0
    qacc = ref.forward(list(q), [0.0] * 6, [0.0] * 4)
    assert qacc[5] > 0.0 and abs(qacc[4]) < qacc[5]


def test_box_pressed_into_an_obstacle(facts):
    """the box 2 mm into obstacle7 (centre -0.12, -0.12, half 0.01) from +x: four points at the corners of the overlap rectangle,
    normal +x, depth 2 mm; forces >= 0 push the box back along +x only"""
    q = [0.0, 0.0, 0.0, 0.0, -0.12 + 0.02 - 0.002, -0.12]
    ref, C, F = _forward_contacts(facts, q)
    assert [facts.pair_names[c["pair"]] for c in C] == [("box", "obstacle7_geom")] * 4
    for c in C:
        assert c["n"] == (1.0, 0.0) and abs(c["dist"] + 0.002) < 1e-15
    xs = sorted({round(c["pos"][0], 12) for c in C})
    ys = sorted({round(c["pos"][1], 12) for c in C})
    assert xs == [round(-0.12 + 0.01 - 0.002, 12), -0.11] and ys == [-0.13, -0.11]
    assert all(x >= 0.0 for fr in F for x in fr)
    qacc = ref.forward(list(q), [0.0] * 6, [0.0] * 4)
    assert qacc[4] > 0.0 and qacc[5] == 0.0 and qacc[:4] == [0.0] * 4


def test_abi_symbols_and_descriptor_size():
    from mopa_rl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    new = ["mopa_pusher_dyn_desc_size", "mopa_env_attach_pusher_dynamics", "mopa_env_set_pusher_stats", "mopa_env_pusher_substeps_batch",
           "mopa_env_step_pusher_batch"]
    for sym in new:
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    for sym in new:
        getattr(L, sym)
    assert L.mopa_pusher_dyn_desc_size() == C.sizeof(_lib.MopaPusherDynDesc)
