"""The host halves of env, IK and dynamics creation (no GPU): mopa_env_tables_host / mopa_ik_tables_host / mopa_dyn_tables_host
reproduce, for the shipped envs, the fingerprints of the tables recorded before the three compilers were folded onto the shared
model check and body-walk compiler (csrc/mopa_model_host.hpp); and what the scene compiler refuses of a malformed model's bodies,
joints and geom_body, they and mopa_env_create / mopa_ik_create refuse with the same code and text, before any device is looked for.

tests/golden/env_tables.json is recorded by running this module as a script (it rewrites the file from the library in use:
MOPA_HIP_LIB selects the build)."""
import copy
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_scenes as RS  # noqa: E402
from test_random_scenes_host import _malformed  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "env_tables.json")
SAWYER = ["SawyerPushObstacle-v0", "SawyerLiftObstacle-v0", "SawyerAssemblyObstacle-v0"]
ENVS = SAWYER + ["PusherObstacle-v0"]
# the IK site of the MoPA + IK rollouts per env (RolloutConfig.ik_target, rollout.IK_ENV_DEFAULTS): Pusher's is the 2-D one
IK_SITE = {env: "fingertip" if env == "PusherObstacle-v0" else "grip_site" for env in ENVS}
# the structure cases of test_random_scenes_host._malformed(): bodies, joints, geom_body
STRUCTURE = ["geom_body beyond nbody", "geom_body negative", "body_parent beyond nbody", "body_parent negative", "body_parent[b] == b",
             "body_parent[b] > b", "body_jntnum beyond njnt", "body_jntadr beyond njnt", "body_jntnum negative", "jnt_qposadr beyond nq",
             "jnt_qposadr negative", "bodies breadth-first", "free joint with 6 slots left"]


def _u64():
    return C.c_uint64(0)


# ---------------- descriptions of the shipped envs, as BatchKinematicEnv / BatchIK fill them ----------------
@functools.lru_cache(maxsize=None)
def _shipped(env):
    from mopa_rl_amd.kinematic_env import env_facts
    from mopa_rl_amd.scene import ENV_SPECS, load_scene
    spec = ENV_SPECS[env]
    model = load_scene(spec.scene)
    return spec, model, env_facts(env, model)


def shipped_env_desc(env):
    from mopa_rl_amd.kinematic_env import env_desc
    spec, model, facts = _shipped(env)
    pusher = env == "PusherObstacle-v0"
    return env_desc(model, facts, ac_scale=spec.ac_scale, distance_threshold=0.05 if pusher else 0.06, success_reward=150.0,
                    max_episode_steps=150 if pusher else 250)


def shipped_dyn_desc(env, penalty=False):
    from mopa_rl_amd.dynamics import dyn_facts, obj_facts
    from mopa_rl_amd.kinematic_env import dyn_desc
    _, model, facts = _shipped(env)
    df = dyn_facts(model, facts, frame_dt=0.15)
    return dyn_desc(df, obj_facts(model, df) if penalty else None)


def env_tables(desc):
    from mopa_rl_amd import _lib
    fp, nb, ns = _u64(), C.c_int32(-1), C.c_int32(-1)
    _lib.check(_lib.lib().mopa_env_tables_host(C.byref(desc), C.byref(fp), C.byref(nb), C.byref(ns)))
    return dict(fingerprint="%016x" % fp.value, nb=nb.value, n_save=ns.value)


def ik_tables(desc):
    from mopa_rl_amd import _lib
    fp, nb = _u64(), C.c_int32(-1)
    _lib.check(_lib.lib().mopa_ik_tables_host(C.byref(desc), C.byref(fp), C.byref(nb)))
    return dict(fingerprint="%016x" % fp.value, nb=nb.value)


def dyn_tables(edesc, ddesc):
    from mopa_rl_amd import _lib
    fp, ns = _u64(), C.c_int32(-1)
    _lib.check(_lib.lib().mopa_dyn_tables_host(C.byref(edesc), C.byref(ddesc), C.byref(fp), C.byref(ns)))
    return dict(fingerprint="%016x" % fp.value, n_save=ns.value)


def compute():
    """everything the fixture holds, from the library in use"""
    from mopa_rl_amd.ik import ik_desc
    out = {"env": {}, "ik": {}, "dyn": {}}
    for env in ENVS:
        spec, model, _ = _shipped(env)
        edesc, keep = shipped_env_desc(env)
        out["env"][env] = env_tables(edesc)
        idesc, ikeep = ik_desc(model, IK_SITE[env], spec.robot_joints)
        out["ik"][f"{env} {IK_SITE[env]}"] = ik_tables(idesc)
        if env in SAWYER:
            ddesc, dkeep = shipped_dyn_desc(env)
            out["dyn"][env] = dyn_tables(edesc, ddesc)
    edesc, keep = shipped_env_desc(SAWYER[0])
    ddesc, dkeep = shipped_dyn_desc(SAWYER[0], penalty=True)
    out["dyn"][SAWYER[0] + " penalty object"] = dyn_tables(edesc, ddesc)
    return out


@pytest.fixture(scope="module")
def clean_knobs():
    """(MOPA_IK_NO_PREFIX changes the IK header)"""
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]}
    yield
    os.environ.update(saved)


def test_tables_equal_the_recorded_ones(clean_knobs):
    with open(GOLDEN) as f:
        recorded = json.load(f)
    got = compute()
    assert sorted(got["env"]) == sorted(ENVS) and len(got["ik"]) == 4 and len(got["dyn"]) == 4
    assert got == recorded


# what env_lds_bytes (mopa_env.inc) makes of the walk the host half reports: (max(n_save, 1) * 7 + n_touch * 12) * 64 doubles; the
# values are the library's before the compilers were shared
@pytest.mark.parametrize("env,nb,n_save,n_touch,lds", [("SawyerPushObstacle-v0", 15, 1, 0, 3584), ("SawyerLiftObstacle-v0", 19, 1, 7, 46592),
                                                       ("SawyerAssemblyObstacle-v0", 14, 0, 0, 3584)])
def test_sawyer_walks_keep_their_lds_sizes(env, nb, n_save, n_touch, lds):
    edesc, keep = shipped_env_desc(env)
    t = env_tables(edesc)
    assert (t["nb"], t["n_save"]) == (nb, n_save)
    assert len(_shipped(env)[2].touch_geom) == n_touch
    assert (max(t["n_save"], 1) * 7 + n_touch * 12) * 64 * 8 == lds


# ---------------- a push env and an IK site on a scene that is none of the shipped ones ----------------
def tree_bodies(m):
    """the bodies of random_scenes' moving tree (hinge / slide joints), in body order, and the free body behind them"""
    first = [int(m.jnt_type[m.body_jntadr[b]]) if m.body_jntnum[b] else -1 for b in range(len(m.body_parent))]
    return [b for b, t in enumerate(first) if t in (RS.JNT_HINGE, RS.JNT_SLIDE)], [b for b, t in enumerate(first) if t == RS.JNT_FREE]


def deep_facts(m):
    """EnvFacts of kind push on random_scenes.deep_branches (tree parents [-1, 0, 1, 2, 3, 2, 1, 6, 0, 8]): no gripper, the arm = the first
    seven hinge / slide coordinates, the frames on five branches (the free body among them, as the cube is in the shipped env)"""
    from mopa_rl_amd.kinematic_env import KIND_PUSH, EnvFacts
    from mopa_rl_amd.scene import qpos_joint_arrays
    tree, free = tree_bodies(m)
    assert len(tree) == 10 and len(free) == 1
    arm = np.array([m.jnt_qposadr[j] for j in range(len(m.jnt_type)) if m.jnt_type[j] in (RS.JNT_HINGE, RS.JNT_SLIDE)][:7], dtype=np.int32)
    arm_j = [int(np.nonzero(np.asarray(m.jnt_qposadr) == a)[0][0]) for a in arm]
    lim = np.asarray(m.jnt_limited)[arm_j] == 1
    rng = np.random.default_rng(5)
    jidx, jlo, jhi, jlim = qpos_joint_arrays(m)
    return EnvFacts(
        kind=KIND_PUSH, arm_qpos_idx=arm, grip_qpos_idx=np.zeros(0, dtype=np.int32), act_qpos_idx=arm.copy(),
        act_lo=np.where(lim, 0.8 * m.jnt_range[arm_j, 0], -np.inf), act_hi=np.where(lim, 0.8 * m.jnt_range[arm_j, 1], np.inf),
        frame_body=np.array([tree[4], tree[5], tree[7], free[0], tree[9]], dtype=np.int32), frame_off=rng.uniform(-0.05, 0.05, (5, 3)),
        quat_body=np.array([tree[4], free[0]], dtype=np.int32), touch_geom=np.zeros(0, dtype=np.int32), n_touch_left=0,
        qpos_min=jlo[jidx].astype(np.float64), qpos_max=jhi[jidx].astype(np.float64), qpos_limited=jlim[jidx].astype(np.int32),
        reset_jitter_idx=np.zeros(0, dtype=np.int64))


DEEP_ENV = dict(ac_scale=0.05, distance_threshold=0.06, success_reward=150.0, max_episode_steps=250)


def deep_site(m):
    """(model with a site "tip" on it, the site's movable joints by name): the site sits on the deepest body whose ancestor chain
    carries at most one joint per body and three to eight hinge / slide joints"""
    best = None
    for b in range(1, len(m.body_parent)):
        chain = []
        c = b
        while c > 0:
            chain.append(c)
            c = int(m.body_parent[c])
        joints = [int(m.body_jntadr[c]) for c in reversed(chain) if m.body_jntnum[c] == 1]
        ok = all(m.body_jntnum[c] <= 1 for c in chain) and 3 <= len(joints) <= 8 and all(m.jnt_type[j] in (RS.JNT_HINGE, RS.JNT_SLIDE) for j in joints)
        if ok and (best is None or len(chain) > best[1]):
            best = (b, len(chain), joints)
    assert best is not None
    m2 = copy.copy(m)
    m2.site_names = ["tip"]
    m2.site_body = np.array([best[0]], dtype=np.int32)
    m2.site_pos = np.array([[0.03, -0.02, 0.05]])
    m2.site_quat = np.array([[np.cos(0.2), 0.0, np.sin(0.2), 0.0]])
    return m2, [m.jnt_names[j] for j in best[2]]


def _site_on(m, like):
    m2 = copy.copy(m)
    for k in ("site_names", "site_body", "site_pos", "site_quat"):
        setattr(m2, k, getattr(like, k))
    return m2


def test_deep_branches_env_and_ik_compile():
    from mopa_rl_amd.ik import ik_desc
    from mopa_rl_amd.kinematic_env import env_desc
    m, _ = RS.scene("deep_branches")
    edesc, keep = env_desc(m, deep_facts(m), **DEEP_ENV)
    t = env_tables(edesc)
    assert t["n_save"] >= 2 and t["nb"] >= 8
    ms, joints = deep_site(m)
    assert 3 <= len(joints) <= 8
    idesc, ikeep = ik_desc(ms, "tip", joints)
    assert ik_tables(idesc)["nb"] == len(joints)      # (every body of the tree carries one joint; the chain starts at the world)


@pytest.mark.parametrize("case", STRUCTURE)
def test_malformed_models_are_refused_by_env_and_ik(case):
    from mopa_rl_amd import _lib
    from mopa_rl_amd.ik import ik_desc
    from mopa_rl_amd.kinematic_env import env_desc
    good, _ = RS.scene("deep_branches")
    model, _, code, text = _malformed()[case]
    L = _lib.lib()
    ms, joints = deep_site(good)
    edesc, keep = env_desc(model, deep_facts(good), **DEEP_ENV)
    idesc, ikeep = ik_desc(_site_on(model, ms), "tip", joints)

    def refused(rc):
        assert rc == code and text in L.mopa_last_error().decode(), (rc, L.mopa_last_error().decode())

    refused(L.mopa_env_tables_host(C.byref(edesc), None, None, None))
    refused(L.mopa_ik_tables_host(C.byref(idesc), None, None))
    # creation compiles on the host before it looks for a device: the same refusal, with or without a GPU
    for create, desc in ((L.mopa_env_create, edesc), (L.mopa_ik_create, idesc)):
        h = C.c_void_p(1)
        refused(create(C.byref(desc), C.byref(h)))
        assert not h.value


def test_every_structure_case_of_the_scene_is_taken():
    cases = _malformed()
    mine = [k for k in cases if k.startswith(("body_", "jnt_qposadr", "geom_body")) or k in ("bodies breadth-first", "free joint with 6 slots left")]
    assert sorted(mine) == sorted(STRUCTURE)


def test_valid_descriptions_end_at_the_device_or_succeed():
    """without a GPU a valid description still ends in "no HIP device"; with one it is created"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.kinematic_env import env_desc
    m, _ = RS.scene("deep_branches")
    L = _lib.lib()
    edesc, keep = env_desc(m, deep_facts(m), **DEEP_ENV)
    h = C.c_void_p()
    rc = L.mopa_env_create(C.byref(edesc), C.byref(h))
    if L.mopa_device_count() == 0:
        assert rc == 3 and not h.value and "no HIP device" in L.mopa_last_error().decode()
    else:
        assert rc == 0 and h.value
        L.mopa_env_destroy(h)


# ---------------- the dynamic tree: depth-first order is checked, not assumed ----------------
def _four_dofs(parent):
    """the Push env's dynamics description cut down to its first four dofs, with `parent` as their tree"""
    from mopa_rl_amd.dynamics import dyn_facts
    from mopa_rl_amd.kinematic_env import dyn_desc, env_desc
    import dataclasses
    spec, model, facts = _shipped(SAWYER[0])
    df = dyn_facts(model, facts, frame_dt=0.15)
    assert list(df.qadr[:4]) == list(facts.arm_qpos_idx[:4])
    f4 = dataclasses.replace(facts, arm_qpos_idx=facts.arm_qpos_idx[:4], grip_qpos_idx=facts.grip_qpos_idx[:0], act_qpos_idx=facts.act_qpos_idx[:4],
                             act_lo=facts.act_lo[:4], act_hi=facts.act_hi[:4])
    d4 = dataclasses.replace(df, nd=4, parent=np.array(parent, dtype=np.int32))
    edesc, keep = env_desc(model, f4, ac_scale=spec.ac_scale)
    ddesc, dkeep = dyn_desc(d4)
    return edesc, ddesc, (keep, dkeep)


def test_breadth_first_dof_list_is_refused():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    edesc, ddesc, keep = _four_dofs([-1, 0, 0, 1])          # a breadth-first numbering of a branching tree
    fp, ns = _u64(), C.c_int32(-1)
    assert L.mopa_dyn_tables_host(C.byref(edesc), C.byref(ddesc), C.byref(fp), C.byref(ns)) == 2      # MOPA_ERR_UNSUPPORTED
    assert "bodies are not in depth-first order" in L.mopa_last_error().decode()
    edesc, ddesc, keep = _four_dofs([-1, 0, 1, 0])          # its depth-first renumbering
    assert dyn_tables(edesc, ddesc)["n_save"] == 1


if __name__ == "__main__":
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        del os.environ[k]
    with open(GOLDEN, "w") as f:
        json.dump(compute(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
