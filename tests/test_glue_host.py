"""glue_bodies on the host (no GPU): the weld form against the reference's write-back form on the CPU oracle, the glued scene compile
through mopa_scene_k1_export_glued, and the argument handling of PyKinematicPlanner / SamplingBasedPlanner."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import glue_ref as G  # noqa: E402

ENVS = list(G.GLUE_CASES)

# (a): largest |min_dist(weld) - min_dist(write-back)| measured over the three scenes' states below, and the tolerance 16 x that
WELD_MEASURED = 8.06e-14
WELD_TOL = 16 * WELD_MEASURED


def _mju_mulquat(a, b):
    """MuJoCo's mju_mulQuat, one multiplication / addition per operator (no fma)"""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _both_forms(c, qa, ne):
    """(weld verdicts, weld min_dist, write-back verdicts, write-back min_dist) of qa [ne * S, na]: S states of each of the first ne
    env rows.  The write-back pose is computed as MuJoCo would (rotation matrix times vector and mju_mulQuat without fused operations),
    i.e. rounded differently from the weld."""
    S = c.S
    n = ne * S
    full = np.repeat(c.rows[:ne], S, axis=0)
    full[:, c.act] = qa
    gv, gmd = np.zeros(n, dtype=np.uint8), np.zeros(n)
    for e in range(ne):
        sl = slice(e * S, (e + 1) * S)
        gv[sl], gmd[sl] = c.ref(e).orc.is_valid_batch(qa[sl], c.rows[e:e + 1], samples_per_env=S, nthreads=0)
    wb = full.copy()
    for i in range(n):
        ref = c.ref(i // S)
        xp, xq = c.orc.fk_bodies(full[i])       # unglued FK: body_a where the state's joint values put it
        M = np.array(G.quat2mat(xq[c.a])).reshape(3, 3)
        wb[i, c.adr:c.adr + 3] = xp[c.a] + M @ ref.t
        wb[i, c.adr + 3:c.adr + 7] = _mju_mulquat(xq[c.a], ref.rq)
    wv, wmd = c.orc.is_valid_batch(qa, wb, samples_per_env=1, nthreads=0)
    return gv, gmd, wv, wmd


@pytest.mark.parametrize("env", ENVS)
def test_weld_form_against_write_back_form(env, oracle_mod):
    """The reference (GlueTransformation, mujoco_ompl_interface.cpp:810-907) writes body_b's world pose p_a' + R_a' t, q_a' * rq into
    the free joint's qpos and runs the ordinary checker; this project poses body_b as a jointless child of body_a (the weld form).
    2560 states per scene -- the first 10 env rows of the shared glue inputs, 256 perturbations (+-0.3 rad, seed 100) of each row's arm
    pose -- through both forms on the CPU oracle, the write-back pose computed as MuJoCo would (rotation matrix times vector and
    mju_mulQuat without fused operations), i.e. rounded differently from the weld.

    Measured here: the largest |min_dist difference| is 8.06e-14 (Assembly; Push 3.6e-16, Lift 0), the tolerance is 16 x that =
    1.29e-12; no verdict differs and no state lies within the tolerance of the threshold (0 % excluded; the cap is 1 %).
    These states stay near the attach pose.  Further from it the two forms no longer agree in min_dist on every state, only in the
    verdict: test_weld_form_verdicts_on_the_shared_inputs below."""
    c = G.glue_case(oracle_mod, env)
    ne, S = 10, c.S
    n = ne * S
    rng = np.random.default_rng(100)
    qa = np.clip(np.repeat(c.rows[:ne, c.act], S, axis=0) + rng.uniform(-0.3, 0.3, (n, len(c.act))), c.pi.jnt_minimum, c.pi.jnt_maximum)
    gv, gmd, wv, wmd = _both_forms(c, qa, ne)
    diff = np.abs(wmd - gmd)
    band = np.abs(gmd - c.thr) < WELD_TOL
    print(f"{env}: {n} states, {int(gv.sum())} valid; max |min_dist difference| {diff.max():.3g} (tolerance {WELD_TOL:.3g}); "
          f"{int(band.sum())} states within the tolerance of the threshold; verdicts differ on {int((wv != gv).sum())}")
    assert n >= 2000 and 0.05 < gv.mean() < 0.95
    assert diff.max() <= WELD_TOL
    assert band.mean() <= 0.01
    assert np.array_equal(wv[~band], gv[~band])


@pytest.mark.parametrize("env", ENVS)
def test_weld_form_verdicts_on_the_shared_inputs(env, oracle_mod):
    """the same two forms on the inputs the GPU tests use: the 64 env rows of the shared glue case and their 256 states each (+-0.7
    rad; Lift +-1.5 rad), 16384 states per scene.  Only the verdicts are compared: equal on every state outside the tolerance band of
    the threshold, which may hold 1 % of the states at most.

    Measured here: no verdict differs and the band is empty.  min_dist agrees to 3e-12 on all but 79 of the 49152 states (Push 48, Lift
    6, Assembly 25).  On those the penetration depth of the iterative narrow phase is not a continuous function of the pose: the two
    forms' poses differ in the last bits and the depths by up to 8.2e-5 m on Push (45 of the 48 states less than 1 cm deep, 19 of them
    valid), 6.2e-5 m on Lift, 4.9e-2 m on Assembly (all of them at least 4.5 cm deep).  So the forms are verdict-equal on what was
    measured, and min_dist-equal outside such states -- not equal up to rounding everywhere."""
    c = G.glue_case(oracle_mod, env)
    ne = c.E
    qa = c.qa
    gv, gmd, wv, wmd = _both_forms(c, qa, ne)
    band = np.abs(gmd - c.thr) < WELD_TOL
    shallow = np.minimum(gmd, wmd) > -0.1
    print(f"{env}: {len(gv)} states, {int(gv.sum())} valid; verdicts differ on {int((wv != gv).sum())}; max |min_dist difference| "
          f"{np.abs(wmd - gmd).max():.3g}, {np.abs(wmd - gmd)[shallow].max():.3g} over the {int(shallow.sum())} states less than 0.1 m deep")
    assert len(gv) >= 2000 and band.mean() <= 0.01
    assert np.array_equal(wv[~band], gv[~band])


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the glued scene compile
# ---------------------------------------------------------------------------------------------------------------------------
def _hdr(ex, field):
    from mopa_rl_amd import _lib
    off = _lib.lib().mopa_scene_hdr_offset(field.encode())
    assert off >= 0, field
    return int(np.frombuffer(ex["hdr"].tobytes()[off:off + 4], dtype=np.int32)[0])


def _exports(O, env):
    from mopa_rl_amd import _lib
    c = G.glue_case(O, env)
    return c, _lib.k1_export(*c.scene_args()), _lib.k1_export(*c.scene_args(), glue=(c.a, c.b))


@pytest.mark.parametrize("env", ENVS)
def test_glued_compile_tables(env, oracle_mod):
    """body_b's subtree hangs in the arm's chains, the walk's save / load program hands every body its own parent's pose, nothing of
    the subtree is tile-posed, and no pruning proof is applied to a pair of the subtree."""
    c, u, g = _exports(oracle_mod, env)
    m = c.model
    I = g["ints"]
    nmb = _hdr(g, "nmb")
    tab = lambda name, n: I[_hdr(g, name):_hdr(g, name) + n]
    parent, load, save = tab("o_mb_parent", nmb), tab("o_mb_load", nmb), tab("o_mb_save", nmb)
    g_mb = tab("o_g_mb", len(m.geom_type))
    cadr, clen = tab("o_chain_adr", nmb), tab("o_chain_len", nmb)
    chain = lambda k: list(I[_hdr(g, "o_chain_items") + cadr[k]:][:clen[k]])
    sub = G.subtree_bodies(m, c.b)
    gb = np.asarray(m.geom_body)
    wrist = int(g_mb[[i for i in range(len(gb)) if m.body_names[gb[i]] == "right_l6"][0]])
    carried = [i for i in range(len(gb)) if sub[gb[i]]]
    assert carried
    for i in carried:
        ch = chain(int(g_mb[i]))
        assert ch[:len(chain(wrist))] == chain(wrist), "a carried geom's chain does not run through the arm"
        assert 0 < _hdr(g, "pfk_maxlen") and len(ch) <= _hdr(g, "pfk_maxlen")
    # the walk of the lane-per-state kernels: registers / save slots, emulated with body ids for poses
    slot, reg = {}, None
    for k in range(nmb):
        if load[k] == -1:
            assert reg == parent[k]
        elif load[k] >= 0:
            assert slot[int(load[k])] == parent[k], f"body {k} would be posed from body {slot[int(load[k])]}'s pose"
        else:
            assert parent[k] < 0
        reg = k
        if save[k] >= 0:
            slot[int(save[k])] = k
    assert max(int(s) for s in save) < _hdr(g, "n_save")
    # tile poses: the unglued Assembly scene poses the furniture once per tile; glued it moves with every state
    if env.startswith("SawyerAssembly"):
        assert _hdr(u, "n_pas_b") > 0
    assert _hdr(g, "n_pas_b") == 0
    # pruning: every candidate pair of the model with a carried geom is handed over, none with a tightened cull radius
    have = {(int(a), int(b)) for a, b in g["pair_geom"]}
    touching = [(int(a), int(b)) for a, b in np.asarray(m.pair_geom).reshape(-1, 2) if sub[gb[a]] or sub[gb[b]]]
    assert touching and all(p in have for p in touching)
    for (a, b), r in zip(g["pair_geom"], g["pair_cull_radius"]):
        if sub[gb[a]] or sub[gb[b]]:
            assert r == 0.0
    assert g["fingerprint"] != u["fingerprint"]


@pytest.mark.parametrize("env", ENVS)
def test_unglued_compile_is_the_recorded_one(env, oracle_mod, monkeypatch, capfd):
    """with the glue code in the compiler, and a glued compile made just before in the same process, the ordinary compile of the
    scene still equals the recorded one byte for byte (tests/golden/scene_build.json)"""
    import json
    from mopa_rl_amd import _lib
    from test_scene_build_host import GOLDEN, _args, _clear_knobs, _record
    _clear_knobs(monkeypatch.setenv, monkeypatch.delenv)
    c = G.glue_case(oracle_mod, env)
    _, args = _args(env)
    _lib.k1_export(*args, glue=(c.a, c.b))
    capfd.readouterr()
    got = _record(_lib.k1_export(*args), capfd.readouterr().err)
    with open(GOLDEN) as f:
        want = json.load(f)[env]["default"]
    assert got == want


def test_glue_refusals_are_status_codes():
    """Semantics item 5: body_b without exactly one free joint, body_a static, body_a >= body_b, body_a inside body_b's subtree --
    MOPA_ERR_UNSUPPORTED (2) with a message, from the host half of mopa_scene_create_glued"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    L = _lib.lib()

    def rc(env, a, b):
        pi = planner_inputs(env)
        m = pi.model
        name = lambda x: m.body_names.index(x) if isinstance(x, str) else x
        desc, keep, _, _ = _lib.scene_desc(m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
        sizes = np.zeros(8, dtype=np.int64)
        code = L.mopa_scene_k1_export_glued(C.byref(desc), name(a), name(b), sizes.ctypes.data_as(C.c_void_p), None, None, None, None, None)
        return code, L.mopa_last_error().decode()

    push, asm = "SawyerPushObstacle-v0", "SawyerAssemblyObstacle-v0"
    assert rc(push, "clawGripper", "cube")[0] == 0
    code, msg = rc(push, "clawGripper", "rightclaw")           # a slide joint
    assert code == 2 and "exactly one free joint" in msg
    code, msg = rc(push, "clawGripper", "table")               # no joint at all
    assert code == 2 and "exactly one free joint" in msg
    code, msg = rc(push, "table", "cube")
    assert code == 2 and "static" in msg
    code, msg = rc(push, "target", "cube")                     # a moving body behind the cube in body order
    assert code == 2 and "before body_b" in msg
    code, msg = rc(asm, "4_part4", "furniture")
    assert code == 2 and "subtree" in msg
    assert rc(asm, "furniture", "furniture")[0] == 2
    code, msg = rc(push, 0, "cube")
    assert code == 1 and "world" in msg
    assert rc(push, 10 ** 6, "cube")[0] == 1 and rc(push, -1, "cube")[0] == 1
    with pytest.raises(_lib.MopaError, match="no body named"):
        _lib.glue_ids(planner_inputs(push).model, "no_such_body", "cube")


# ---------------------------------------------------------------------------------------------------------------------------
# (c) PyKinematicPlanner / SamplingBasedPlanner
# ---------------------------------------------------------------------------------------------------------------------------
def _planner_args(glue, algo=b"rrt_connect"):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs("SawyerPushObstacle-v0")
    return (b"sawyer_push_obstacle.xml", algo, 7, b"", 0.0, pi.spec.range, list(pi.passive_joint_idx), glue,
            list(pi.ignored_contacts), pi.spec.contact_threshold, 0.05, False, 0.1, 3)


def _construct(make):
    """the planner, or None where no GPU is visible (the scene then refuses: the arguments were accepted)"""
    from mopa_rl_amd import _lib
    try:
        return make()
    except _lib.MopaError as e:
        assert "no HIP device" in str(e)
        return None


def test_planner_glue_bodies_arguments():
    from mopa_rl_amd.planner import PyKinematicPlanner
    for bad in (["cube"], ["clawGripper", "cube", "table"], [17, 48], ["clawGripper", 48]):
        with pytest.raises(NotImplementedError, match="two body names"):
            PyKinematicPlanner(*_planner_args(bad))
    with pytest.raises(NotImplementedError, match="glue_bodies with algo='rrt_star'"):
        PyKinematicPlanner(*_planner_args([b"clawGripper", b"cube"], algo=b"rrt_star"))
    for glue in ([b"clawGripper", b"cube"], ["clawGripper", "cube"], [b"clawGripper", "cube"]):
        p = _construct(lambda: PyKinematicPlanner(*_planner_args(glue)))       # no NotImplementedError any more
        if p is not None:
            assert p.glue_bodies == ["clawGripper", "cube"] and p._query_scene.glue == (17, 48) and p._scene.glue is None
    # the refused combinations name themselves (the check plan() runs first, here on a planner that owns no scene)
    p = PyKinematicPlanner.__new__(PyKinematicPlanner)
    p.glue_bodies, p.algo, p.portfolio, p.vertex_simplify, p.path_shortcut, p.path_smooth = ["clawGripper", "cube"], "rrt_connect", 1, False, False, False
    p._check_glue_combination()
    p.portfolio = 4
    with pytest.raises(NotImplementedError, match="glue_bodies with portfolio > 1"):
        p._check_glue_combination()
    p.portfolio = 1
    for flag in ("vertex_simplify", "path_shortcut", "path_smooth"):
        setattr(p, flag, True)
        with pytest.raises(NotImplementedError, match=f"glue_bodies with {flag}"):
            p._check_glue_combination()
        setattr(p, flag, False)
    p.algo = "rrt_star"
    with pytest.raises(NotImplementedError, match="rrt_star"):
        p._check_glue_combination()
    p.glue_bodies = []
    p._check_glue_combination()          # without glue nothing is refused here


def test_sampling_based_planner_passes_glue_bodies_through():
    from types import SimpleNamespace
    from mopa_rl_amd.sampling_based_planner import SamplingBasedPlanner
    a = _planner_args([])
    cfg = SimpleNamespace(planner_type="rrt_connect", range=a[5], planner_objective="", threshold=0.0, seed=3)
    kw = dict(passive_joint_idx=a[6], ignored_contacts=a[8], contact_threshold=a[9])
    with pytest.raises(NotImplementedError, match="two body names"):
        SamplingBasedPlanner(cfg, "sawyer_push_obstacle.xml", 7, None, glue_bodies=["cube"], **kw)
    sp = _construct(lambda: SamplingBasedPlanner(cfg, "sawyer_push_obstacle.xml", 7, None, glue_bodies=["clawGripper", "cube"], **kw))
    if sp is not None:
        assert sp.planner.glue_bodies == ["clawGripper", "cube"]
