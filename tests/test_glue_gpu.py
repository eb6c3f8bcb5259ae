"""glue_bodies on the GPU: the glued scene (Scene.glued) against tests/glue_ref.py -- the CPU oracle run on the model re-parented with
each env row's offset.  Every comparison is on uint64 views.  Inputs: tests/glue_ref.py GlueCase (a different object pose in every
env, a non-unit free-joint quaternion in env 0; Push with only the cube-gripper pairs ignored, Lift / Assembly with the object-gripper
pairs added to their defaults)."""
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

pytestmark = pytest.mark.gpu
ENVS = list(G.GLUE_CASES)
_SCENES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scenes(O, env, kernel=None):
    """(case, unglued Scene, its glued sibling); kernel: MOPA_VALID_KERNEL pinned while the scenes are created (read once, there)"""
    from mopa_rl_amd import _lib
    key = (env, kernel)
    if key not in _SCENES:
        c = G.glue_case(O, env)
        old = os.environ.get("MOPA_VALID_KERNEL")
        if kernel is not None:
            os.environ["MOPA_VALID_KERNEL"] = kernel
        try:
            sc = _lib.Scene(*c.scene_args(), range_=c.pi.spec.range, seed=7)
            gl = sc.glued(c.a, c.b)
        finally:
            if kernel is not None:
                if old is None:
                    os.environ.pop("MOPA_VALID_KERNEL", None)
                else:
                    os.environ["MOPA_VALID_KERNEL"] = old
        _SCENES[key] = (c, sc, gl)
    return _SCENES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for _, sc, _ in _SCENES.values():
        sc.close()
    _SCENES.clear()


@pytest.mark.parametrize("env", ENVS)
def test_attach_rows(env, oracle_mod):
    """mopa_glue_attach_batch against the reference's (t, rq): E = 64 rows, everything else of a row copied"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    c, sc, gl = _scenes(oracle_mod, env)
    assert gl.glue == (c.a, c.b) and sc.glue is None
    ids = np.zeros(2, dtype=np.int32)
    from mopa_rl_amd import _lib
    _lib.check(_lib.lib().mopa_scene_glue(gl.handle, ids.ctypes.data_as(C.POINTER(C.c_int32))))
    assert tuple(ids) == (c.a, c.b)
    _lib.check(_lib.lib().mopa_scene_glue(sc.handle, ids.ctypes.data_as(C.POINTER(C.c_int32))))
    assert tuple(ids) == (-1, -1)
    got = BatchPlanner(gl).glue_attach(torch.from_numpy(c.rows).cuda()).cpu().numpy()
    want = np.array([G.attached_row(c.orc, c.a, c.b, r) for r in c.rows])
    assert not np.array_equal(want[:, c.adr:c.adr + 7], c.rows[:, c.adr:c.adr + 7])
    assert np.array_equal(_bits(got), _bits(want))
    # mopa_debug_fk attaches the state itself: every geom, the carried ones included, lies where the ordinary scene poses it, up to
    # the rounding of one rotation there and back (coordinates of about 1 m: 1e-12 is four orders above an ulp)
    for r in c.rows[:2]:
        (gp, gm), (up, um) = gl.debug_fk(r), sc.debug_fk(r)
        assert np.abs(gp - up).max() < 1e-12 and np.abs(gm - um).max() < 1e-12


@pytest.mark.parametrize("kernel", [None, "v2"])
@pytest.mark.parametrize("env", ENVS)
def test_is_valid(env, kernel, oracle_mod):
    """verdicts and min_dist of the glued scene, with and without min_dist: 64 states (one wave per state) and 64 x 256 states (one
    lane per state: the third-generation kernel, and the second with MOPA_VALID_KERNEL=v2)"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    c, sc, gl = _scenes(oracle_mod, env, kernel)
    uv, gv, gmd = c.validity()
    assert (uv != gv).sum() >= 32
    bp = BatchPlanner(gl)
    rows = torch.from_numpy(c.rows).cuda()
    # small batch: 64 states of several envs, each with its own env row
    idx = c.small_batch(64)
    assert (uv[idx] != gv[idx]).sum() >= 32
    if kernel is None:
        assert gl.valid_kernel(64) == "k_is_valid" and gl.valid_kernel(c.E * c.S) == "k_is_valid_v5"
    else:
        assert gl.valid_kernel(c.E * c.S) == "k_is_valid_v2"
    qs, rs = torch.from_numpy(c.qa[idx]).cuda(), rows[torch.from_numpy(idx // c.S).cuda()].contiguous()
    v, md = bp.is_valid(qs, rs, samples_per_env=1, want_min_dist=True)
    v2 = bp.is_valid(qs, rs, samples_per_env=1)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), gv[idx]) and np.array_equal(v2.cpu().numpy(), gv[idx])
    assert np.array_equal(_bits(md.cpu().numpy()), _bits(gmd[idx]))
    # large batch
    qa = torch.from_numpy(c.qa).cuda()
    v, md = bp.is_valid(qa, rows, samples_per_env=c.S, want_min_dist=True)
    v2 = bp.is_valid(qa, rows, samples_per_env=c.S)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), gv) and np.array_equal(v2.cpu().numpy(), gv)
    assert np.array_equal(_bits(md.cpu().numpy()), _bits(gmd))
    # the unglued scene created next to it still equals the unglued oracle
    uvd = BatchPlanner(sc).is_valid(qa, rows, samples_per_env=c.S)
    torch.cuda.synchronize()
    assert np.array_equal(uvd.cpu().numpy(), uv)


@pytest.mark.parametrize("cap", [100000, 64, 0])
def test_lift_mesh_row_list(cap, oracle_mod, monkeypatch):
    """Lift's carried can is a mesh: the gate's row list on, overflowing and off (as test_lift_mesh_row_list_and_its_overflow)"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    monkeypatch.setenv("MOPA_MESH_ROWS_CAP", str(cap))          # (read per call)
    c, sc, gl = _scenes(oracle_mod, "SawyerLiftObstacle-v0")
    _, gv, gmd = c.validity()
    bp = BatchPlanner(gl)
    qa, rows = torch.from_numpy(c.qa).cuda(), torch.from_numpy(c.rows).cuda()
    for _ in range(2):
        v, md = bp.is_valid(qa, rows, samples_per_env=c.S, want_min_dist=True)
        v2 = bp.is_valid(qa, rows, samples_per_env=c.S)
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy(), gv) and np.array_equal(v2.cpu().numpy(), gv)
        assert np.array_equal(_bits(md.cpu().numpy()), _bits(gmd))


@pytest.mark.parametrize("env", ENVS)
def test_check_motion(env, oracle_mod):
    """64 segments (one wave each) and 8192 segments (expanded into their states for the lane-per-state kernel)"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    c, sc, gl = _scenes(oracle_mod, env)
    bp = BatchPlanner(gl)
    per = 128
    rng = np.random.default_rng(8)
    qa = c.qa.reshape(c.E, c.S, -1)[:, :per].reshape(c.E * per, -1)
    qb = np.clip(qa + rng.uniform(-0.12, 0.12, qa.shape), c.pi.jnt_minimum, c.pi.jnt_maximum)
    want = np.concatenate([c.ref(e).orc.check_motion_batch(qa[e * per:(e + 1) * per], qb[e * per:(e + 1) * per], c.rows[e:e + 1], samples_per_env=per,
                                                           nthreads=0) for e in range(c.E)])
    unglued = c.orc.check_motion_batch(qa, qb, c.rows, samples_per_env=per, nthreads=0)
    assert 0.05 < want.mean() < 0.95 and (want != unglued).sum() >= 8
    rows = torch.from_numpy(c.rows).cuda()
    assert gl.motion_kernel(c.E) == "k_check_motion" and gl.motion_kernel(c.E * per) == "k_motion_expand"
    got = bp.check_motion(torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), rows, samples_per_env=per)
    first = np.arange(c.E) * per
    got1 = bp.check_motion(torch.from_numpy(qa[first]).cuda(), torch.from_numpy(qb[first]).cuda(), rows, samples_per_env=1)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got1.cpu().numpy(), want[first])


BUILDS = (("default", None, None, {}), ("w1", "w1", None, {}), ("w2", "w2", None, {"max_workgroups": -1}), ("wg", "wg", None, {}),
          ("wg_small_mirror", "wg", "64", {}))


@pytest.mark.parametrize("env", ENVS)
def test_plan(env, oracle_mod, monkeypatch):
    """16 queries under every K3 build `plan` can select (as test_planner_builds_agree selects them): status, path length, consumed
    checks and the path rows -- the free-joint columns = the carried body's pose at the waypoint -- equal the reference's"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    c, sc, gl = _scenes(oracle_mod, env)
    starts, goals, res = G.plan_case(oracle_mod, env)
    bp = BatchPlanner(gl)
    s, g = torch.from_numpy(starts).cuda(), torch.from_numpy(goals).cuda()
    for name, build, cap, kw in BUILDS:
        if build is None:
            monkeypatch.delenv("MOPA_PLAN_BUILD", raising=False)
        else:
            monkeypatch.setenv("MOPA_PLAN_BUILD", build)
        if cap is None:
            monkeypatch.delenv("MOPA_PLAN_NN_CAP", raising=False)
        else:
            monkeypatch.setenv("MOPA_PLAN_NN_CAP", cap)
        path, plen, status, chk = [t.cpu().numpy() for t in bp.plan(s, g, **G.PLAN_PARAMS, **kw)]
        for k, (st, rows, nchk, _) in enumerate(res):
            assert status[k] == st and plen[k] == len(rows) and chk[k] == nchk, (name, k)
            assert np.array_equal(_bits(path[k, :len(rows)]), _bits(rows)), (name, k)
    with pytest.raises(Exception, match="glued scene"):
        bp.plan(s, g, **G.PLAN_PARAMS, keep_state=True)


def test_glue_rows_alone(oracle_mod):
    """mopa_glue_rows_batch on rows of its own: path_len 0, 1 and max_path; rows at and past path_len and every other column stay"""
    import torch
    from mopa_rl_amd.batch import BatchPlanner
    env = "SawyerAssemblyObstacle-v0"
    c, sc, gl = _scenes(oracle_mod, env)
    bp = BatchPlanner(gl)
    max_path = 37
    lens = np.array([0, 1, max_path, 5], dtype=np.int32)
    E = len(lens)
    rng = np.random.default_rng(12)
    path = rng.normal(size=(E, max_path, c.model.nq))
    for e in range(E):
        path[e][:, c.act] = rng.uniform(c.pi.jnt_minimum, c.pi.jnt_maximum, (max_path, len(c.act)))
    att = bp.glue_attach(torch.from_numpy(c.rows[:E]).cuda())
    got = bp.glue_rows(torch.from_numpy(path).cuda(), torch.from_numpy(lens).cuda(), att).cpu().numpy()
    want = path.copy()
    for e in range(E):
        for r in range(lens[e]):
            full = c.rows[e].copy()
            full[c.act] = path[e, r, c.act]
            want[e, r, c.adr:c.adr + 7] = c.ref(e).pose_columns(full)[c.adr:c.adr + 7]
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got[2]), _bits(path[2]))


def test_drop_in_planner_and_refusals(oracle_mod):
    """PyKinematicPlanner(glue_bodies=[...]): isValidState attaches the state itself, plan the start state; both equal the reference.
    The entry points that are not built for a glued scene return MOPA_ERR_UNSUPPORTED on it."""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_NODES, MAX_PATH, PyKinematicPlanner
    O = oracle_mod
    env = "SawyerPushObstacle-v0"
    c = G.glue_case(O, env)
    pk = PyKinematicPlanner(b"sawyer_push_obstacle.xml", b"rrt_connect", 7, b"", 0.0, c.pi.spec.range, c.passive, [b"clawGripper", b"cube"], c.ignored,
                            c.thr, 0.05, False, 0.1, 11)
    # isValidState: the state is its own attach row
    for i in list(c.small_batch(12)):
        e = int(i) // c.S
        s = c.rows[e].copy()
        s[c.act] = c.qa[i]
        ref = G.GluedRef(O, c.orc, c.a, c.b, s, c.passive, c.ignored, c.thr)
        assert pk.isValidState(s) == ref.orc.is_valid(s)[0]
    # plan: a solved query, then one whose goal the carried cube makes invalid
    starts, goals, res = G.plan_case(O, env)
    timelimit = 0.15
    for count, k in enumerate((1, 8)):
        e = G.PLAN_QUERIES[env][k][0]
        st, rows, _ = c.ref(e).plan(starts[k], goals[k], c.pi.spec.range, 0.005, max_iters=int(round(timelimit * ITERS_PER_SECOND)), max_nodes=MAX_NODES,
                                    seed=11, env_id=count, max_path=MAX_PATH)
        got = np.array(pk.plan(starts[k], goals[k], timelimit))
        if k == 8:
            assert st == -5 and np.array_equal(got, np.full((1, c.model.nq), -5.0))
        else:
            assert st == 0 and len(rows) >= 3 and np.array_equal(_bits(got), _bits(rows))
            assert not np.array_equal(got[-1, c.adr:c.adr + 3], got[0, c.adr:c.adr + 3])        # the cube travels with the gripper
    # the combinations that are not built
    pk.portfolio = 2
    with pytest.raises(NotImplementedError, match="portfolio"):
        pk.plan(starts[1], goals[1], timelimit)
    pk.portfolio, pk.path_shortcut = 1, True
    with pytest.raises(NotImplementedError, match="path_shortcut"):
        pk.plan(starts[1], goals[1], timelimit)
    # an unglued planner of the same process still equals the unglued oracle
    pu = PyKinematicPlanner(b"sawyer_push_obstacle.xml", b"rrt_connect", 7, b"", 0.0, c.pi.spec.range, c.passive, [], c.ignored, c.thr, 0.05, False, 0.1, 11)
    ost, opath, _, _ = c.orc.plan(starts[1], goals[1], c.pi.spec.range, 0.005, max_iters=int(round(timelimit * ITERS_PER_SECOND)), max_nodes=MAX_NODES, seed=11,
                                  env_id=0, max_path=MAX_PATH)
    assert ost == 0 and np.array_equal(_bits(np.array(pu.plan(starts[1], goals[1], timelimit))), _bits(opath))
    # refusals on the glued scene: MOPA_ERR_UNSUPPORTED (2), nothing runs
    gl = pk._query_scene
    L = _lib.lib()
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(d.data_ptr())
    h = gl.handle
    star = _lib.MopaStarParams(10, 16, 8, 0, 0, None, None, 0.05, 0.0, 1.1, 0)
    race = _lib.MopaRaceParams(10, 16, 8, 2, 0, 0, None, None, 0, 0)
    calls = {
        "plan_star": lambda: L.mopa_plan_star_batch(h, p, p, 1, C.byref(star), p, p, p, p, p, None),
        "plan_race": lambda: L.mopa_plan_race_batch(h, p, p, 1, C.byref(race), p, p, p, p, p, p, p, None),
        "simplify": lambda: L.mopa_simplify_paths_batch(h, 1, 8, p, p, None, 0, 0, None, None, 3, None, None),
        "shortcut": lambda: L.mopa_shortcut_paths_batch(h, 1, 8, p, p, None, 0, 0, None, None, 7, 4, None, None),
        "smooth": lambda: L.mopa_smooth_paths_batch(h, 1, 8, p, p, None, 0, 0, None, None, 15, 4, None, None),
        "pullback": lambda: L.mopa_pullback_batch(h, p, p, 1, 0.1, 2, p, p, None),
        "contacts": lambda: L.mopa_contacts_batch(h, p, p, 1, 1, -0.002, 4, p, p, p, None),
        "interpolate": lambda: L.mopa_interpolate_batch(h, 1, 7, 4, p, p, 0.05, p, p, p, p, None),
    }
    for name, call in calls.items():
        assert call() == 2, name
        assert "glued scene" in L.mopa_last_error().decode(), name
    for single in (lambda: gl.plan_star(starts[1], goals[1], max_iters=10), lambda: gl.plan_race(starts[1], goals[1], 2, max_iters=10),
                   lambda: gl.contacts_state_raw(starts[1])):
        with pytest.raises(_lib.MopaError, match="error 2"):
            single()
    # the drop-in class's extras: `scene` is the glued scene, the contact report refuses
    assert pk.scene is gl and gl.glue == (c.a, c.b) and pu.scene.glue is None
    with pytest.raises(NotImplementedError, match="contacts"):
        pk.contacts(starts[1])
    torch.cuda.synchronize()
    pk.close()
    pu.close()
