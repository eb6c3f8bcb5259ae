"""K3b under the clearance objective on the GPU: k_rrt_star_clear (csrc/mopa_rrtstar_clear.inc) against the sequential reference
star_clearance_ref.py over the shared cases of star_clearance_cases.py -- status, path_len, path rows, clearance, length and all
eleven info columns on bit patterns, no tolerances -- then against the clearance report and path-length RRT* on the same inputs, slab
reuse, the launch variants, the synthetic cases, the refusals and the drop-in class."""
import ctypes as C
import math

import numpy as np
import pytest

import rrtstar_ref as R
import star_clearance_cases as CC
import star_clearance_ref as SR

pytestmark = pytest.mark.gpu

CASES = [(env, band) for env, (_, _, bands) in CC.SIZES.items() for band in bands]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(res):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def _assert_equal(got, want, what=""):
    """got: (path, plen, status, clearance, length[, info]) numpy; want: plan_star_clearance_batch's tuple"""
    assert np.array_equal(got[2], want[2]), f"{what}: status differs"
    assert np.array_equal(got[1], want[1]), f"{what}: path_len differs"
    for e in range(len(want[1])):
        n = int(want[1][e])
        assert np.array_equal(_bits(got[0][e, :n]), _bits(want[0][e, :n])), f"{what}: rows of query {e} differ"
    assert np.array_equal(_bits(got[3]), _bits(want[3])), f"{what}: clearance differs\n{got[3]}\n{want[3]}"
    assert np.array_equal(_bits(got[4]), _bits(want[4])), f"{what}: length differs\n{got[4]}\n{want[4]}"
    if len(got) > 5:
        assert np.array_equal(got[5], want[5]), f"{what}: info differs\n{got[5]}\n{want[5]}"


class Ctx:
    def __init__(self, O, env):
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        self.env = env
        self.pi, self.orc = CC.scene_of(O, env)
        pi = self.pi
        self.range = CC.range_of(pi, env)
        self.scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=self.range, seed=0, device=0)
        self.bp = BatchPlanner(self.scene)
        start, goal = CC.queries(O, env)
        self.start, self.goal = torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()
        self.prm = dict(max_iters=CC.SIZES[env][1], max_path=CC.MAX_PATH, seed=CC.SEED, **CC.PARAMS)


@pytest.fixture(scope="module")
def ctxs(oracle_mod):
    return {env: Ctx(oracle_mod, env) for env in CC.SIZES}


@pytest.fixture(scope="module")
def full(ctxs):
    """the plain launch of every case, made once: (env, band) -> numpy copies"""
    return {(env, band): _np(ctxs[env].bp.plan_star_clearance(ctxs[env].start, ctxs[env].goal, band, want_info=True, **ctxs[env].prm))
            for env, band in CASES}


@pytest.mark.parametrize("env,band", CASES)
def test_cases_equal_the_reference(oracle_mod, full, env, band):
    """fails on a library without mopa_plan_star_clearance_batch"""
    _assert_equal(full[env, band], CC.reference(oracle_mod, env, band)[:6], f"{env} at {band}")


@pytest.mark.parametrize("env,band", [(CC.PUSHER, 0.01), (CC.PUSHER, 0.05), (CC.PUSH, 0.01), (CC.LIFT, 0.01)])
def test_result_against_the_other_kernels(ctxs, full, env, band):
    """clearance = the clearance report's on the returned rows; node set = plan_star's; every returned segment passes check_motion"""
    import torch
    c = ctxs[env]
    path, plen, status, clearance, length, info = full[env, band]
    tp, tl = torch.from_numpy(path).cuda(), torch.from_numpy(plen).cuda()
    rep = c.bp.path_clearance(tp, tl, band)
    torch.cuda.synchronize()
    solved = status == 0
    assert solved.any()
    assert np.array_equal(_bits(rep.clearance.cpu().numpy()[solved]), _bits(clearance[solved]))
    assert (clearance[~solved] == -math.inf).all() and (length[~solved] == math.inf).all() and (plen[~solved] == 0).all()
    pl = _np(c.bp.plan_star(c.start, c.goal, want_info=True, **c.prm))
    assert np.array_equal(pl[2], status)
    for col in (1, 4, 5):
        assert np.array_equal(pl[4][:, col], info[:, col]), f"info column {col}"
    act = np.asarray(c.orc.active_idx)
    qa = np.concatenate([path[e, :plen[e] - 1][:, act] for e in np.nonzero(solved)[0]])
    qb = np.concatenate([path[e, 1:plen[e]][:, act] for e in np.nonzero(solved)[0]])
    rows = np.concatenate([np.repeat(path[e, :1], plen[e] - 1, axis=0) for e in np.nonzero(solved)[0]])
    ok = c.bp.check_motion(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (qa, qb, rows)), samples_per_env=1)
    torch.cuda.synchronize()
    assert bool(ok.cpu().numpy().all())


@pytest.fixture(scope="module")
def nine(oracle_mod, ctxs):
    """nine Pusher queries that end at -5, -4 and 0: the eight of the case set with one goal made invalid and one budget-starved
    start / goal pair (the last query repeats the first)"""
    import torch
    c = ctxs[CC.PUSHER]
    cases, _ = CC.synthetic(oracle_mod)
    start, goal = (np.concatenate([a, a[:1]]) for a in CC.queries(oracle_mod, CC.PUSHER))
    goal[2] = cases["invalid_goal"][1]
    start[5] = cases["invalid_start"][0]
    return torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()


def test_slab_reuse_with_one_workgroup(ctxs, nine):
    """E = 9 on one workgroup: every wave runs two or three queries on the same slab and LDS vectors, behind queries that ended at
    -5, -4 and 0; equal to the same queries run one by one"""
    c = ctxs[CC.PUSHER]
    start, goal = nine
    prm = dict(c.prm, max_iters=150)
    got = _np(c.bp.plan_star_clearance(start, goal, 0.01, want_info=True, max_workgroups=1, **prm))
    assert {-5, -4, 0} <= set(got[2].tolist())
    for e in range(9):
        one = _np(c.bp.plan_star_clearance(start[e:e + 1].contiguous(), goal[e:e + 1].contiguous(), 0.01, want_info=True, env_id_base=e, **prm))
        for x, y in zip(got, one):
            assert x[e].tobytes() == y[0].tobytes(), f"query {e}"


def test_launch_variants(ctxs, full):
    import torch
    c = ctxs[CC.PUSHER]
    ref = full[CC.PUSHER, 0.01]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device="cuda")
    sub = np.array([6, 2, 7, 0, 4])                          # reordered; no multiple of the four waves of a workgroup
    idx = t(sub)
    got = _np(c.bp.plan_star_clearance(c.start[idx].contiguous(), c.goal[idx].contiguous(), 0.01, env_id_base=555, env_ids=idx,
                                       seeds=t([CC.SEED] * len(sub)), want_info=True, **dict(c.prm, seed=999)))
    _assert_equal(got, [a[sub] for a in ref], "subset")
    again = _np(c.bp.plan_star_clearance(c.start, c.goal, 0.01, want_info=True, **c.prm))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r1 = c.bp.plan_star_clearance(c.start, c.goal, 0.01, want_info=True, stream=s1, **c.prm)
    r2 = c.bp.plan_star_clearance(c.start, c.goal, 0.01, want_info=True, stream=s2, **c.prm)
    for other in (again, _np(r1), _np(r2)):
        for x, y in zip(ref, other):
            assert x.tobytes() == y.tobytes()
    empty = c.bp.plan_star_clearance(c.start[:0].contiguous(), c.goal[:0].contiguous(), 0.01, want_info=True, **c.prm)
    assert [tuple(x.shape) for x in empty] == [(0, CC.MAX_PATH, c.scene.nq), (0,), (0,), (0,), (0,), (0, 11)]


def test_synthetic_cases(oracle_mod, ctxs):
    import torch
    c = ctxs[CC.PUSHER]
    cases, sid = CC.synthetic(oracle_mod)
    iters = CC.SIZES[CC.PUSHER][1]
    for name, (s, g, kw, want_status) in cases.items():
        kw = dict(dict(max_path=CC.MAX_PATH, max_nodes=None), **kw)
        want = SR.plan_star_clearance_batch(c.pi, c.orc, s[None], g[None], c.range, 0.01, iters, kw["max_nodes"], kw["max_path"], seed=CC.SEED,
                                            env_id_base=sid, **CC.PARAMS)
        got = _np(c.bp.plan_star_clearance(torch.from_numpy(s[None].copy()).cuda(), torch.from_numpy(g[None].copy()).cuda(), 0.01, max_iters=iters,
                                           seed=CC.SEED, env_id_base=sid, want_info=True, **CC.PARAMS, **kw))
        _assert_equal(got, want[:6], name)
        if want_status is not None:
            assert got[2][0] == want_status and got[1][0] == 0 and got[3][0] == -math.inf and got[4][0] == math.inf, name
    assert want is not None
    # the single-query host form gives the same, with full iterations counted
    s, g, kw, _ = cases["full_tree"]
    st, rows, clr, length, info = c.scene.plan_star_clearance(s, g, 0.01, iters, max_nodes=64, max_path=CC.MAX_PATH, seed=CC.SEED, env_id=sid, **CC.PARAMS)
    want = SR.plan_star_clearance(c.pi, c.orc, s, g, c.range, 0.01, iters, 64, CC.MAX_PATH, CC.SEED, sid, **CC.PARAMS)
    assert st == want.status and np.array_equal(_bits(rows), _bits(want.rows)) and np.array_equal(info, want.info)
    assert np.array_equal(_bits([clr, length]), _bits([want.clearance, want.length])) and info[7] >= 1


def test_c_level_refusals(ctxs):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    c = ctxs[CC.PUSHER]
    L = _lib.lib()
    E = 2
    path = torch.zeros(E, 8, c.scene.nq, dtype=torch.float64, device="cuda")
    plen = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    status = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    clr = torch.zeros(E, dtype=torch.float64, device="cuda")
    thr = c.pi.spec.contact_threshold
    assert thr < 0.0

    full_scene = c.scene.contact_scene()                         # the whole pair list: what BatchPlanner.plan_star_clearance runs on

    def call(scene=full_scene.handle, E=E, band=0.01, iters=10, nodes=11, mp=8, bias=0.05, gt=0.0, rf=1.1, p=_ptr(path), cl=_ptr(clr)):
        prm = _lib.MopaStarParams(iters, nodes, mp, 1, 0, None, None, bias, gt, rf, 0)
        return L.mopa_plan_star_clearance_batch(scene, _ptr(c.start), _ptr(c.goal), E, C.byref(prm), band, p, _ptr(plen), _ptr(status), cl, None, None, None)
    assert call(scene=None) == 1 and call(E=-1) == 1 and call(iters=-1) == 1 and call(nodes=1) == 1 and call(mp=1) == 1
    assert call(bias=1.5) == 1 and call(gt=-1.0) == 1 and call(rf=0.0) == 1 and call(p=None) == 1 and call(cl=None) == 1
    assert call(band=-0.001) == 1 and call(band=float("nan")) == 1 and call(band=float("inf")) == 1
    assert call(nodes=1 << 30) == 2                              # trees the scratch cannot hold
    assert call(rf=40.0, nodes=4096) == 2 and b"neighbours" in L.mopa_last_error()       # k(max_nodes) > 64
    if full_scene is not c.scene:                                # a scene created with pair_cull_radius is proven at its threshold only
        assert call(scene=c.scene.handle) == 2 and b"pair_cull_radius" in L.mopa_last_error()
    assert call(E=0) == 0
    torch.cuda.synchronize()
    assert (plen == 77).all() and (status == 77).all(), "a rejected call launched something"
    assert call(band=0.0) == 0
    torch.cuda.synchronize()
    assert set(status.cpu().tolist()) <= {0, -4}
    # band <= contact_threshold: thresholds above zero are not built and band >= 0, so the case is band 0 on a scene with threshold 0
    pi = c.pi
    loose = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, 0.0, range_=c.range, seed=0, device=0, prune_pairs=False)
    assert call(scene=loose.handle, band=0.0) == 1 and b"contact_threshold" in L.mopa_last_error()
    torch.cuda.synchronize()
    assert (plen[:E].cpu() >= 0).all()
    loose.close()


def test_glued_scene_is_refused(ctxs):
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    c = ctxs[CC.PUSH]
    glued = c.scene.glued("clawGripper", "cube")
    with pytest.raises(_lib.MopaError, match="glue"):
        BatchPlanner(glued).plan_star_clearance(c.start, c.goal, 0.01, **c.prm)


def test_drop_in_class(oracle_mod, ctxs):
    """PyKinematicPlanner with objective = "maximize_min_clearance": Scene.plan_star_clearance's rows, last_cost / last_length, the
    sentinels, and what is not built raises"""
    import types
    from mopa_rl_amd import _lib
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_PATH, PyKinematicPlanner
    from mopa_rl_amd.sampling_based_planner import SamplingBasedPlanner
    c = ctxs[CC.PUSHER]
    pi = c.pi
    start, goal = (a[0] for a in CC.queries(oracle_mod, CC.PUSHER))
    timelimit = 0.1
    iters = int(round(timelimit * ITERS_PER_SECOND))
    args = lambda algo, opt=b"path_length", glue=[]: (b"pusher_obstacle.xml", algo, 4, opt, 0.15, c.range, pi.passive_joint_idx, glue, pi.ignored_contacts,
                                                      pi.spec.contact_threshold, 0.5, False, 0.1, CC.SEED)
    with pytest.raises(NotImplementedError, match="path-length"):
        PyKinematicPlanner(*args(b"rrt_star", b"maximize_min_clearance"))
    pk = PyKinematicPlanner(*args(b"rrt_star"))
    assert pk.objective == "path_length" and pk.clearance_band is None
    pk.objective = "maximize_min_clearance"
    with pytest.raises(ValueError, match="clearance_band"):
        pk.plan(start, goal, timelimit)
    pk.clearance_band = 0.01
    for name in ("vertex_simplify", "path_shortcut", "path_smooth"):
        setattr(pk, name, True)
        with pytest.raises(NotImplementedError, match=name):
            pk.plan(start, goal, timelimit)
        setattr(pk, name, False)
    pk.objective = "min_clearance"
    with pytest.raises(ValueError, match="objective"):
        pk.plan(start, goal, timelimit)
    pk.objective = "maximize_min_clearance"
    assert pk._plan_count == 0
    st, want_rows, clr, length, _ = pk.scene.plan_star_clearance(start, goal, 0.01, iters, max_nodes=iters + 1, max_path=MAX_PATH, seed=CC.SEED,
                                                                 env_id=0, goal_bias=_lib.STAR_GOAL_BIAS, goal_threshold=0.15)
    want = SR.plan_star_clearance(pi, c.orc, start, goal, c.range, 0.01, iters, None, MAX_PATH, CC.SEED, 0, goal_threshold=0.15)
    assert st == 0 == want.status and np.array_equal(_bits(want_rows), _bits(want.rows))
    rows = np.array(pk.plan(start, goal, timelimit))
    assert np.array_equal(_bits(rows), _bits(want_rows)) and _bits([pk.last_cost, pk.last_length]).tolist() == _bits([clr, length]).tolist()
    assert pk.getPlannerStatus() == b"Exact solution"
    cases, _ = CC.synthetic(oracle_mod)
    assert pk.plan(start, cases["invalid_goal"][1], timelimit) == [[-5.0] * pk.scene.nq]
    assert pk.last_cost == -math.inf and pk.last_length == math.inf
    assert pk.plan(cases["invalid_start"][0], goal, timelimit) == [[-4.0] * pk.scene.nq]
    pk.close()
    rc = PyKinematicPlanner(*args(b"rrt_connect"))
    rc.objective, rc.clearance_band = "maximize_min_clearance", 0.01
    with pytest.raises(NotImplementedError, match="rrt_star"):
        rc.plan(start, goal, timelimit)
    rc.close()
    cfg = types.SimpleNamespace(planner_type="rrt_star", range=c.range, planner_objective="path_length", threshold=0.15, seed=CC.SEED)
    sbp = SamplingBasedPlanner(cfg, "pusher_obstacle.xml", 4, pi.non_limited_idx, passive_joint_idx=pi.passive_joint_idx, ignored_contacts=pi.ignored_contacts,
                               contact_threshold=pi.spec.contact_threshold, star_objective="maximize_min_clearance", clearance_band=0.01)
    assert sbp.planner.objective == "maximize_min_clearance" and sbp.planner.clearance_band == 0.01
    sbp.planner.close()


def test_glue_bodies_with_the_objective_raises():
    from mopa_rl_amd.planner import PyKinematicPlanner
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(CC.PUSH)
    pk = PyKinematicPlanner(b"sawyer_push_obstacle.xml", b"rrt_connect", 7, b"", 0.0, pi.spec.range, pi.passive_joint_idx, ["clawGripper", "cube"],
                            pi.ignored_contacts, pi.spec.contact_threshold, 0.05, False, 0.1, 0)
    pk.objective, pk.clearance_band = "maximize_min_clearance", 0.01
    with pytest.raises(NotImplementedError, match="glue"):
        pk.plan(np.zeros(pk.scene.nq), np.zeros(pk.scene.nq), 0.01)
    pk.close()
