"""K3b RRT* on the GPU: k_rrt_star (csrc/mopa_rrtstar.inc) against the sequential reference rrtstar_ref.py over the shared cases
of star_cases.py -- status, path_len, path rows, cost and all eight info columns on bit patterns, no tolerances -- the threshold /
bias variant, the synthetic cases, explicit ids / seeds, repeatability, the K9 switches behind the launch, and the drop-in classes."""
import numpy as np
import pytest

import rrtstar_ref as R
import star_cases as SC

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(res):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def _assert_equal(got, want, what=""):
    """got: (path, plen, status, cost[, info]) numpy; want: plan_star_batch's tuple"""
    assert np.array_equal(got[2], want[2]), f"{what}: status differs"
    assert np.array_equal(got[1], want[1]), f"{what}: path_len differs"
    for e in range(len(want[1])):
        n = int(want[1][e])
        assert np.array_equal(_bits(got[0][e, :n]), _bits(want[0][e, :n])), f"{what}: rows of query {e} differ"
    assert np.array_equal(_bits(got[3]), _bits(want[3])), f"{what}: cost differs"
    if len(got) > 4:
        assert np.array_equal(got[4], want[4]), f"{what}: info differs\n{got[4]}\n{want[4]}"


class Ctx:
    def __init__(self, O, env):
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        self.env = env
        self.pi, self.orc = SC.scene_of(O, env)
        pi = self.pi
        self.scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range,
                                seed=0, device=0)
        self.bp = BatchPlanner(self.scene)
        start, goal = SC.queries(O, env)
        self.start, self.goal = torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()
        self.prm = dict(max_iters=SC.MAX_ITERS, max_path=SC.MAX_PATH, seed=SC.SEED)


@pytest.fixture(scope="module")
def ctxs(oracle_mod):
    return {env: Ctx(oracle_mod, env) for env in (SC.PUSH, SC.PUSHER)}


@pytest.fixture(scope="module")
def full(ctxs):
    """the plain launch of both case sets, made once: (device tensors, numpy copies)"""
    out = {}
    for env, c in ctxs.items():
        res = c.bp.plan_star(c.start, c.goal, want_info=True, **c.prm)
        out[env] = (res, _np(res))
    return out


@pytest.mark.parametrize("env", [SC.PUSH, SC.PUSHER])
def test_cases_equal_the_reference(oracle_mod, full, env):
    """fails on a library without mopa_plan_star_batch"""
    _assert_equal(full[env][1], SC.reference(oracle_mod, env), env)


def test_threshold_and_bias_variant(oracle_mod, ctxs):
    c = ctxs[SC.PUSHER]
    got = _np(c.bp.plan_star(c.start, c.goal, want_info=True, **SC.VARIANT, **c.prm))
    want = SC.reference(oracle_mod, SC.PUSHER, variant=True)
    assert (want[4][:, 4] >= 2).any()
    _assert_equal(got, want, "threshold 0.15, bias 0.2")


def test_synthetic_cases(oracle_mod, ctxs):
    import torch
    c = ctxs[SC.PUSHER]
    cases, sid = SC.synthetic(oracle_mod)
    for name, (s, g, kw, want_status) in cases.items():
        kw = dict(dict(max_path=SC.MAX_PATH, max_nodes=None), **kw)
        want = R.plan_star_batch(c.orc, s[None], g[None], c.pi.spec.range, SC.MAX_ITERS, kw["max_nodes"], kw["max_path"], seed=SC.SEED,
                                 env_id_base=sid)
        got = _np(c.bp.plan_star(torch.from_numpy(s[None].copy()).cuda(), torch.from_numpy(g[None].copy()).cuda(), max_iters=SC.MAX_ITERS,
                                 seed=SC.SEED, env_id_base=sid, want_info=True, **kw))
        _assert_equal(got, want, name)
        if want_status is not None:
            assert got[2][0] == want_status, name
    # the single-query host form gives the same
    s, g, kw, _ = cases["full_tree"]
    st, rows, cost, info = c.scene.plan_star(s, g, SC.MAX_ITERS, max_nodes=64, max_path=SC.MAX_PATH, seed=SC.SEED, env_id=sid)
    want = R.plan_star(c.orc, s, g, c.pi.spec.range, SC.MAX_ITERS, 64, SC.MAX_PATH, SC.SEED, sid)
    assert st == want.status and np.array_equal(_bits(rows), _bits(want.rows)) and np.array_equal(info, want.info)
    assert np.array_equal(_bits([cost]), _bits([want.cost])) and info[7] >= 1


def test_compacted_subset_with_explicit_ids_and_seeds(ctxs, full):
    import torch
    c = ctxs[SC.PUSH]
    sub = np.array([13, 2, 10, 7, 4])                        # reordered; no multiple of the four waves of a workgroup
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device="cuda")
    idx = t(sub)
    prm = dict(c.prm, seed=999)
    got = _np(c.bp.plan_star(c.start[idx].contiguous(), c.goal[idx].contiguous(), env_id_base=555, env_ids=idx, seeds=t([SC.SEED] * len(sub)),
                             want_info=True, **prm))
    ref = full[SC.PUSH][1]
    _assert_equal(got, [a[sub] for a in ref], "subset")


def test_two_runs_give_identical_bytes(ctxs, full):
    import torch
    c = ctxs[SC.PUSHER]
    a = full[SC.PUSHER][1]
    b = _np(c.bp.plan_star(c.start, c.goal, want_info=True, max_workgroups=1, **c.prm))     # (and with one workgroup: each wave runs four queries)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_k9_switches_behind_the_launch(ctxs, full):
    """plan_star(vertex_simplify, path_shortcut) = plan_star followed by the K9 reference on its rows"""
    import shortcut_ref
    c = ctxs[SC.PUSH]
    path, plen, status, cost, info = full[SC.PUSH][1]
    assert ((status == 0) & (plen >= 3)).sum() >= 4
    want = shortcut_ref.shortcut_batch(c.orc, path, plen, status, seed=SC.SEED, passes=7)
    got = _np(c.bp.plan_star(c.start, c.goal, vertex_simplify=True, path_shortcut=True, **c.prm))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], status)
    for e in range(len(plen)):
        n = int(want[1][e])
        assert np.array_equal(_bits(got[0][e, :n]), _bits(want[0][e, :n])), f"rows of query {e} differ"
    assert np.array_equal(_bits(got[3]), _bits(cost)), "cost stays the planner's"
    assert any(want[1][e] != plen[e] or not np.array_equal(want[0][e, :plen[e]], path[e, :plen[e]]) for e in range(len(plen))), "K9 changed nothing"


def test_argument_errors_return_their_codes(ctxs):
    import ctypes as C
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    c = ctxs[SC.PUSHER]
    L = _lib.lib()
    assert L.mopa_star_params_size() == C.sizeof(_lib.MopaStarParams)
    E = 2
    path = torch.zeros(E, 8, c.scene.nq, dtype=torch.float64, device="cuda")
    plen = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    status = torch.full((E,), 77, dtype=torch.int32, device="cuda")

    def call(scene=c.scene.handle, E=E, iters=10, nodes=11, mp=8, bias=0.05, thr=0.0, rf=1.1, p=_ptr(path)):
        prm = _lib.MopaStarParams(iters, nodes, mp, 1, 0, None, None, bias, thr, rf, 0)
        return L.mopa_plan_star_batch(scene, _ptr(c.start), _ptr(c.goal), E, C.byref(prm), p, _ptr(plen), _ptr(status), None, None, None)
    assert call(scene=None) == 1 and call(E=-1) == 1 and call(iters=-1) == 1 and call(nodes=1) == 1 and call(mp=1) == 1
    assert call(bias=1.5) == 1 and call(thr=-1.0) == 1 and call(rf=0.0) == 1 and call(p=None) == 1
    assert call(nodes=1 << 30, rf=1.1) == 2                      # trees the scratch cannot hold
    assert call(rf=40.0, nodes=4096) == 2 and b"neighbours" in L.mopa_last_error()       # k(max_nodes) > 64
    assert call(E=0) == 0
    torch.cuda.synchronize()
    assert (plen == 77).all() and (status == 77).all(), "a rejected call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    assert set(status.cpu().tolist()) <= {0, -4}


def test_drop_in_classes_return_the_reference_path(oracle_mod, ctxs):
    """PyKinematicPlanner(algo=b"rrt_star") and SamplingBasedPlanner(planner_type="rrt_star"): the reference's path of the first
    Pusher query (stream (seed, 0) on the first call, goal bias 0.05 whatever the constructor is given); b"rrt" keeps raising"""
    import types
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_PATH, PyKinematicPlanner
    from mopa_rl_amd.sampling_based_planner import SamplingBasedPlanner
    c = ctxs[SC.PUSHER]
    pi = c.pi
    start, goal = (a[0] for a in SC.queries(oracle_mod, SC.PUSHER))
    timelimit = 0.1
    iters = int(round(timelimit * ITERS_PER_SECOND))
    want = R.plan_star(c.orc, start, goal, pi.spec.range, iters, None, MAX_PATH, SC.SEED, 0)
    assert want.status == 0 and len(want.rows) >= 2
    args = lambda algo: (b"pusher_obstacle.xml", algo, 4, b"path_length", 0.0, pi.spec.range, pi.passive_joint_idx, [], pi.ignored_contacts,
                         pi.spec.contact_threshold, 0.5, False, 0.1, SC.SEED)
    with pytest.raises(NotImplementedError, match="rrt_star"):
        PyKinematicPlanner(*args(b"rrt"))
    pk = PyKinematicPlanner(*args(b"rrt_star"))
    rows = np.array(pk.plan(start, goal, timelimit))
    assert np.array_equal(_bits(rows), _bits(want.rows)) and np.array_equal(_bits([pk.last_cost]), _bits([want.cost]))
    assert pk.getPlannerStatus() == b"Exact solution"
    second = R.plan_star(c.orc, start, goal, pi.spec.range, iters, None, MAX_PATH, SC.SEED, 1)           # a fresh stream per call
    assert np.array_equal(_bits(np.array(pk.plan(start, goal, timelimit))), _bits(second.rows))
    cfg = types.SimpleNamespace(planner_type="rrt_connect", range=pi.spec.range, planner_objective="path_length", threshold=0.0, seed=SC.SEED)
    sbp = SamplingBasedPlanner(cfg, "pusher_obstacle.xml", 4, pi.non_limited_idx, planner_type="rrt_star", passive_joint_idx=pi.passive_joint_idx,
                               ignored_contacts=pi.ignored_contacts, contact_threshold=pi.spec.contact_threshold)
    traj, states, valid, exact = sbp.plan(start, goal, timelimit)
    assert valid and exact and sbp.planner.algo == "rrt_star"
    q0, q1 = sbp.convert_nonlimited(start.copy()), sbp.convert_nonlimited(goal.copy())
    want_w = R.plan_star(c.orc, q0, q1, pi.spec.range, iters, None, MAX_PATH, SC.SEED, 0)
    assert np.array_equal(_bits(states), _bits(want_w.rows))
    assert np.array_equal(_bits(traj), _bits(np.add.accumulate(np.vstack([start[None], sbp._unwrapped_steps(want_w.rows)]), axis=0)))
