"""K9 on the GPU: k_simplify_paths (csrc/mopa_k9.inc) against the sequential reference simplify_ref.py -- surviving rows on
bit patterns, lengths, motion-check and draw counts -- over the device planner's own paths of the blocked Push / Pusher queries
of test_simplify_host.py and over synthetic paths; skipped paths, launch shapes, ids / seeds, continuation, streams, argument
errors, and the flag through SamplingBasedPlanner and the rollout."""
import numpy as np
import pytest

import simplify_ref as R
from simplify_cases import (MAX_NODES, MAX_PATH, PLAN_SEED, QUERY_SETS, blocked_queries, push_out_and_back, pusher_wrap_path, scene_of)

pytestmark = pytest.mark.gpu

PUSH, PUSHER = "SawyerPushObstacle-v0", "PusherObstacle-v0"
NAN_BITS = 0x7FF8DEADBEEF0001          # a quiet NaN with a payload: what never-written rows hold


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_rows(got_path, got_len, want_path, want_len, what=""):
    assert np.array_equal(got_len, want_len), f"{what}: path_len differs"
    for e in range(len(want_len)):
        n = int(want_len[e])
        assert np.array_equal(_bits(got_path[e, :n]), _bits(want_path[e, :n])), f"{what}: rows of path {e} differ"


class Ctx:
    """per env: scene, the device planner's paths of the blocked queries (never modified) and their reference simplification"""

    def __init__(self, O, env):
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        self.env = env
        self.pi, self.orc = scene_of(O, env)
        pi = self.pi
        self.scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range,
                                seed=0, device=0)
        self.bp = BatchPlanner(self.scene)
        start, goal = blocked_queries(pi, self.orc, env)
        self.start, self.goal = torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()
        self.prm = dict(max_iters=QUERY_SETS[env][2], max_nodes=MAX_NODES, max_path=MAX_PATH, seed=PLAN_SEED)
        res = self.bp.plan(self.start, self.goal, **self.prm)
        torch.cuda.synchronize()
        self.planned = res                                   # device tensors: clone before simplifying
        self.path, self.plen, self.status, self.nchk = (t.cpu().numpy() for t in res)
        self.ref = R.simplify_batch(self.orc, self.path, self.plen, self.status, seed=PLAN_SEED)

    def clones(self):
        return [t.clone() for t in self.planned]


@pytest.fixture(scope="module")
def ctxs(oracle_mod):
    return {env: Ctx(oracle_mod, env) for env in (PUSH, PUSHER)}


def _filled(E, max_path, nq):
    import torch
    path = torch.empty(E, max_path, nq, dtype=torch.float64, device="cuda")
    path.view(torch.int64).fill_(NAN_BITS)
    return path


@pytest.mark.parametrize("env", [PUSH, PUSHER])
def test_planned_paths_equal_the_reference(ctxs, env):
    """fails on a library without mopa_simplify_paths_batch"""
    import torch
    c = ctxs[env]
    want_path, want_len, want_info, events = c.ref
    solved = np.where(c.status == 0)[0]
    shortened = [e for e in solved if events[e]["splice"] >= 1 and want_len[e] < c.plen[e]]
    assert len(shortened) >= (8 if env == PUSH else 3), "the device planner's paths do not exercise reduceVertices"
    assert sum(events[e]["collapse_block"] for e in solved) >= 1
    path, plen, status, nchk = c.clones()
    info = c.bp.simplify_paths(path, plen, status, seed=PLAN_SEED, want_info=True)
    torch.cuda.synchronize()
    _assert_rows(path.cpu().numpy(), plen.cpu().numpy(), want_path, want_len, "two-step form")
    assert np.array_equal(info.cpu().numpy(), want_info), "motion-check / draw counts differ"
    assert np.array_equal(status.cpu().numpy(), c.status)
    # the flag on plan(): the same, and n_checks stays the planner's own count
    one = c.bp.plan(c.start, c.goal, vertex_simplify=True, **c.prm)
    torch.cuda.synchronize()
    _assert_rows(one[0].cpu().numpy(), one[1].cpu().numpy(), want_path, want_len, "plan(vertex_simplify=True)")
    assert np.array_equal(one[2].cpu().numpy(), c.status) and np.array_equal(one[3].cpu().numpy(), c.nchk)
    # flag off: what the planner gave before
    off = c.bp.plan(c.start, c.goal, vertex_simplify=False, **c.prm)
    _assert_rows(off[0].cpu().numpy(), off[1].cpu().numpy(), c.path, c.plen, "plan()")


def _synthetic(c):
    """(path [3, 16, nq], plen) of free-space paths for the env of c"""
    if c.env == PUSH:
        rows = push_out_and_back(c.pi, c.orc)
        cases = [rows, rows[:len(rows) // 2], rows[::-1].copy()]
    else:
        rows = pusher_wrap_path(c.pi, c.orc)
        cases = [rows, rows[::-1].copy(), rows[:3]]
    path = np.zeros((len(cases), 16, c.orc.nq))
    plen = np.array([len(r) for r in cases], dtype=np.int32)
    for k, r in enumerate(cases):
        path[k, :len(r)] = r
    return path, plen


@pytest.mark.parametrize("env", [PUSH, PUSHER])
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_each_routine_alone_on_synthetic_paths(ctxs, env, passes):
    import torch
    c = ctxs[env]
    path, plen = _synthetic(c)
    want = R.simplify_batch(c.orc, path, plen, None, seed=5, env_id_base=3, passes=passes)
    ev = want[3]
    if passes == 2:
        assert sum(e["collapse_removal"] for e in ev) >= 1 and not want[2][:, 1].any(), "collapse alone: removals, no draws"
    if passes == 1:
        assert all(e["collapse_removal"] == e["collapse_block"] == 0 for e in ev) and sum(e["first_check"] + e["splice"] for e in ev) >= 1
    p, n = torch.from_numpy(path).cuda(), torch.from_numpy(plen).cuda()
    info = c.bp.simplify_paths(p, n, None, seed=5, env_id_base=3, passes=passes, want_info=True)
    torch.cuda.synchronize()
    _assert_rows(p.cpu().numpy(), n.cpu().numpy(), want[0], want[1], f"passes={passes}")
    assert np.array_equal(info.cpu().numpy(), want[2])


def test_skipped_paths_are_not_touched(ctxs):
    import torch
    c = ctxs[PUSH]
    e0 = int(np.where(c.status == 0)[0][0])
    L = int(c.plen[e0])
    status = np.array([0, -4, -5, 0, 0, 0, 0], dtype=np.int32)
    plen = np.array([L, L, L, 0, 1, 2, L], dtype=np.int32)
    E = len(plen)
    base = _filled(E, L + 3, c.orc.nq)
    for e in range(E):
        base[e, :L] = c.planned[0][e0, :L]
    before = base.cpu().numpy()
    for st in (status, None):
        path, n = base.clone(), torch.from_numpy(plen).cuda()
        st_t = torch.from_numpy(st).cuda() if st is not None else None
        info = c.bp.simplify_paths(path, n, st_t, seed=PLAN_SEED, env_id_base=e0, want_info=True)
        torch.cuda.synchronize()
        got, got_n, got_info = path.cpu().numpy(), n.cpu().numpy(), info.cpu().numpy()
        want = R.simplify_batch(c.orc, before, plen, st, seed=PLAN_SEED, env_id_base=e0)
        skipped = [e for e in range(E) if plen[e] < 3 or (st is not None and st[e] != 0)]
        assert skipped == ([1, 2, 3, 4, 5] if st is not None else [3, 4, 5])
        for e in skipped:
            assert np.array_equal(_bits(got[e]), _bits(before[e])), f"bytes of skipped path {e} changed"
            assert got_n[e] == plen[e] and not got_info[e].any()
        _assert_rows(got, got_n, want[0], want[1], "status given" if st is not None else "null status")
        assert np.array_equal(got_info, want[2])
        assert got_n[0] == c.ref[1][e0] and got_n[0] < L       # row 0 is query e0 with its own stream id


@pytest.mark.parametrize("E", [1, 5, 67])
def test_partial_workgroups_and_full_length_paths(ctxs, E):
    """E no multiple of the four waves of a workgroup; max_path = the longest path, which therefore fills its buffer"""
    import torch
    c = ctxs[PUSH]
    solved = np.where(c.status == 0)[0]
    src = solved[np.argsort(-c.plen[solved], kind="stable")][np.arange(E) % len(solved)]       # path 0: the longest
    mp = int(c.plen[src[0]])
    path = _filled(E, mp, c.orc.nq)
    for k, e in enumerate(src):
        path[k, :int(c.plen[e])] = c.planned[0][e, :int(c.plen[e])]
    plen = torch.from_numpy(c.plen[src].copy()).cuda()
    assert int(plen[0]) == mp
    want = R.simplify_batch(c.orc, path.cpu().numpy(), c.plen[src], None, seed=21, env_id_base=100)
    info = c.bp.simplify_paths(path, plen, None, seed=21, env_id_base=100, want_info=True)
    torch.cuda.synchronize()
    _assert_rows(path.cpu().numpy(), plen.cpu().numpy(), want[0], want[1], f"E={E}")
    assert np.array_equal(info.cpu().numpy(), want[2])
    if E > len(solved):      # the same rows under another stream id: other draws
        assert any(not np.array_equal(want[2][k], want[2][k + len(solved)]) for k in range(E - len(solved)))


def test_compacted_subset_with_explicit_ids_and_seeds(ctxs):
    import torch
    c = ctxs[PUSH]
    solved = np.where(c.status == 0)[0]
    sub = np.concatenate([solved[::-2], np.where(c.status != 0)[0][:2]])      # reordered, with two unsolved queries
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
    idx = t(sub, torch.int64)
    path, plen, status = c.planned[0][idx].contiguous(), c.planned[1][idx].contiguous(), c.planned[2][idx].contiguous()
    c.bp.simplify_paths(path, plen, status, seed=999, env_id_base=555, env_ids=idx, seeds=t([PLAN_SEED] * len(sub), torch.int64))
    torch.cuda.synchronize()
    _assert_rows(path.cpu().numpy(), plen.cpu().numpy(), c.ref[0][sub], c.ref[1][sub], "subset")


def test_continuation_simplifies_every_query_once(ctxs):
    import torch
    c = ctxs[PUSH]
    prm = dict(c.prm)
    full_iters = prm.pop("max_iters")
    p1 = c.bp.plan(c.start, c.goal, max_iters=30, keep_state=True, vertex_simplify=True, **prm)
    p2 = c.bp.plan(c.start, c.goal, max_iters=full_iters, resume=p1[4], vertex_simplify=True, **prm)
    torch.cuda.synchronize()
    n1, n2 = p1[1].cpu().numpy(), p2[1].cpu().numpy()
    assert (n1 > 0).sum() >= 2 and (n2 > 0).sum() >= 2 and not ((n1 > 0) & (n2 > 0)).any(), "both launches must solve some queries"
    late = torch.from_numpy(n2 > 0).cuda()
    path = torch.where(late[:, None, None], p2[0], p1[0]).cpu().numpy()
    plen = np.where(n2 > 0, n2, n1)
    _assert_rows(path, plen, c.ref[0], c.ref[1], "first launch + continuation")
    assert np.array_equal(plen > 0, c.status == 0)


def test_side_stream_launch_does_not_synchronise(ctxs):
    import torch
    c = ctxs[PUSHER]
    s = torch.cuda.Stream()
    path, plen, status, _ = c.clones()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(s):
            info = c.bp.simplify_paths(path, plen, status, seed=PLAN_SEED, stream=s, want_info=True)
            one = c.bp.plan(c.start, c.goal, stream=s, vertex_simplify=True, **c.prm)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for got in ((path, plen), (one[0], one[1])):
        _assert_rows(got[0].cpu().numpy(), got[1].cpu().numpy(), c.ref[0], c.ref[1], "side stream")
    assert np.array_equal(info.cpu().numpy(), c.ref[2])


def test_argument_errors_return_their_codes(ctxs):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    c = ctxs[PUSH]
    L = _lib.lib()
    cap = L.mopa_simplify_paths_max_path(c.scene.handle)
    assert 512 <= cap <= 65535
    path, plen, status, _ = c.clones()
    before = (path.clone(), plen.clone())
    h, E = c.scene.handle, path.shape[0]
    call = lambda scene=h, E=E, mp=MAX_PATH, p=_ptr(path), n=_ptr(plen), passes=3: L.mopa_simplify_paths_batch(
        scene, E, mp, p, n, _ptr(status), PLAN_SEED, 0, None, None, passes, None, None)
    assert call(scene=None) == 1 and call(E=-1) == 1 and call(mp=1) == 1 and call(passes=0) == 1 and call(passes=4) == 1
    assert call(p=None) == 1 and call(n=None) == 1
    assert call(mp=cap + 1) == 2 and b"max_path" in L.mopa_last_error()           # MOPA_ERR_UNSUPPORTED
    assert call(E=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(path, before[0]) and torch.equal(plen, before[1]), "a rejected call launched something"
    with pytest.raises(_lib.MopaError):
        c.bp.simplify_paths(path, plen.to(torch.int64), status)
    with pytest.raises(_lib.MopaError):
        c.bp.simplify_paths(path, plen, status, passes=0)


def test_sampling_based_planner_returns_the_unwrapped_reference_rows(ctxs):
    """the flag through the drop-in classes: `states` are the reference's survivors of the single-query plan, `traj` their
    un-wrapped form; is_simplified keeps raising"""
    import types
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_NODES as NODES, MAX_PATH as PATH
    from mopa_rl_amd.sampling_based_planner import SamplingBasedPlanner
    c = ctxs[PUSHER]
    pi = c.pi
    cfg = types.SimpleNamespace(planner_type="rrt_connect", range=pi.spec.range, planner_objective="path_length", threshold=0.0, seed=PLAN_SEED)
    mk = lambda **kw: SamplingBasedPlanner(cfg, "pusher_obstacle.xml", 4, pi.non_limited_idx, passive_joint_idx=pi.passive_joint_idx,
                                           ignored_contacts=pi.ignored_contacts, contact_threshold=pi.spec.contact_threshold, **kw)
    with pytest.raises(NotImplementedError, match="vertex_simplify"):
        mk(is_simplified=True)
    plain, simp = mk(), mk(vertex_simplify=True)
    assert plain.planner.vertex_simplify is False and simp.planner.vertex_simplify is True
    e = int(np.where(c.status == 0)[0][0])
    start, goal = c.start[e].cpu().numpy(), c.goal[e].cpu().numpy()
    timelimit = 1.5
    iters = int(round(timelimit * ITERS_PER_SECOND))
    # the single-query plan samples stream (seed, 0) on its first call
    st, rows, _, _ = c.orc.plan(start, goal, pi.spec.range, 0.005, iters, NODES, seed=PLAN_SEED, env_id=0, max_path=PATH)
    assert st == 0 and len(rows) >= 3
    keep, _, _, _ = R.simplify_path(c.orc, rows, PLAN_SEED, 0)
    assert len(keep) < len(rows)
    traj0, states0, v0, x0 = plain.plan(start, goal, timelimit)
    assert v0 and x0 and np.array_equal(_bits(states0), _bits(rows))
    traj, states, valid, exact = simp.plan(start, goal, timelimit)
    assert valid and exact and np.array_equal(_bits(states), _bits(rows[keep]))
    want = np.add.accumulate(np.vstack([start[None], simp._unwrapped_steps(rows[keep])]), axis=0)
    assert np.array_equal(_bits(traj), _bits(want))
    assert simp.get_planner_status() == "Exact solution"


def test_rollout_forms_agree_with_the_flag(ctxs):
    """64 Push envs driven into blocked targets: lock-step and asynchronous (a small first budget, continuation chained behind it)
    give every env the same transitions with vertex_simplify on, and with it off; the flag changes what is executed"""
    import torch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    E, T = 64, 3
    rng = np.random.default_rng(4)
    AC = rng.uniform(-1, 1, size=(E, T, 7)) * rng.choice([0.6, 0.9, 1.0], size=(E, T, 1))
    AC[:, 1, 1], AC[:, 1, 3] = 1.0, -1.0                      # blocked straight lines: RRT-Connect queries
    ACt = torch.tensor(AC, device="cuda")
    runs = {}
    for flag in (True, False):
        for mode in ("lockstep", "async"):
            env = make_env(PUSH, E, seed=12, max_episode_steps=1000)
            env.reset()
            ro = BatchMoPARollout(env, RolloutConfig(timelimit=0.15, max_nodes=512, max_path=128, num_trials=10, async_planner=(mode == "async"),
                                                     planner_first_iters=60, planner_min_job=1, vertex_simplify=flag,
                                                     simple_planner_vertex_simplify=flag))
            seq = [[] for _ in range(E)]
            calls = 0
            while min(len(q) for q in seq) < T:
                te = ro.t_env.clamp(max=T - 1)
                out = ro.agent_step(ACt[torch.arange(E, device="cuda"), te].contiguous())
                st = out["stepped"].cpu().numpy()
                rows = np.concatenate([out["rew"].cpu().numpy()[:, None], out["done"].cpu().numpy()[:, None].astype(np.float64),
                                       out["intra_steps"].cpu().numpy()[:, None].astype(np.float64), env.qpos.cpu().numpy()[:, :9],
                                       out["ac"].cpu().numpy()], axis=1)
                for e in np.where(st)[0]:
                    seq[e].append(rows[e])
                calls += 1
                assert calls < 100
            runs[flag, mode] = (np.array([np.array(q[:T]) for q in seq]), int(ro.counters["mp"].sum()), getattr(ro, "n_retried", 0))
    for flag in (True, False):
        assert np.array_equal(_bits(runs[flag, "lockstep"][0]), _bits(runs[flag, "async"][0])), f"vertex_simplify={flag}"
        assert runs[flag, "lockstep"][1] > 0 and int(runs[flag, "async"][2]) > 0          # planner used, second launches happened
    on, off = runs[True, "lockstep"][0], runs[False, "lockstep"][0]
    assert not np.array_equal(_bits(on), _bits(off)), "the flag changed nothing: no planner path was simplified"
