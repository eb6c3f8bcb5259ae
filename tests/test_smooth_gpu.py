"""K9 smoothBSpline on the GPU: k_smooth_paths (csrc/mopa_k9.inc) against the sequential reference smooth_ref.py -- the rows,
new and moved states included, on bit patterns, lengths and all ten info columns -- over the blocked Push / Pusher queries of
test_smooth_host.py and over synthetic paths; bit 3 clear against k_shortcut_paths, skipped paths, ids / seeds, streams,
continuation, argument errors, and the flag through SamplingBasedPlanner and the rollout."""
import os
import re

import numpy as np
import pytest

import smooth_ref as B
from simplify_cases import (MAX_NODES, MAX_PATH, PLAN_SEED, QUERY_SETS, blocked_queries, oracle_plans, push_out_and_back,
                            pusher_wrap_path, scene_of)

pytestmark = pytest.mark.gpu

PUSH, PUSHER = "SawyerPushObstacle-v0", "PusherObstacle-v0"
NAN_BITS = 0x7FF8DEADBEEF0001          # a quiet NaN with a payload: what never-written rows hold
ALL = dict(vertex_simplify=True, path_shortcut=True, path_smooth=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_rows(got_path, got_len, want_path, want_len, what=""):
    assert np.array_equal(got_len, want_len), f"{what}: path_len differs: {got_len} != {want_len}"
    for e in range(len(want_len)):
        n = int(want_len[e])
        assert np.array_equal(_bits(got_path[e, :n]), _bits(want_path[e, :n])), f"{what}: rows of path {e} differ"


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Ctx:
    """per env: scene, the oracle's and the device planner's paths of the blocked queries (never modified) and their reference
    forms: passes = 12 over the oracle's rows (the host test's coverage conditions hold for these), passes = 15 over the device's"""

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
        self.ref15 = B.smooth_batch(self.orc, self.path, self.plen, self.status, seed=PLAN_SEED, passes=15)
        ost, opaths = oracle_plans(pi, self.orc, env, start, goal)
        self.opath = np.zeros((len(ost), MAX_PATH, self.orc.nq))
        self.oplen = np.zeros(len(ost), dtype=np.int32)
        for e, p in enumerate(opaths):
            self.opath[e, :len(p)] = p
            self.oplen[e] = len(p)
        self.ostatus = ost
        self.oref12 = B.smooth_batch(self.orc, self.opath, self.oplen, ost, seed=PLAN_SEED, passes=12)

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


def _run(bp, path, plen, status=None, **kw):
    """smooth_paths on copies of numpy arrays -> (path, plen, info) as numpy"""
    import torch
    p, n = _cuda(path), _cuda(plen)
    info = bp.smooth_paths(p, n, _cuda(status) if status is not None else None, want_info=True, **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), n.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("env", [PUSH, PUSHER])
def test_planned_paths_equal_the_reference(ctxs, env):
    """fails on a library without mopa_smooth_paths_batch"""
    import torch
    c = ctxs[env]
    # the oracle's rows, shortcutPath + smoothBSpline: the cases whose coverage the host test asserts
    want_path, want_len, want_info, runs = c.oref12
    solved = [e for e in range(len(c.ostatus)) if c.ostatus[e] == 0]
    assert len(solved) >= (8 if env == PUSH else 3)
    ev = {k: sum(runs[e].events[k] for e in solved) for k in runs[solved[0]].events}
    assert min(ev["moved"], ev["below_min"], ev["fail_first"], ev["fail_second"], ev["no_move"]) >= 1, "the cases do not exercise every outcome"
    if env == PUSH:
        assert min(ev["invalid_mid"], ev["outer_fail"], ev["mid_dropped"]) >= 1
    else:
        assert ev["seam_eval"] >= 1
    got = _run(c.bp, c.opath, c.oplen, c.ostatus, seed=PLAN_SEED, passes=12)
    print(env, "info sums, device:", got[2].sum(axis=0), "reference:", want_info.sum(axis=0))
    _assert_rows(got[0], got[1], want_path, want_len, "smooth_paths(passes=12) on the oracle's rows")
    assert np.array_equal(got[2], want_info), "info differs"
    # the flags on plan(): the device planner's own rows through passes = 15; n_checks stays the planner's own count
    want_path, want_len, want_info, _ = c.ref15
    one = c.bp.plan(c.start, c.goal, **ALL, **c.prm)
    torch.cuda.synchronize()
    _assert_rows(one[0].cpu().numpy(), one[1].cpu().numpy(), want_path, want_len, "plan(vertex_simplify, path_shortcut, path_smooth)")
    assert np.array_equal(one[2].cpu().numpy(), c.status) and np.array_equal(one[3].cpu().numpy(), c.nchk)
    path, plen, status, _ = c.clones()
    info = c.bp.smooth_paths(path, plen, status, seed=PLAN_SEED, want_info=True)
    torch.cuda.synchronize()
    _assert_rows(path.cpu().numpy(), plen.cpu().numpy(), want_path, want_len, "two-step form")
    assert np.array_equal(info.cpu().numpy(), want_info) and np.array_equal(status.cpu().numpy(), c.status)
    assert int(info[:, 7].sum()) >= 1, "no vertex was moved"
    # flag off: what the planner gave before
    off = c.bp.plan(c.start, c.goal, path_smooth=False, **c.prm)
    _assert_rows(off[0].cpu().numpy(), off[1].cpu().numpy(), c.path, c.plen, "plan()")


@pytest.mark.parametrize("passes", [8, 9, 10, 11, 12, 13, 14, 15])
def test_each_passes_on_out_and_back(ctxs, passes):
    c = ctxs[PUSH]
    rows = push_out_and_back(c.pi, c.orc)
    assert len(rows) == 12
    cases = [rows, rows[::-1].copy(), rows[:7]]
    path = np.zeros((len(cases), 32, c.orc.nq))
    plen = np.array([len(r) for r in cases], dtype=np.int32)
    for k, r in enumerate(cases):
        path[k, :len(r)] = r
    want = B.smooth_batch(c.orc, path, plen, None, seed=5, env_id_base=3, passes=passes)
    assert want[2][:, 6].sum() >= 1 and want[2][:, 9].sum() >= 1, "no smoothing step was taken"
    got = _run(c.bp, path, plen, None, seed=5, env_id_base=3, passes=passes)
    _assert_rows(got[0], got[1], want[0], want[1], f"passes={passes}")
    assert np.array_equal(got[2], want[2]), f"info differs: {got[2]} != {want[2]}"


@pytest.mark.parametrize("max_path", [6, 7, 13, 256])
def test_wrap_path_and_the_capacity_stop(ctxs, max_path):
    c = ctxs[PUSHER]
    rows = pusher_wrap_path(c.pi, c.orc)
    path = np.zeros((2, max_path, c.orc.nq))
    path[:, :4] = rows
    path[1, :4] = rows[::-1]
    plen = np.array([4, 4], dtype=np.int32)
    want = B.smooth_batch(c.orc, path, plen, None, seed=3, env_id_base=0, passes=8)
    steps, stops, rows_out = {6: (0, 1, 4), 7: (1, 1, 7), 13: (2, 1, 13), 256: (3, 0, 13)}[max_path]
    assert (want[2][0, 6], want[2][0, 4], want[1][0]) == (steps, stops, rows_out), "the reference does not take the steps the case is about"
    if max_path >= 13:
        assert want[3][0].events["seam_eval"] >= 1 and want[2][0, 7] >= 1, "no move across the seam"
    got = _run(c.bp, path, plen, None, seed=3, env_id_base=0, passes=8)
    _assert_rows(got[0], got[1], want[0], want[1], f"max_path={max_path}")
    assert np.array_equal(got[2], want[2]) and got[1].max() <= max_path, f"info differs: {got[2]} != {want[2]}"


@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5, 6, 7])
def test_bit_3_clear_gives_the_bytes_of_shortcut_paths(ctxs, passes):
    import torch
    c = ctxs[PUSH]
    a, b = c.clones(), c.clones()
    ia = c.bp.shortcut_paths(a[0], a[1], a[2], seed=PLAN_SEED, passes=passes, want_info=True)
    ib = c.bp.smooth_paths(b[0], b[1], b[2], seed=PLAN_SEED, passes=passes, want_info=True)
    torch.cuda.synchronize()
    _assert_rows(b[0].cpu().numpy(), b[1].cpu().numpy(), a[0].cpu().numpy(), a[1].cpu().numpy(), f"passes={passes}")
    assert torch.equal(ia, ib[:, :6]) and not ib[:, 6:].any()
    assert not torch.equal(a[1], c.planned[1]) or passes == 2


def test_skipped_paths_are_not_touched(ctxs):
    c = ctxs[PUSH]
    e0 = int(np.where(c.status == 0)[0][0])
    L = int(c.plen[e0])
    MP = 2 * L + 3
    status = np.array([0, -4, -5, 0, 0, 0, 0], dtype=np.int32)
    plen = np.array([L, L, L, 0, 2, MP + 1, L], dtype=np.int32)
    E = len(plen)
    base = _filled(E, MP, c.orc.nq)
    for e in range(E):
        base[e, :L] = c.planned[0][e0, :L]
    before = base.cpu().numpy()
    info0 = np.full((E, 10), -7, dtype=np.int64)
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    path, n, st, info = base.clone(), _cuda(plen), _cuda(status), _cuda(info0)
    _lib.check(_lib.lib().mopa_smooth_paths_batch(c.scene.handle, E, MP, _ptr(path), _ptr(n), _ptr(st), PLAN_SEED, e0, None, None, 15, 16,
                                                  _ptr(info), None))
    torch.cuda.synchronize()
    got, got_n, got_info = path.cpu().numpy(), n.cpu().numpy(), info.cpu().numpy()
    want = B.smooth_batch(c.orc, before, plen, status, seed=PLAN_SEED, env_id_base=e0, passes=15)
    for e in (1, 2, 3, 4, 5):
        assert np.array_equal(_bits(got[e]), _bits(before[e])), f"bytes of skipped path {e} changed"
        assert got_n[e] == plen[e] and np.array_equal(got_info[e], info0[e]), f"length or info of skipped path {e} changed"
    for e in (0, 6):
        n_e = int(want[1][e])
        assert got_n[e] == n_e and np.array_equal(_bits(got[e, :n_e]), _bits(want[0][e, :n_e])) and np.array_equal(got_info[e], want[2][e])
    assert got_info[0, 6] >= 1 and got_info[0, 5] <= MP


def test_per_query_ids_and_seeds_equal_the_scalar_form(ctxs):
    import torch
    c = ctxs[PUSH]
    solved = np.where(c.status == 0)[0]
    sub = np.concatenate([solved[::-2], np.where(c.status != 0)[0][:2]])      # reordered, with two unsolved queries
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device="cuda")
    idx = t(sub, torch.int64)
    path, plen, status = c.planned[0][idx].contiguous(), c.planned[1][idx].contiguous(), c.planned[2][idx].contiguous()
    c.bp.smooth_paths(path, plen, status, seed=999, env_id_base=555, env_ids=idx, seeds=t([PLAN_SEED] * len(sub), torch.int64))
    torch.cuda.synchronize()
    _assert_rows(path.cpu().numpy(), plen.cpu().numpy(), c.ref15[0][sub], c.ref15[1][sub], "subset")


def test_two_streams_write_the_same_bytes(ctxs):
    import torch
    c = ctxs[PUSHER]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = c.clones(), c.clones()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(s1):
            ia = c.bp.smooth_paths(a[0], a[1], a[2], seed=PLAN_SEED, stream=s1, want_info=True)
        with torch.cuda.stream(s2):
            ib = c.bp.smooth_paths(b[0], b[1], b[2], seed=PLAN_SEED, stream=s2, want_info=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(ia, ib)
    _assert_rows(a[0].cpu().numpy(), a[1].cpu().numpy(), c.ref15[0], c.ref15[1], "stream 1")
    _assert_rows(b[0].cpu().numpy(), b[1].cpu().numpy(), c.ref15[0], c.ref15[1], "stream 2")
    assert np.array_equal(ia.cpu().numpy(), c.ref15[2])


def test_continuation_smooths_every_query_once(ctxs):
    import torch
    c = ctxs[PUSH]
    prm = dict(c.prm)
    full_iters = prm.pop("max_iters")
    p1 = c.bp.plan(c.start, c.goal, max_iters=30, keep_state=True, **ALL, **prm)
    p2 = c.bp.plan(c.start, c.goal, max_iters=full_iters, resume=p1[4], **ALL, **prm)
    torch.cuda.synchronize()
    n1, n2 = p1[1].cpu().numpy(), p2[1].cpu().numpy()
    assert (n1 > 0).sum() >= 2 and (n2 > 0).sum() >= 2 and not ((n1 > 0) & (n2 > 0)).any(), "both launches must solve some queries"
    late = torch.from_numpy(n2 > 0).cuda()
    path = torch.where(late[:, None, None], p2[0], p1[0]).cpu().numpy()
    plen = np.where(n2 > 0, n2, n1)
    _assert_rows(path, plen, c.ref15[0], c.ref15[1], "first launch + continuation")
    assert np.array_equal(plen > 0, c.status == 0)


def test_argument_errors_return_their_codes(ctxs):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    c = ctxs[PUSH]
    L = _lib.lib()
    cap = L.mopa_smooth_paths_max_path(c.scene.handle)
    assert MAX_PATH <= cap <= L.mopa_shortcut_paths_max_path(c.scene.handle)
    path, plen, status, _ = c.clones()
    before = (path.clone(), plen.clone())
    h, E = c.scene.handle, path.shape[0]
    call = lambda scene=h, E=E, mp=MAX_PATH, p=_ptr(path), n=_ptr(plen), passes=15, rounds=16: L.mopa_smooth_paths_batch(
        scene, E, mp, p, n, _ptr(status), PLAN_SEED, 0, None, None, passes, rounds, None, None)
    assert call(scene=None) == 1 and call(E=-1) == 1 and call(mp=1) == 1 and call(passes=0) == 1 and call(passes=16) == 1
    assert call(rounds=0) == 1 and call(p=None) == 1 and call(n=None) == 1
    assert call(mp=cap + 1) == 2 and b"max_path" in L.mopa_last_error()           # MOPA_ERR_UNSUPPORTED
    assert call(E=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(path, before[0]) and torch.equal(plen, before[1]), "a rejected call launched something"
    with pytest.raises(_lib.MopaError):
        c.bp.smooth_paths(path, plen.to(torch.int64), status)
    with pytest.raises(_lib.MopaError):
        c.bp.smooth_paths(path, plen, status, passes=16)
    # the older entry points keep rejecting the newer bits
    assert L.mopa_shortcut_paths_batch(h, E, MAX_PATH, _ptr(path), _ptr(plen), _ptr(status), PLAN_SEED, 0, None, None, 8, 16, None, None) == 1
    assert L.mopa_simplify_paths_batch(h, E, MAX_PATH, _ptr(path), _ptr(plen), _ptr(status), PLAN_SEED, 0, None, None, 4, None, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(path, before[0]) and torch.equal(plen, before[1]), "a rejected call launched something"


def test_symbols_are_declared_and_exported():
    from mopa_rl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mopa_hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for sym in ("mopa_smooth_paths_batch", "mopa_smooth_paths_max_path"):
        assert re.search(r"\bint " + sym + r"\(", header), f"{sym} is not declared in the header"
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(L, sym) is not None


def test_sampling_based_planner_returns_the_unwrapped_reference_rows(ctxs):
    """the flag through the drop-in classes: `states` are the reference's rows of the single-query plan, `traj` their un-wrapped
    form; is_simplified keeps raising and names all three attributes"""
    import types
    from mopa_rl_amd import _lib
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_NODES as NODES, MAX_PATH as PATH
    from mopa_rl_amd.planner_agent import PlannerAgent
    from mopa_rl_amd.sampling_based_planner import SamplingBasedPlanner
    c = ctxs[PUSHER]
    pi = c.pi
    cfg = types.SimpleNamespace(planner_type="rrt_connect", range=pi.spec.range, planner_objective="path_length", threshold=0.0, seed=PLAN_SEED,
                                _xml_path="pusher_obstacle.xml", contact_threshold=pi.spec.contact_threshold, timelimit=1.5)
    mk = lambda **kw: SamplingBasedPlanner(cfg, "pusher_obstacle.xml", 4, pi.non_limited_idx, passive_joint_idx=pi.passive_joint_idx,
                                           ignored_contacts=pi.ignored_contacts, contact_threshold=pi.spec.contact_threshold, **kw)
    with pytest.raises(NotImplementedError, match="vertex_simplify") as err:
        mk(is_simplified=True, path_smooth=True)
    assert "path_shortcut" in str(err.value) and "path_smooth" in str(err.value) and "wall clock" in str(err.value)
    plain, both, every = mk(), mk(path_shortcut=True, path_smooth=True), mk(**ALL)
    assert plain.planner.path_smooth is False and both.planner.path_smooth is True and both.planner.vertex_simplify is False
    agent = PlannerAgent(cfg, 4, pi.non_limited_idx, passive_joint_idx=pi.passive_joint_idx, ignored_contacts=pi.ignored_contacts,
                         path_smooth=True)
    assert agent.planner.planner.path_smooth is True and agent.planner.planner.path_shortcut is False
    e = int(np.where(c.status == 0)[0][0])
    start, goal = c.start[e].cpu().numpy(), c.goal[e].cpu().numpy()
    timelimit = 1.5
    iters = int(round(timelimit * ITERS_PER_SECOND))
    # the single-query plan samples stream (seed, 0) on its first call
    st, rows, _, _ = c.orc.plan(start, goal, pi.spec.range, 0.005, iters, NODES, seed=PLAN_SEED, env_id=0, max_path=PATH)
    assert st == 0 and len(rows) >= 3
    cap = min(PATH, _lib.lib().mopa_smooth_paths_max_path(c.scene.handle))          # the capacity PyKinematicPlanner gives the rows
    for planner, passes in ((both, 12), (every, 15)):
        ref = B.SmoothSimplifier(c.orc, rows, PLAN_SEED, 0, max_path=cap)
        ref.run(passes)
        want_rows = ref.result_rows()
        assert ref.n_steps >= 1
        traj, states, valid, exact = planner.plan(start, goal, timelimit)
        assert valid and exact and np.array_equal(_bits(states), _bits(want_rows)), f"passes={passes}"
        want = np.add.accumulate(np.vstack([start[None], planner._unwrapped_steps(want_rows)]), axis=0)
        assert np.array_equal(_bits(traj), _bits(want))
        assert planner.get_planner_status() == "Exact solution"
    traj0, states0, v0, x0 = plain.plan(start, goal, timelimit)
    assert v0 and x0 and np.array_equal(_bits(states0), _bits(rows))


def test_rollout_executes_the_rows_of_plan_with_the_flag(ctxs):
    """64 Push envs driven into blocked targets, shortcutPath on in both runs: every planner launch of the rollout carries the
    config's path_smooth, its rows are those of `BatchPlanner.plan` followed by `smooth_paths` for the same queries (flag clear:
    those of `plan(path_shortcut=True)`), and the flag changes what is executed"""
    import torch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout, RolloutConfig
    assert RolloutConfig().path_smooth is False and RolloutConfig().simple_planner_path_smooth is False
    E, T = 64, 3
    rng = np.random.default_rng(4)
    AC = rng.uniform(-1, 1, size=(E, T, 7)) * rng.choice([0.6, 0.9, 1.0], size=(E, T, 1))
    AC[:, 1, 1], AC[:, 1, 3] = 1.0, -1.0                      # blocked straight lines: RRT-Connect queries
    ACt = torch.tensor(AC, device="cuda")
    runs = {}
    for flag in (True, False):
        env = make_env(PUSH, E, seed=12, max_episode_steps=1000)
        env.reset()
        ro = BatchMoPARollout(env, RolloutConfig(timelimit=0.15, max_nodes=512, max_path=128, num_trials=10, path_shortcut=True,
                                                 simple_planner_path_shortcut=True, path_smooth=flag, simple_planner_path_smooth=flag))
        calls = []
        inner = ro.bp.plan

        def spy(start, goal, **kw):
            res = inner(start, goal, **kw)
            calls.append((start.clone(), goal.clone(), dict(kw), [t.clone() for t in res[:3]]))
            return res
        ro.bp.plan = spy
        seq = [[] for _ in range(E)]
        n_calls = 0
        while min(len(q) for q in seq) < T:
            te = ro.t_env.clamp(max=T - 1)
            out = ro.agent_step(ACt[torch.arange(E, device="cuda"), te].contiguous())
            st = out["stepped"].cpu().numpy()
            rows = np.concatenate([out["rew"].cpu().numpy()[:, None], out["intra_steps"].cpu().numpy()[:, None].astype(np.float64),
                                   env.qpos.cpu().numpy()[:, :9], out["ac"].cpu().numpy()], axis=1)
            for e in np.where(st)[0]:
                seq[e].append(rows[e])
            n_calls += 1
            assert n_calls < 100
        torch.cuda.synchronize()
        assert calls and int(ro.counters["mp"].sum()) > 0, "the planner was not used"
        n_changed = 0
        for start, goal, kw, res in calls:
            assert kw.get("path_smooth", False) is flag and kw.get("path_shortcut", False) is True and not kw.get("vertex_simplify", False)
            assert flag or "path_smooth" not in kw, "with the flag off the launches get the keywords they always got"
            base = {k: v for k, v in kw.items() if k not in ("path_shortcut", "path_smooth", "vertex_simplify", "stream", "keep_state", "resume")}
            assert "resume" not in kw or kw["resume"] is None
            cut = inner(start, goal, path_shortcut=True, **base)
            want = inner(start, goal, **base)[:3]
            if flag:
                ro.bp.smooth_paths(want[0], want[1], want[2], seed=base.get("seed", 0), env_id_base=base.get("env_id_base", 0),
                                   env_ids=base.get("env_ids"), seeds=base.get("seeds"), passes=12)
            else:
                want = cut
            torch.cuda.synchronize()
            _assert_rows(res[0].cpu().numpy(), res[1].cpu().numpy(), want[0].cpu().numpy(), want[1].cpu().numpy(), f"path_smooth={flag}")
            if flag:
                n_changed += int((~(cut[0] == want[0]).all(dim=2).all(dim=1)).sum())
        assert not flag or n_changed >= 1, "no planner path was changed by the smoothing"
        runs[flag] = np.array([np.array(q[:T]) for q in seq])
    assert not np.array_equal(_bits(runs[True]), _bits(runs[False])), "the flag changed nothing that was executed"
