"""K3 race on the GPU: k_rrt_connect<K3Race> + k_race_pick (csrc/mopa_planner_k3.inc, mopa_race.inc) against the sequential form
race_ref.py over the shared cases of race_cases.py -- every output on bit patterns, no tolerances --, portfolio 1 against `plan`, the
independence of the result from timing (no_abort, three workgroups, a permutation, a side stream), K9 behind the race and the drop-in
class."""
import numpy as np
import pytest

import race_cases as RC
import race_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(res):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in res]


def _assert_equal(got, want, what=""):
    """got: plan_race's (path, plen, status, n_checks, winner, win_seed[, info]) as numpy; want: race_ref.as_arrays' tuple"""
    assert np.array_equal(got[2], want[2]), f"{what}: status differs\n{got[2]}\n{want[2]}"
    assert np.array_equal(got[4], want[4]), f"{what}: winner differs\n{got[4]}\n{want[4]}"
    assert np.array_equal(got[1], want[1]), f"{what}: path_len differs"
    assert np.array_equal(got[3], want[3]), f"{what}: n_checks differs"
    assert np.array_equal(got[5], want[5]), f"{what}: win_seed differs"
    for e in range(len(want[1])):
        n = int(want[1][e])
        assert np.array_equal(_bits(got[0][e, :n]), _bits(want[0][e, :n])), f"{what}: rows of query {e} differ"
    if len(got) > 6:
        assert np.array_equal(got[6][:, 2], want[6]), f"{what}: the winner's iterations differ"


class Ctx:
    def __init__(self, O, case):
        import torch
        from mopa_rl_amd import _lib
        from mopa_rl_amd.batch import BatchPlanner
        self.case = case
        self.env, start, goal, ids, self.iters = RC.queries(O, case, invalid_goal=True)
        self.pi, self.orc = RC.scene_of(O, self.env)
        pi = self.pi
        self.scene = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range,
                                seed=0, device=0)
        self.bp = BatchPlanner(self.scene)
        self.start, self.goal = torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()
        self.ids = torch.from_numpy(ids).cuda()
        self.prm = dict(portfolio=RC.K, max_iters=self.iters, max_nodes=RC.MAX_NODES, max_path=RC.MAX_PATH, seed=RC.SEED, env_ids=self.ids)
        self.want = R.as_arrays(RC.reference(O, case, invalid_goal=True), RC.MAX_PATH, self.scene.nq)


@pytest.fixture(scope="module")
def ctxs(oracle_mod):
    return {case: Ctx(oracle_mod, case) for case in RC.CASES}


@pytest.fixture(scope="module")
def full(ctxs):
    """the plain race launch of every case, made once"""
    return {case: _np(c.bp.plan_race(c.start, c.goal, want_info=True, **c.prm)) for case, c in ctxs.items()}


@pytest.mark.parametrize("case", list(RC.CASES))
def test_cases_equal_the_reference(ctxs, full, case):
    """fails on a library without mopa_plan_race_batch"""
    c, got = ctxs[case], full[case]
    assert c.want[2][-1] == -5 and (c.want[2] == 0).any()
    _assert_equal(got, c.want, case)
    # members cut / checks spent depend on timing; their bounds do not
    assert ((got[6][:, 0] >= 0) & (got[6][:, 0] <= RC.K - 1)).all() and (got[6][:, 1] <= c.want[7]).all() and (got[6][:, 1] >= got[3]).all()


def test_portfolio_one_equals_plan(ctxs):
    c = ctxs["push16"]
    prm = dict(c.prm, portfolio=1)
    race = _np(c.bp.plan_race(c.start, c.goal, **prm))
    del prm["portfolio"]
    plain = _np(c.bp.plan(c.start, c.goal, **prm))
    assert (plain[2] == 0).sum() >= 4 and (plain[2] == -4).any() and plain[2][-1] == -5
    assert np.array_equal(race[2], plain[2]) and np.array_equal(race[1], plain[1]) and np.array_equal(race[3], plain[3])
    for e in range(len(plain[1])):
        n = int(plain[1][e])
        assert np.array_equal(_bits(race[0][e, :n]), _bits(plain[0][e, :n])), e
    assert np.array_equal(race[4], np.where(plain[2] == 0, 0, -1)) and (race[5] == RC.SEED).all()


@pytest.mark.parametrize("how", ["no_abort", "three_workgroups", "permuted", "side_stream"])
def test_the_rule_does_not_depend_on_timing(ctxs, full, how):
    import torch
    c = ctxs["pusher48"]
    want = c.want
    if how == "no_abort":
        got = _np(c.bp.plan_race(c.start, c.goal, want_info=True, no_abort=True, **c.prm))
        assert (got[6][:, 0] == 0).all() and np.array_equal(got[6][:, 1], want[7])
    elif how == "three_workgroups":                # members of a query are no longer resident together
        got = _np(c.bp.plan_race(c.start, c.goal, want_info=True, max_workgroups=3, **c.prm))
    elif how == "permuted":
        perm = np.random.default_rng(5).permutation(len(want[1]))
        idx = torch.from_numpy(perm).cuda()
        got = _np(c.bp.plan_race(c.start[idx].contiguous(), c.goal[idx].contiguous(), want_info=True, **dict(c.prm, env_ids=c.ids[idx].contiguous())))
        want = [a[perm] for a in want]
    else:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        res = c.bp.plan_race(c.start, c.goal, want_info=True, stream=side, **c.prm)
        side.synchronize()
        got = _np(res)
    _assert_equal(got, want, how)
    if how != "no_abort":
        assert ((got[6][:, 0] >= 0) & (got[6][:, 0] <= RC.K - 1)).all() and (got[6][:, 1] <= want[7]).all()
    for a, b in zip(got[:6], full["pusher48"][:6]) if how != "permuted" else ():
        assert a.tobytes() == b.tobytes()


def test_k9_behind_the_race(ctxs, full):
    """plan_race(path_shortcut, path_smooth, vertex_simplify) = plan_race followed by smooth_paths(seeds=win_seed, passes=15)"""
    import torch
    c = ctxs["push16"]
    path, plen, status, nchk, winner, wseed = (torch.from_numpy(a.copy()).cuda() for a in full["push16"][:6])
    before = path.clone()
    assert ((status == 0) & (plen >= 3)).sum() >= 4 and len(set(wseed[status == 0].tolist())) >= 2
    c.bp.smooth_paths(path, plen, status, seed=RC.SEED, env_ids=c.ids, seeds=wseed, passes=15)
    got = _np(c.bp.plan_race(c.start, c.goal, path_shortcut=True, path_smooth=True, vertex_simplify=True, **c.prm))
    want = _np((path, plen))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], full["push16"][2]) and np.array_equal(got[3], full["push16"][3])
    assert np.array_equal(got[4], full["push16"][4]) and np.array_equal(got[5], full["push16"][5])
    for e in range(len(want[1])):
        n = int(want[1][e])
        assert np.array_equal(_bits(got[0][e, :n]), _bits(want[0][e, :n])), f"rows of query {e} differ"
    assert not torch.equal(before, path), "K9 changed nothing"


def test_drop_in_class_returns_the_winner_where_the_plain_query_fails(oracle_mod, ctxs):
    """pusher48 query 0 (stream id 5): member 0 runs out of its 2000 iterations, member 7 wins.  A planner object with seed 23 whose
    plan counter stands at 5 draws exactly that stream."""
    from mopa_rl_amd.planner import ITERS_PER_SECOND, MAX_NODES, MAX_PATH, PyKinematicPlanner
    assert (ITERS_PER_SECOND, MAX_NODES) == (2000, RC.MAX_NODES)
    c = ctxs["pusher48"]
    pi = c.pi
    _, s, g, ids, iters = RC.queries(oracle_mod, "pusher48")
    assert ids[0] == 5 and iters == 2000
    want = R.race(c.orc, s[0], g[0], pi.spec.range, RC.K, iters, MAX_NODES, MAX_PATH, RC.SEED, 5)
    assert want.status == 0 and want.winner != 0 and want.members[0].status == -4
    args = lambda algo: (b"pusher_obstacle.xml", algo, 4, b"", 0.0, pi.spec.range, pi.passive_joint_idx, [], pi.ignored_contacts,
                         pi.spec.contact_threshold, 0.05, False, 0.1, RC.SEED)
    pk = PyKinematicPlanner(*args(b"rrt_connect"))
    pk._plan_count = 5
    assert pk.portfolio == 1
    assert pk.plan(s[0], g[0], 1.0) == [[-4.0] * c.scene.nq] and pk.getPlannerStatus() == b"Timeout"
    pk._plan_count = 5
    pk.portfolio = RC.K
    rows = np.array(pk.plan(s[0], g[0], 1.0))
    assert np.array_equal(_bits(rows), _bits(want.rows)) and pk.getPlannerStatus() == b"Exact solution"
    st, prow, chk, win, wseed, info = c.scene.plan_race(s[0], g[0], RC.K, iters, MAX_NODES, MAX_PATH, seed=RC.SEED, env_id=5)
    assert (st, chk, win, wseed, int(info[2])) == (0, want.n_checks, want.winner, want.win_seed, want.iters)
    star = PyKinematicPlanner(*args(b"rrt_star"))
    star.portfolio = 2
    with pytest.raises(NotImplementedError, match="portfolio"):
        star.plan(s[0], g[0], 0.01)


def test_argument_errors_return_their_codes(ctxs):
    import ctypes as C
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import _ptr
    c = ctxs["push16"]
    L = _lib.lib()
    E = 2
    path = torch.zeros(E, 8, c.scene.nq, dtype=torch.float64, device="cuda")
    plen = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    status = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    nchk = torch.zeros(E, dtype=torch.int64, device="cuda")
    winner = torch.zeros(E, dtype=torch.int32, device="cuda")
    wseed = torch.zeros(E, dtype=torch.int64, device="cuda")

    def call(scene=c.scene.handle, E=E, iters=10, nodes=64, mp=8, K=4, p=_ptr(path), w=_ptr(winner)):
        prm = _lib.MopaRaceParams(iters, nodes, mp, K, 1, 0, None, None, 0, 0)
        return L.mopa_plan_race_batch(scene, _ptr(c.start), _ptr(c.goal), E, C.byref(prm), p, _ptr(plen), _ptr(status), _ptr(nchk), w, _ptr(wseed),
                                      None, None)
    assert call(scene=None) == 1 and call(E=-1) == 1 and call(iters=-1) == 1 and call(nodes=1) == 1 and call(mp=1) == 1
    assert call(K=0) == 1 and call(K=257) == 1 and call(p=None) == 1 and call(w=None) == 1
    assert call(nodes=1 << 30, K=256) == 4 and b"bytes" in L.mopa_last_error()         # trees the device cannot hold: no launch, no fault
    assert call(E=0) == 0
    torch.cuda.synchronize()
    assert (plen == 77).all() and (status == 77).all(), "a rejected call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    assert set(status.cpu().tolist()) <= {0, -4}
