"""K3b RRT* on the CPU: the invariants of the sequential reference rrtstar_ref.py (the definition the kernel k_rrt_star has to
reproduce), the coverage of its branches by the shared cases of star_cases.py, the host table k(n) of the library, and the
constructor surface of the drop-in planner."""
import math

import numpy as np
import pytest

import rrtstar_ref as R
import star_cases as SC
from simplify_ref import dist, so2_flags


def _check_tree(orc, res, start):
    """every returned segment passes check_motion; cost = the chain's top-down sum; every node's cost = cost[parent] + inc"""
    Q, parent, inc, cost, goals = res.tree
    so2 = so2_flags(orc.model, orc.active_idx)
    assert parent[0] == -1 and cost[0] == 0.0 and inc[0] == 0.0
    for i in range(1, len(Q)):
        p = int(parent[i])
        assert 0 <= p < len(Q) and p != i
        assert cost[i] == cost[p] + inc[i], f"node {i}: cost is not its parent's plus the increment"
        assert inc[i] == dist(Q[p], Q[i], so2)
    if res.status != R.PLAN_OK:
        assert len(res.rows) == 0 and res.cost == math.inf
        return
    act = np.asarray(orc.active_idx)
    rows = res.rows
    assert np.array_equal(rows[0], start) and 2 <= len(rows)
    total = 0.0
    for k in range(len(rows) - 1):
        assert orc.check_motion(rows[0], rows[k, act], rows[k + 1, act], 0.005)[0], f"segment {k} fails the motion check"
        total = total + dist(rows[k, act], rows[k + 1, act], so2)
    assert res.cost == total
    chain = res.events["chain"]
    assert chain[0] == 0 and chain[-1] in goals and all(cost[chain[-1]] <= cost[g] for g in goals)
    # passive columns are the start row's
    passive = np.setdiff1d(np.arange(rows.shape[1]), act)
    assert np.array_equal(rows[:, passive], np.repeat(start[None, passive], len(rows), axis=0))


def test_pusher_cases_cover_the_branches(oracle_mod):
    pi, orc = SC.scene_of(oracle_mod, SC.PUSHER)
    start, goal = SC.queries(oracle_mod, SC.PUSHER)
    path, plen, status, cost, info, res = SC.reference(oracle_mod, SC.PUSHER)
    assert (status == 0).all(), "all 16 Pusher queries are solved"
    assert plen.min() >= 2 and plen.max() <= 7
    assert sum(r.events["rewire"] >= 1 for r in res) >= 8, "half of the queries rewire"
    assert sum(r.events["desc"] >= 1 for r in res) >= 1, "a rewire that refreshes a descendant's cost"
    assert all(r.events["parent_not_nearest"] >= 1 for r in res), "every query chooses a parent other than the nearest node"
    assert (info[:, 0] == SC.MAX_ITERS).all() and (info[:, 7] == 0).all()
    assert all(r.events["trapped"] >= 1 for r in res)
    for e, r in enumerate(res):
        _check_tree(orc, r, start[e])
        assert np.array_equal(path[e, plen[e] - 1, orc.active_idx], goal[e, orc.active_idx]), "threshold 0: the path ends in the goal itself"
    # neither branch is reachable from these cases (DESIGN.md "K3b RRT*" says why): a failed verdict re-used by a rewire, a
    # nearest node outside the neighbour set
    assert not any(r.events["reused_fail"] or r.events["nearest_outside"] for r in res)


def test_pusher_threshold_variant_has_several_goal_nodes(oracle_mod):
    pi, orc = SC.scene_of(oracle_mod, SC.PUSHER)
    start, _ = SC.queries(oracle_mod, SC.PUSHER)
    path, plen, status, cost, info, res = SC.reference(oracle_mod, SC.PUSHER, variant=True)
    assert (status == 0).all()
    assert sum(info[:, 4] >= 2) >= 1, "a query that ends with two goal nodes"
    for e, r in enumerate(res):
        _check_tree(orc, r, start[e])
        assert dist(path[e, plen[e] - 1, orc.active_idx], SC.queries(oracle_mod, SC.PUSHER)[1][e, orc.active_idx],
                    so2_flags(orc.model, orc.active_idx)) <= SC.VARIANT["goal_threshold"]


def test_push_cases_have_both_statuses(oracle_mod):
    pi, orc = SC.scene_of(oracle_mod, SC.PUSH)
    start, _ = SC.queries(oracle_mod, SC.PUSH)
    path, plen, status, cost, info, res = SC.reference(oracle_mod, SC.PUSH)
    assert sorted(set(status.tolist())) == [R.PLAN_NO_EXACT, R.PLAN_OK]
    assert (status == 0).sum() >= 4 and (status == R.PLAN_NO_EXACT).sum() >= 4
    assert sum(r.events["rewire"] >= 1 for r in res) >= 1
    assert ((info[:, 5] >= 0) == (status == 0)).all()
    for e, r in enumerate(res):
        _check_tree(orc, r, start[e])


def test_synthetic_cases(oracle_mod):
    pi, orc = SC.scene_of(oracle_mod, SC.PUSHER)
    cases, sid = SC.synthetic(oracle_mod)
    out = {}
    for name, (s, g, kw, want) in cases.items():
        kw = dict(dict(max_path=SC.MAX_PATH), **kw)
        r = R.plan_star(orc, s, g, pi.spec.range, SC.MAX_ITERS, seed=SC.SEED, stream_id=sid, **kw)
        out[name] = r
        if want is not None:
            assert r.status == want, name
    assert out["invalid_goal"].info[2] == 0 and out["invalid_start"].info[2] == 0 and out["invalid_start"].info[5] == -1
    full = out["full_tree"]
    assert full.info[1] == 64 and full.info[7] >= 1, "max_nodes = 64: iterations that find the tree full"
    assert full.info[0] == SC.MAX_ITERS
    _check_tree(orc, full, cases["full_tree"][0])
    short = out["short_max_path"]
    assert short.info[4] >= 1 and len(short.rows) == 0, "a goal node exists, its chain has more than max_path rows"


def test_k_table_of_the_library_is_pythons():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    for na in (4, 7):
        for n in range(1, 4097):
            assert L.mopa_plan_star_k(na, n, R.REWIRE_FACTOR) == R.k_of(na, n), (na, n)
    assert L.mopa_plan_star_k(0, 5, 1.1) == -1 and L.mopa_plan_star_k(4, 0, 1.1) == -1
    assert R.k_of(4, 4097) <= R.K_MAX and R.k_of(7, 4097) <= R.K_MAX


def test_native_planner_takes_rrt_star_by_that_name_only():
    """fails on a tree without the feature: `rrt_star` raises there.  Checked up to the scene's creation, which needs a device."""
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.planner import PyKinematicPlanner
    mk = lambda algo, opt=b"path_length": PyKinematicPlanner(b"pusher_obstacle.xml", algo, 4, opt, 0.0, 0.2, [], [], [], -0.001, 0.05, False, 0.1, 0)
    with pytest.raises(NotImplementedError, match="rrt_star"):
        mk(b"rrt")
    with pytest.raises(NotImplementedError, match="path-length"):
        mk(b"rrt_star", b"maximize_min_clearance")
    with pytest.raises(NotImplementedError):
        PyKinematicPlanner(b"pusher_obstacle.xml", b"rrt_star", 4, b"", 0.0, 0.2, [], [], [], -0.001, 0.05, True, 0.1, 0)
    if torch.cuda.is_available():
        assert mk(b"rrt_star").algo == "rrt_star" and mk(b"rrt_star", b"").opt == ""
    else:
        with pytest.raises(_lib.MopaError, match="no HIP device"):       # past the argument checks: only the device is missing
            mk(b"rrt_star")
        mk_c = lambda: mk(b"rrt_connect", b"maximize_min_clearance")      # other objectives stay accepted and ignored there
        with pytest.raises(_lib.MopaError, match="no HIP device"):
            mk_c()
