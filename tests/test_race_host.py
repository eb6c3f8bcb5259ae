"""The sequential form of the K3 race (race_ref.py over the CPU oracle) on its own, so that the GPU test cannot hide a failure of the
reference: how many queries of pusher48 are decided by the seed, the -5 rule, portfolio 1 = the plain query."""
import numpy as np

import race_cases as RC
import race_ref as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_pusher48_is_decided_by_the_seed_on_a_fifth_of_its_queries(oracle_mod):
    ref = RC.reference(oracle_mod, "pusher48")
    assert len(ref) == 48 and all(len(r.members) == RC.K for r in ref)
    solved = [[m.status == 0 for m in r.members] for r in ref]
    mixed = [g for g, s in enumerate(solved) if any(s) and not all(s)]
    assert len(mixed) >= 8, mixed
    rescued = [g for g in mixed if not solved[g][0]]
    assert len(rescued) >= 2 and 0 in rescued and 20 in rescued, rescued
    other = [g for g, r in enumerate(ref) if r.status == 0 and r.winner != 0]
    assert len(other) >= 3 and {0, 1, 20} <= set(other), other
    assert sum(1 for s in solved if not any(s)) >= 20
    for g, r in enumerate(ref):
        if r.status == 0:
            w = r.members[r.winner]
            assert (w.n_checks, r.winner) == min((m.n_checks, k) for k, m in enumerate(r.members) if m.status == 0)
            assert r.n_checks == w.n_checks and r.win_seed == R.member_seed(RC.SEED, r.winner) and r.iters == w.iters
            assert np.array_equal(_bits(r.rows), _bits(w.rows)) and 2 <= len(r.rows) <= RC.MAX_PATH
        else:
            assert r.status == -4 and r.winner == -1 and len(r.rows) == 0 and r.iters == -1
            assert r.n_checks == r.members[0].n_checks and r.win_seed == RC.SEED


def test_members_that_end_early_unsolved_found_a_chain_longer_than_max_path(oracle_mod):
    """assembly8, queries 1 and 12 (positions 0 and 1): several members stop before the budget with -4; the same member with room for
    the chain solves in the same iterations and checks with more than max_path rows -- it is not solved and never wins"""
    ref = RC.reference(oracle_mod, "assembly8")
    env, s, g, ids, iters = RC.queries(oracle_mod, "assembly8")
    pi, orc = RC.scene_of(oracle_mod, env)
    seen = 0
    for q in (0, 1):
        early = [k for k, m in enumerate(ref[q].members) if m.status == -4 and m.iters < iters]
        assert early, q
        for k in early[:2]:
            m = ref[q].members[k]
            st, rows, chk, it = orc.plan(s[q], g[q], pi.spec.range, 0.005, max_iters=iters, max_nodes=RC.MAX_NODES, seed=m.seed, env_id=int(ids[q]),
                                         max_path=4 * RC.MAX_PATH)
            assert st == 0 and len(rows) > RC.MAX_PATH and chk == m.n_checks and it == m.iters
            seen += 1
        assert ref[q].winner != -1 and ref[q].members[ref[q].winner].status == 0
    assert seen >= 2


def test_push16_holds_the_wide_spread_query(oracle_mod):
    ref = RC.reference(oracle_mod, "push16")
    m = ref[9].members
    assert m[0].status == 0 and m[5].status == 0 and m[0].iters >= 300 and m[5].iters <= 10 and len(m[5].rows) < len(m[0].rows)
    assert ref[9].winner == 5


def test_invalid_goal_gives_minus_five(oracle_mod):
    for case in RC.CASES:
        r = RC.reference(oracle_mod, case, invalid_goal=True)[-1]
        assert r.status == -5 and r.winner == -1 and len(r.rows) == 0 and r.n_checks == 1 and r.win_seed == RC.SEED
        assert all(m.status == -5 for m in r.members)


def test_portfolio_one_is_the_plain_query(oracle_mod):
    env, s, g, ids, iters = RC.queries(oracle_mod, "push16")
    pi, orc = RC.scene_of(oracle_mod, env)
    for q in (0, 1, 9, 12):
        r = R.race(orc, s[q], g[q], pi.spec.range, 1, iters, RC.MAX_NODES, RC.MAX_PATH, RC.SEED, int(ids[q]))
        st, rows, chk, it = orc.plan(s[q], g[q], pi.spec.range, 0.005, max_iters=iters, max_nodes=RC.MAX_NODES, seed=RC.SEED, env_id=int(ids[q]),
                                     max_path=RC.MAX_PATH)
        assert r.status == st and r.n_checks == chk and np.array_equal(_bits(r.rows), _bits(rows))
        assert r.winner == (0 if st == 0 else -1) and r.win_seed == RC.SEED
