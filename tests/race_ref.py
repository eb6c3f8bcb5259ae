"""The sequential form of the portfolio RRT-Connect race (`plan_race`, DESIGN.md "K3 race") over the CPU oracle's `plan`, unchanged.

Member m of a query runs the plain query's stream id with the seed (seed + m * 0x9E3779B97F4A7C15) mod 2^64 and the full budget.  The
winner is the solved member (status 0: a solution that fits max_path) with the smallest (consumed checks, m); with no solved member
the status is -5 if the goal is invalid (every member agrees) and -4 otherwise, and n_checks / win_seed are member 0's."""
from collections import namedtuple

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
PLAN_OK, PLAN_NO_EXACT, PLAN_INVALID_GOAL = 0, -4, -5

Member = namedtuple("Member", "status rows n_checks iters seed")
Race = namedtuple("Race", "status rows n_checks winner win_seed iters members")


def member_seed(seed: int, m: int) -> int:
    return (int(seed) + m * GOLDEN) & MASK


def race(orc, start, goal, range_, portfolio, max_iters, max_nodes, max_path, seed, env_id) -> Race:
    members = []
    for m in range(int(portfolio)):
        s = member_seed(seed, m)
        st, rows, chk, it = orc.plan(start, goal, range_, 0.005, max_iters=max_iters, max_nodes=max_nodes, seed=s, env_id=int(env_id),
                                     max_path=max_path)
        members.append(Member(int(st), rows, int(chk), int(it), s))
    solved = [(mb.n_checks, m) for m, mb in enumerate(members) if mb.status == PLAN_OK]
    if solved:
        w = min(solved)[1]
        mb = members[w]
        return Race(PLAN_OK, mb.rows, mb.n_checks, w, mb.seed, mb.iters, members)
    m0 = members[0]
    status = PLAN_INVALID_GOAL if m0.status == PLAN_INVALID_GOAL else PLAN_NO_EXACT
    if status == PLAN_INVALID_GOAL:
        assert all(mb.status == PLAN_INVALID_GOAL for mb in members)
    return Race(status, np.zeros((0, len(np.asarray(start)))), m0.n_checks, -1, m0.seed, -1, members)


def race_batch(orc, start, goal, range_, portfolio, max_iters, max_nodes, max_path, seed=0, env_id_base=0, env_ids=None, seeds=None):
    """-> list of Race, query g on stream id env_ids[g] (or env_id_base + g) with seed seeds[g] (or seed)"""
    out = []
    for g in range(len(start)):
        out.append(race(orc, start[g], goal[g], range_, portfolio, max_iters, max_nodes, max_path,
                        int(seeds[g]) & MASK if seeds is not None else seed, int(env_ids[g]) if env_ids is not None else env_id_base + g))
    return out


def as_arrays(races, max_path, nq):
    """the outputs of BatchPlanner.plan_race(want_info=True) as numpy arrays: path, path_len, status, n_checks, winner, win_seed (int64
    bit pattern), info column 2 (winner's iterations), sum of all members' checks"""
    E = len(races)
    path = np.zeros((E, max_path, nq))
    plen = np.zeros(E, dtype=np.int32); status = np.zeros(E, dtype=np.int32); chk = np.zeros(E, dtype=np.int64)
    winner = np.zeros(E, dtype=np.int32); wseed = np.zeros(E, dtype=np.uint64); iters = np.zeros(E, dtype=np.int64)
    total = np.zeros(E, dtype=np.int64)
    for g, r in enumerate(races):
        plen[g] = len(r.rows); status[g] = r.status; chk[g] = r.n_checks; winner[g] = r.winner; wseed[g] = r.win_seed; iters[g] = r.iters
        path[g, :len(r.rows)] = r.rows
        total[g] = sum(mb.n_checks for mb in r.members)
    return path, plen, status, chk, winner, wseed.view(np.int64), iters, total
