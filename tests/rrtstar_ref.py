"""Sequential reference of K3b (csrc/mopa_rrtstar.inc, DESIGN.md "K3b RRT*") for test_star_host.py and test_star_gpu.py: OMPL's
RRT* as the reference configures it (k-nearest, path-length objective, no cost threshold) restated over `OracleScene.is_valid` /
`check_motion`, with reuse_ref.py's counter RNG, simplify_ref.py's distance and shortcut_ref.py's fma / interpolate.  Every
floating-point operation is fixed here: plain float64 adds in the stated order, one division (range / d), interpolate's fma, and
the sample's fma.  This form is the definition: the kernel has to reproduce it exactly -- path rows, cost and counters."""
import math

import numpy as np

from reuse_ref import M64, rng_key, rng_uniform_k
from shortcut_ref import fma, interpolate
from simplify_ref import dist, so2_flags

E_CONST = 2.718281828459045
REWIRE_FACTOR = 1.1
K_MAX = 64                  # one lane per neighbour
INFO_COLS = 8               # iterations run, nodes, motion checks, rewires, goal nodes, first goal iteration, descendant updates, full iterations
PLAN_OK, PLAN_NO_EXACT, PLAN_INVALID_GOAL = 0, -4, -5


def k_rrt(na, rewire_factor=REWIRE_FACTOR):
    return rewire_factor * (E_CONST + E_CONST / na)


def k_of(na, n, rewire_factor=REWIRE_FACTOR):
    """neighbours asked for when the tree holds n nodes"""
    return int(math.ceil(k_rrt(na, rewire_factor) * math.log(n + 1)))


def sample_bounds(model, active_idx):
    """per active coordinate (lo, hi) of the uniform sample: +-pi on an SO(2) coordinate, otherwise the joint range"""
    lo, hi = [], []
    for adr, w in zip(active_idx, so2_flags(model, active_idx)):
        j = [k for k in range(len(model.jnt_type)) if int(model.jnt_qposadr[k]) == int(adr)][0]
        lo.append(-math.pi if w else float(model.jnt_range[j][0]))
        hi.append(math.pi if w else float(model.jnt_range[j][1]))
    return lo, hi


class StarResult:
    def __init__(self, status, rows, cost, info, events, tree):
        self.status, self.rows, self.cost, self.info, self.events, self.tree = status, rows, cost, info, events, tree


def _dists(Q, n, p, so2):
    """dist(Q[i], p) for i < n: the adds of simplify_ref.dist, coordinate by coordinate over all nodes at once"""
    d = np.zeros(n)
    for a, w in enumerate(so2):
        t = np.abs(Q[:n, a] - float(p[a]))
        if w:
            t = np.where(t > math.pi, 2.0 * math.pi - t, t)
        d = d + t
    return d


def plan_star(orc, start, goal, range_, max_iters, max_nodes=None, max_path=256, seed=0, stream_id=0, goal_bias=0.05,
              goal_threshold=0.0, rewire_factor=REWIRE_FACTOR, resolution=0.005, so2=None, bounds=None):
    """One query.  `start` / `goal`: full qpos rows; the passive entries of `start` are the env row of every check."""
    row = np.asarray(start, dtype=np.float64)
    act = np.asarray(orc.active_idx, dtype=np.int64)
    na = len(act)
    so2 = so2 if so2 is not None else so2_flags(orc.model, orc.active_idx)
    lo, hi = bounds if bounds is not None else sample_bounds(orc.model, orc.active_idx)
    max_nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)
    if k_of(na, max_nodes, rewire_factor) > K_MAX:
        raise ValueError("k(max_nodes) > 64")
    qs, qg = row[act].copy(), np.asarray(goal, dtype=np.float64)[act].copy()
    ev = {"trapped": 0, "rewire": 0, "desc": 0, "parent_not_nearest": 0, "reused_fail": 0, "nearest_outside": 0, "goal_nodes": 0,
          "full": 0, "checks": 0, "parent_checks": 0, "rewire_checks": 0}
    info = np.zeros(INFO_COLS, dtype=np.int64)
    info[5] = -1

    def state_valid(q):
        s = row.copy()
        s[act] = q
        return bool(orc.is_valid(s)[0])

    def motion(a, b):
        ev["checks"] += 1
        return bool(orc.check_motion(row, np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), resolution)[0])

    if not state_valid(qg):
        return StarResult(PLAN_INVALID_GOAL, np.zeros((0, len(row))), math.inf, info, ev, None)
    if not state_valid(qs):
        return StarResult(PLAN_NO_EXACT, np.zeros((0, len(row))), math.inf, info, ev, None)
    Q = np.zeros((max_nodes, na))
    parent = np.full(max_nodes, -1, dtype=np.int64)
    inc = np.zeros(max_nodes)
    cost = np.zeros(max_nodes)
    Q[0] = qs
    n = 1
    goals = []
    key = rng_key(int(seed) & M64, int(stream_id) & M64)
    first_goal = -1
    for it in range(int(max_iters)):
        u = rng_uniform_k(key, it * (na + 1))
        if not goals and u < goal_bias:
            r = qg.copy()
        else:
            r = np.array([fma(hi[a] - lo[a], rng_uniform_k(key, it * (na + 1) + 1 + a), lo[a]) for a in range(na)])
        dn = _dists(Q, n, r, so2)
        nm = int(np.argmin(dn))                       # (first minimum: lowest index)
        d = float(dn[nm])
        x = np.array(interpolate(Q[nm], r, range_ / d, so2)[0]) if d > range_ else r
        if n >= max_nodes:
            ev["full"] += 1
            continue
        if not motion(Q[nm], x):
            ev["trapped"] += 1
            continue
        dx = _dists(Q, n, x, so2)
        kk = min(k_of(na, n, rewire_factor), n)
        nbh = [int(i) for i in np.argsort(dx, kind="stable")[:kk]]        # ascending (dist, index)
        ninc = [float(dx[i]) for i in nbh]
        c = [float(cost[i]) + ninc[s] for s, i in enumerate(nbh)]
        verdict = [0] * kk
        par, pinc = nm, dist(Q[nm], x, so2)
        pcost = float(cost[nm]) + pinc
        if nm not in nbh:
            ev["nearest_outside"] += 1
        for s in sorted(range(kk), key=lambda s: (c[s], s)):
            if nbh[s] == nm:
                ok = True
            else:
                ev["parent_checks"] += 1
                ok = motion(Q[nbh[s]], x)
            if ok:
                verdict[s] = 1
                par, pinc, pcost = nbh[s], ninc[s], c[s]
                break
            verdict[s] = -1
        if par != nm:
            ev["parent_not_nearest"] += 1
        Q[n], parent[n], inc[n], cost[n] = x, par, pinc, pcost
        for s, i in enumerate(nbh):
            if i == par:
                continue
            nc = float(cost[n]) + ninc[s]
            if not nc < float(cost[i]):
                continue
            if verdict[s] == 1:
                ok = True
            elif verdict[s] == -1:
                ok = False
                ev["reused_fail"] += 1
            else:
                ev["rewire_checks"] += 1
                ok = motion(x, Q[i])
            if not ok:
                continue
            parent[i], inc[i], cost[i] = n, ninc[s], nc
            ev["rewire"] += 1
            # every descendant of i, top down
            done = {i}
            changed = True
            while changed:
                changed = False
                for cnode in range(n + 1):
                    if cnode not in done and int(parent[cnode]) in done:
                        cost[cnode] = cost[parent[cnode]] + inc[cnode]
                        done.add(cnode)
                        ev["desc"] += 1
                        changed = True
        if dist(x, qg, so2) <= goal_threshold:
            goals.append(n)
            if first_goal < 0:
                first_goal = it
        n += 1
    ev["goal_nodes"] = len(goals)
    info[:] = (max_iters, n, ev["checks"], ev["rewire"], len(goals), first_goal, ev["desc"], ev["full"])
    tree = (Q[:n].copy(), parent[:n].copy(), inc[:n].copy(), cost[:n].copy(), list(goals))
    if not goals:
        return StarResult(PLAN_NO_EXACT, np.zeros((0, len(row))), math.inf, info, ev, tree)
    best = goals[0]
    for g in goals[1:]:
        if cost[g] < cost[best]:
            best = g
    chain = []
    t = best
    while t >= 0:
        chain.append(t)
        t = int(parent[t])
    chain.reverse()
    if len(chain) > max_path:
        return StarResult(PLAN_NO_EXACT, np.zeros((0, len(row))), math.inf, info, ev, tree)
    rows = np.repeat(row[None], len(chain), axis=0)
    rows[:, act] = Q[chain]
    ev["chain"] = chain
    return StarResult(PLAN_OK, rows, float(cost[best]), info, ev, tree)


def plan_star_batch(orc, start, goal, range_, max_iters, max_nodes=None, max_path=256, seed=0, env_id_base=0, env_ids=None, seeds=None,
                    **kw):
    """the batch form of `BatchPlanner.plan_star` on numpy arrays -> (path [E, max_path, nq], path_len [E] int32, status [E] int32,
    cost [E], info [E, 8] int64, results).  Rows at and beyond path_len are zero here and unspecified on the device."""
    E, nq = len(start), np.asarray(start).shape[1]
    path = np.zeros((E, max_path, nq))
    plen = np.zeros(E, dtype=np.int32)
    status = np.zeros(E, dtype=np.int32)
    cost = np.full(E, math.inf)
    info = np.zeros((E, INFO_COLS), dtype=np.int64)
    so2 = so2_flags(orc.model, orc.active_idx)
    bounds = sample_bounds(orc.model, orc.active_idx)
    res = []
    for e in range(E):
        sid = int(env_ids[e]) if env_ids is not None else int(env_id_base) + e
        sd = int(seeds[e]) if seeds is not None else int(seed)
        r = plan_star(orc, start[e], goal[e], range_, max_iters, max_nodes, max_path, sd, sid, so2=so2, bounds=bounds, **kw)
        status[e], cost[e], info[e] = r.status, r.cost, r.info
        plen[e] = len(r.rows)
        path[e, :len(r.rows)] = r.rows
        res.append(r)
    return path, plen, status, cost, info, res
