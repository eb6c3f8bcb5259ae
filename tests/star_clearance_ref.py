"""Sequential reference of K3b under the clearance objective (csrc/mopa_rrtstar_clear.inc, DESIGN.md section 4 "K3b under the
clearance objective") for test_star_clearance_host.py and test_star_clearance_gpu.py.  It composes, unchanged, rrtstar_ref.py's
draws, `_dists`, `k_of` and `sample_bounds`, shortcut_ref.interpolate, simplify_ref.dist, and motion_clearance_ref's
`state_clearances` / `motion_clearance`.  This form is the definition: the kernel reproduces it bit for bit.

thr = the scene's contact threshold, band finite, >= 0 and > thr.  sc(q) = the band-saturated clearance of one state on the start
row; mc(a -> b) = motion_clearance's `clearance` of the segment (states s_1 .. s_c, a not evaluated).  A motion is valid iff
mc > thr, which is asserted equal to `orc.check_motion` on every motion evaluated.  A chain's key is (C, L) = (its clearance, its
L1 length); better((C1, L1), (C2, L2)) = C1 > C2 or (C1 == C2 and L1 < L2).  Everything not restated below is rrtstar_ref.plan_star
word for word: entry checks, draws, nearest, steering, the full-tree rule, k(n), the goal rule and the goal-bias rule.

info, 11 columns: iterations run, nodes, motion-clearance evaluations, rewires, goal nodes, first goal iteration, descendant
updates, full iterations, parent-walk evaluations, rewire evaluations, rewires that strictly raised C."""
import math

import numpy as np

import motion_clearance_ref as MC
from reuse_ref import M64, rng_key, rng_uniform_k
from rrtstar_ref import K_MAX, PLAN_INVALID_GOAL, PLAN_NO_EXACT, PLAN_OK, REWIRE_FACTOR, _dists, k_of, sample_bounds
from shortcut_ref import fma, interpolate
from simplify_ref import dist, so2_flags

INFO_COLS = 11


def better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


class ClearResult:
    def __init__(self, status, rows, clearance, length, info, events, tree):
        self.status, self.rows, self.clearance, self.length = status, rows, clearance, length
        self.info, self.events, self.tree = info, events, tree


def plan_star_clearance(pi, orc, start, goal, range_, band, max_iters, max_nodes=None, max_path=256, seed=0, stream_id=0, goal_bias=0.05,
                        goal_threshold=0.0, rewire_factor=REWIRE_FACTOR, resolution=0.005, so2=None, bounds=None):
    """One query.  `start` / `goal`: full qpos rows; the passive entries of `start` are the env row of every evaluation."""
    row = np.asarray(start, dtype=np.float64)
    act = np.asarray(orc.active_idx, dtype=np.int64)
    na = len(act)
    thr = float(pi.spec.contact_threshold)
    band = float(band)
    if not (math.isfinite(band) and band >= 0.0 and band > thr):
        raise ValueError("band must be finite, >= 0 and above the contact threshold")
    so2 = so2 if so2 is not None else so2_flags(orc.model, orc.active_idx)
    lo, hi = bounds if bounds is not None else sample_bounds(orc.model, orc.active_idx)
    max_nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)
    if k_of(na, max_nodes, rewire_factor) > K_MAX:
        raise ValueError("k(max_nodes) > 64")
    qs, qg = row[act].copy(), np.asarray(goal, dtype=np.float64)[act].copy()
    ev = {"trapped": 0, "rewire": 0, "desc": 0, "goal_nodes": 0, "full": 0, "evals": 0, "parent_evals": 0, "rewire_evals": 0,
          "parent_not_path_length": 0, "parent_not_nearest": 0, "bound_cut": 0, "rewire_raise": 0, "rewire_shorten": 0, "unsaturated": 0,
          "states": 0, "best_goal_not_earliest": 0, "pairs": set()}
    info = np.zeros(INFO_COLS, dtype=np.int64)
    info[5] = -1

    def state_valid(q):
        s = row.copy()
        s[act] = q
        return bool(orc.is_valid(s)[0])

    def mc(a, b):
        ev["evals"] += 1
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        rep = MC.motion_clearance(pi, orc, a[None], b[None], row[None], band, 1, resolution)
        m = float(rep["clearance"][0])
        ev["states"] += int(rep["n_states"][0])
        ev["unsaturated"] += int(m < band)
        ev["pairs"].update(int(p) for p in rep["p"][0] if p >= 0)            # the nearest pair of every evaluated state in band
        assert (m > thr) == bool(orc.check_motion(row, a, b, resolution)[0]), "clearance > contact_threshold is not check_motion's verdict"
        return m

    def out(status, rows, c, l, tree):
        return ClearResult(status, rows, c, l, info, ev, tree)

    none = np.zeros((0, len(row)))
    if not state_valid(qg):
        return out(PLAN_INVALID_GOAL, none, -math.inf, math.inf, None)
    if not state_valid(qs):
        return out(PLAN_NO_EXACT, none, -math.inf, math.inf, None)
    Q = np.zeros((max_nodes, na))
    parent = np.full(max_nodes, -1, dtype=np.int64)
    inc = np.zeros(max_nodes)
    edge = np.full(max_nodes, math.inf)
    Cn = np.zeros(max_nodes)
    Ln = np.zeros(max_nodes)
    Q[0] = qs
    d0, p0, _ = MC.state_clearances(pi, orc, qs[None], row[None], band)
    Cn[0] = float(d0[0])
    ev["pairs"].update(int(p) for p in p0 if p >= 0)
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
        nm = int(np.argmin(dn))
        d = float(dn[nm])
        x = np.array(interpolate(Q[nm], r, range_ / d, so2)[0]) if d > range_ else r
        if n >= max_nodes:
            ev["full"] += 1
            continue
        # 4. the first evaluation: the motion check and nm's edge value
        m_nm = mc(Q[nm], x)
        if not m_nm > thr:
            ev["trapped"] += 1
            continue
        # 5. neighbours and their bounds
        dx = _dists(Q, n, x, so2)
        kk = min(k_of(na, n, rewire_factor), n)
        nbh = [int(i) for i in np.argsort(dx, kind="stable")[:kk]]
        ninc = [float(dx[i]) for i in nbh]
        ub = [(float(Cn[i]), float(Ln[i]) + ninc[s]) for s, i in enumerate(nbh)]
        # 6. parent: exact branch and bound over the bounds, best first
        pinc = dist(Q[nm], x, so2)
        best, par, pedge = (min(float(Cn[nm]), m_nm), float(Ln[nm]) + pinc), nm, m_nm
        order = sorted(range(kk), key=lambda s: (-ub[s][0], ub[s][1], s))
        for r_, s in enumerate(order):
            if nbh[s] == nm:
                continue
            if not better(ub[s], best):
                ev["bound_cut"] += int(any(nbh[t] != nm for t in order[r_:]))
                break
            ev["parent_evals"] += 1
            m = mc(Q[nbh[s]], x)
            if m > thr and better((min(ub[s][0], m), ub[s][1]), best):
                best, par, pedge, pinc = (min(ub[s][0], m), ub[s][1]), nbh[s], m, ninc[s]
        # (for the events: the parent path-length RRT* picks on this tree state, rrtstar_ref's walk with L as the cost)
        pl_par = nm
        for s in sorted(range(kk), key=lambda s: (ub[s][1], s)):
            if nbh[s] == nm or bool(orc.check_motion(row, Q[nbh[s]], x, resolution)[0]):
                pl_par = nbh[s]
                break
        ev["parent_not_path_length"] += int(par != pl_par)
        ev["parent_not_nearest"] += int(par != nm)
        # 7. append
        Q[n], parent[n], inc[n], edge[n], Cn[n], Ln[n] = x, par, pinc, pedge, best[0], best[1]
        # 8. rewire
        for s, i in enumerate(nbh):
            if i == par:
                continue
            nl = float(Ln[n]) + ninc[s]
            if not better((float(Cn[n]), nl), (float(Cn[i]), float(Ln[i]))):
                continue
            ev["rewire_evals"] += 1
            m = mc(x, Q[i])
            if not m > thr:
                continue
            nc = min(float(Cn[n]), m)
            if not better((nc, nl), (float(Cn[i]), float(Ln[i]))):
                continue
            if nc > float(Cn[i]):
                ev["rewire_raise"] += 1
            else:
                ev["rewire_shorten"] += 1
            parent[i], inc[i], edge[i], Cn[i], Ln[i] = n, ninc[s], m, nc, nl
            ev["rewire"] += 1
            done = {i}
            changed = True
            while changed:
                changed = False
                for c in range(n + 1):
                    if c not in done and int(parent[c]) in done:
                        Cn[c] = min(float(Cn[parent[c]]), float(edge[c]))
                        Ln[c] = Ln[parent[c]] + inc[c]
                        done.add(c)
                        ev["desc"] += 1
                        changed = True
        if dist(x, qg, so2) <= goal_threshold:
            goals.append(n)
            if first_goal < 0:
                first_goal = it
        n += 1
    ev["goal_nodes"] = len(goals)
    info[:] = (max_iters, n, ev["evals"], ev["rewire"], len(goals), first_goal, ev["desc"], ev["full"], ev["parent_evals"], ev["rewire_evals"],
               ev["rewire_raise"])
    tree = (Q[:n].copy(), parent[:n].copy(), inc[:n].copy(), edge[:n].copy(), Cn[:n].copy(), Ln[:n].copy(), list(goals))
    if not goals:
        return out(PLAN_NO_EXACT, none, -math.inf, math.inf, tree)
    bg = goals[0]
    for g in goals[1:]:
        if better((Cn[g], Ln[g]), (Cn[bg], Ln[bg])):
            bg = g
    ev["best_goal_not_earliest"] = int(bg != goals[0])
    chain = []
    t = bg
    while t >= 0:
        chain.append(t)
        t = int(parent[t])
    chain.reverse()
    if len(chain) > max_path:
        return out(PLAN_NO_EXACT, none, -math.inf, math.inf, tree)
    rows = np.repeat(row[None], len(chain), axis=0)
    rows[:, act] = Q[chain]
    ev["chain"] = chain
    return out(PLAN_OK, rows, float(Cn[bg]), float(Ln[bg]), tree)


def plan_star_clearance_batch(pi, orc, start, goal, range_, band, max_iters, max_nodes=None, max_path=256, seed=0, env_id_base=0, env_ids=None,
                              seeds=None, **kw):
    """the batch form of `BatchPlanner.plan_star_clearance` on numpy arrays -> (path [E, max_path, nq], path_len [E] int32, status [E]
    int32, clearance [E], length [E], info [E, 11] int64, results).  Rows at and beyond path_len are zero here, unspecified on the device."""
    E, nq = len(start), np.asarray(start).shape[1]
    path = np.zeros((E, max_path, nq))
    plen = np.zeros(E, dtype=np.int32)
    status = np.zeros(E, dtype=np.int32)
    clearance = np.full(E, -math.inf)
    length = np.full(E, math.inf)
    info = np.zeros((E, INFO_COLS), dtype=np.int64)
    so2 = so2_flags(orc.model, orc.active_idx)
    bounds = sample_bounds(orc.model, orc.active_idx)
    res = []
    for e in range(E):
        sid = int(env_ids[e]) if env_ids is not None else int(env_id_base) + e
        sd = int(seeds[e]) if seeds is not None else int(seed)
        r = plan_star_clearance(pi, orc, start[e], goal[e], range_, band, max_iters, max_nodes, max_path, sd, sid, so2=so2, bounds=bounds, **kw)
        status[e], clearance[e], length[e], info[e] = r.status, r.clearance, r.length, r.info
        plen[e] = len(r.rows)
        path[e, :len(r.rows)] = r.rows
        res.append(r)
    return path, plen, status, clearance, length, info, res
