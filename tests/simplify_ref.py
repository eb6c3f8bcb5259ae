"""Sequential reference of K9 (csrc/mopa_k9.inc, DESIGN.md "K9 path simplification") for test_simplify_host.py and
test_simplify_gpu.py: OMPL's reduceVertices and collapseCloseVertices restated over `OracleScene.check_motion`, plain float64
adds and reuse_ref.py's counter RNG.  This form is the definition: the kernel has to reproduce it exactly."""
import math

import numpy as np

from reuse_ref import M64, rng_key, rng_uniform_k

DRAW_BASE = 1 << 63        # the simplifier's counters: far above the planner's it * na + a of the same (seed, stream id)
J_HINGE = 3


def so2_flags(model, active_idx):
    """per active coordinate: an unlimited hinge (OMPL SO2StateSpace), as the scene compilers decide it"""
    out = []
    for adr in active_idx:
        j = [k for k in range(len(model.jnt_type)) if int(model.jnt_qposadr[k]) == int(adr)]
        out.append(bool(j) and int(model.jnt_type[j[0]]) == J_HINGE and not bool(model.jnt_limited[j[0]]))
    return out


def dist(a, b, so2):
    """sum over the active coordinates, ascending, from 0.0, of |x - y| (the short way round on an SO(2) coordinate)"""
    d = 0.0
    for x, y, w in zip(a, b, so2):
        t = abs(float(x) - float(y))
        if w and t > math.pi:
            t = 2.0 * math.pi - t
        d += t
    return d


class Simplifier:
    """One path.  `rows` [n, nq] full qpos vectors; `events` counts what happened (the host test's coverage conditions)."""

    def __init__(self, orc, rows, seed, stream_id, resolution=0.005, so2=None):
        self.orc = orc
        self.rows = np.asarray(rows, dtype=np.float64)
        self.act = np.asarray(orc.active_idx, dtype=np.int64)
        self.so2 = so2 if so2 is not None else so2_flags(orc.model, orc.active_idx)
        self.res = resolution
        self.key = rng_key(int(seed) & M64, int(stream_id) & M64)
        self.idx = list(range(len(self.rows)))        # surviving ORIGINAL row indices
        self.n_checks = 0
        self.n_draws = 0
        self.events = {"first_check": 0, "splice": 0, "skip": 0, "collapse_removal": 0, "collapse_block": 0}
        self.trace = []            # (original row i, original row j, verdict) of every motion check, in order

    def check_motion(self, i, j):
        """K2's rule between survivors i and j; the env row is path row 0"""
        self.n_checks += 1
        ok, _ = self.orc.check_motion(self.rows[0], self.rows[self.idx[i], self.act], self.rows[self.idx[j], self.act], self.res)
        self.trace.append((self.idx[i], self.idx[j], ok))
        return ok

    def uniform_int(self, lo, hi):
        m = hi - lo + 1
        u = rng_uniform_k(self.key, (DRAW_BASE + self.n_draws) & M64)
        self.n_draws += 1
        return lo + min(int(u * m), m - 1)

    def reduce_vertices(self):
        n = len(self.idx)
        if n < 3:
            return False
        if self.check_motion(0, n - 1):
            self.idx = [self.idx[0], self.idx[-1]]
            self.events["first_check"] += 1
            return True
        result = False
        nochange = 0
        i = 0
        while i < n and nochange < n:
            count = len(self.idx)
            max_n = count - 1
            rng = 1 + (33 * count + 50) // 100
            p1 = self.uniform_int(0, max_n)
            p2 = self.uniform_int(max(p1 - rng, 0), min(max_n, p1 + rng))
            skip = False
            if abs(p1 - p2) < 2:
                if p1 < max_n - 1:
                    p2 = p1 + 2
                elif p1 > 1:
                    p2 = p1 - 2
                else:
                    skip = True
                    self.events["skip"] += 1
            if not skip:
                if p1 > p2:
                    p1, p2 = p2, p1
                if self.check_motion(p1, p2):
                    del self.idx[p1 + 1:p2]
                    nochange = 0
                    result = True
                    self.events["splice"] += 1
            i += 1
            nochange += 1
        return result

    def collapse_close_vertices(self):
        n = len(self.idx)
        if n < 3:
            return False
        blocked = set()
        result = False
        nochange = 0
        s = 0
        while s < n and nochange < n:
            best, bi, bj = math.inf, -1, -1
            for i in range(len(self.idx)):
                for j in range(i + 2, len(self.idx)):
                    if (self.idx[i], self.idx[j]) in blocked:
                        continue
                    d = dist(self.rows[self.idx[i], self.act], self.rows[self.idx[j], self.act], self.so2)
                    if d < best:
                        best, bi, bj = d, i, j
            if bi < 0:
                break
            if self.check_motion(bi, bj):
                del self.idx[bi + 1:bj]
                nochange = 0
                result = True
                self.events["collapse_removal"] += 1
            else:
                blocked.add((self.idx[bi], self.idx[bj]))
                self.events["collapse_block"] += 1
            s += 1
            nochange += 1
        return result

    def run(self, passes=3):
        reduce = self.reduce_vertices if passes & 1 else (lambda: False)
        collapse = self.collapse_close_vertices if passes & 2 else (lambda: False)
        try_more = True
        while try_more:
            try_more = reduce()
            collapse()
            times = 0
            while try_more and times < 5:
                try_more = reduce()
                times += 1
        return self.idx


def simplify_path(orc, rows, seed, stream_id, passes=3, resolution=0.005, so2=None):
    """-> (surviving original row indices, motion checks made, draws consumed, events)"""
    s = Simplifier(orc, rows, seed, stream_id, resolution, so2)
    s.run(passes)
    return list(s.idx), s.n_checks, s.n_draws, s.events


def simplify_batch(orc, path, path_len, status=None, seed=0, env_id_base=0, env_ids=None, seeds=None, passes=3, resolution=0.005):
    """the batch form of `BatchPlanner.simplify_paths` on numpy arrays; returns (path', path_len', info [E, 2], events per path).
    Skipped paths (status != 0, path_len < 3) come back unchanged with info 0; rows at and beyond a new length keep what they held
    (the device leaves them unspecified: compare the first path_len' rows only)."""
    path = np.array(path, dtype=np.float64, copy=True)
    plen = np.array(path_len, dtype=np.int32, copy=True)
    E = len(plen)
    info = np.zeros((E, 2), dtype=np.int64)
    events = [None] * E
    so2 = so2_flags(orc.model, orc.active_idx)
    for e in range(E):
        if (status is not None and int(status[e]) != 0) or plen[e] < 3:
            continue
        sid = int(env_ids[e]) if env_ids is not None else int(env_id_base) + e
        sd = int(seeds[e]) if seeds is not None else int(seed)
        keep, nc, nd, ev = simplify_path(orc, path[e, :plen[e]], sd, sid, passes, resolution, so2)
        path[e, :len(keep)] = path[e, keep]
        plen[e] = len(keep)
        info[e] = (nc, nd)
        events[e] = ev
    return path, plen, info, events


def out_and_back(q0, q1, n, act, base_row):
    """a synthetic path in free space: n rows from q0 to q1 (active coordinates, linear), then back towards q0 over n rows
    without touching it again, so that non-adjacent rows lie close together"""
    rows = np.repeat(np.asarray(base_row, dtype=np.float64)[None], 2 * n, axis=0)
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    for k in range(n):
        rows[k, act] = q0 + (q1 - q0) * (k / (n - 1))
        rows[n + k, act] = q1 + (q0 - q1) * ((k + 0.5) / n)
    return rows
