"""Sequential reference of K9's shortcutPath (csrc/mopa_k9.inc, DESIGN.md "K9 path simplification: shortcutPath") for
test_shortcut_host.py and test_shortcut_gpu.py: OMPL's PathSimplifier::shortcutPath restated over `OracleScene.check_motion`,
in front of simplify_ref.py's reduceVertices / collapseCloseVertices, which run unchanged on the vertex list.  shortcutPath
creates new floating-point states, so every operation is fixed here: plain float64 adds, subtractions, one product or one
division where named, and a correctly rounded fma in `interpolate` only.  This form is the definition: the kernel has to
reproduce it exactly."""
import ctypes
import ctypes.util
import math

import numpy as np

from reuse_ref import M64, rng_uniform_k
from simplify_ref import DRAW_BASE, Simplifier, dist, so2_flags

RANGE_RATIO = 0.33
SNAP_TO_VERTEX = 0.005
INFO_COLS = 6        # motion checks, draws, rounds, accepted shortcut splices, capacity skips, largest vertex count reached

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double]


def fma(a, b, c):
    return float(_libm.fma(float(a), float(b), float(c)))


def interpolate(a, b, t, so2):
    """`interp_dim` of the library / the oracle's `interpolate` per active coordinate.  -> (values, whether an SO(2) coordinate
    took the way across the seam)"""
    out, wrapped = [], False
    for x, y, w in zip(a, b, so2):
        x, y = float(x), float(y)
        diff = y - x
        if not w or abs(diff) <= math.pi:
            out.append(fma(diff, t, x))
            continue
        wrapped = True
        diff = 2.0 * math.pi - diff if diff > 0.0 else -2.0 * math.pi - diff
        v = fma(-diff, t, x)
        if v > math.pi:
            v -= 2.0 * math.pi
        elif v < -math.pi:
            v += 2.0 * math.pi
        out.append(v)
    return out, wrapped


class ShortcutSimplifier(Simplifier):
    """One path.  `rows` grows by the states shortcutPath creates; `idx` (the vertex list of simplify_ref.Simplifier) holds indices
    into it, so reduceVertices and collapseCloseVertices of the base class work on the current vertices as they are."""

    def __init__(self, orc, rows, seed, stream_id, resolution=0.005, so2=None, max_path=None):
        super().__init__(orc, rows, seed, stream_id, resolution, so2)
        self.max_path = int(max_path) if max_path is not None else 1 << 30
        self.rounds = 0
        self.n_splices = 0
        self.n_cap_skips = 0
        self.max_count = len(self.idx)
        self.events.update({"vv": 0, "vi": 0, "iv": 0, "ii": 0, "grow": 0, "fail_ab": 0, "fail_stub": 0, "same_segment": 0,
                            "cap_skip": 0, "seam_row": 0})
        self.new_rows = []          # (index into rows, crossed the seam) of every state an accepted splice created

    # ---- pieces of shortcut() ----
    def _act(self, k):
        return self.rows[self.idx[k], self.act]

    def _cumulative(self):
        D = [0.0]
        for k in range(1, len(self.idx)):
            D.append(D[-1] + dist(self._act(k - 1), self._act(k), self.so2))
        return D

    def uniform_real(self, lo, hi):
        u = rng_uniform_k(self.key, (DRAW_BASE + self.n_draws) & M64)
        self.n_draws += 1
        return lo + u * (hi - lo)

    @staticmethod
    def locate(D, d, thr):
        p = len(D) - 1
        for k, v in enumerate(D):
            if v >= d:
                p = k
                break
        if p == 0 or D[p] - d < thr:
            return p, p
        while p > 0 and d < D[p]:
            p -= 1
        if d - D[p] < thr:
            return p, p
        return p, -1

    def check_points(self, a, b):
        """K2's rule between two points given by their active coordinates, `a` the earlier one along the path"""
        self.n_checks += 1
        ok, _ = self.orc.check_motion(self.rows[0], np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), self.res)
        return ok

    def _append_row(self, act_values):
        row = self.rows[0].copy()                 # row 0's passive entries
        row[self.act] = act_values
        self.rows = np.vstack([self.rows, row[None]])
        return len(self.rows) - 1

    def shortcut(self):
        n = len(self.idx)
        if n < 3:
            return False
        self._set_distances()
        if self.D[-1] == 0.0:
            return False
        result = False
        nochange = 0
        i = 0
        while i < n and nochange < n:
            if self._shortcut_step():
                nochange = 0
                result = True
            i += 1
            nochange += 1
        return result

    def _set_distances(self):
        self.D = self._cumulative()
        self.thr, self.rd = self.D[-1] * SNAP_TO_VERTEX, RANGE_RATIO * self.D[-1]

    def _shortcut_step(self):
        """one iteration of shortcut(): True iff a splice was accepted"""
        D, thr, rd = self.D, self.thr, self.rd
        d0 = self.uniform_real(0.0, D[-1])
        p0, x0 = self.locate(D, d0, thr)
        d1 = self.uniform_real(max(0.0, d0 - rd), min(d0 + rd, D[-1]))
        p1, x1 = self.locate(D, d1, thr)
        if (p0 == p1 or x0 == p1 or x1 == p0 or p0 + 1 == x1 or p1 + 1 == x0
                or (x0 >= 0 and x1 >= 0 and abs(x0 - x1) < 2)):
            self.events["same_segment"] += 1
            return False
        if p0 > p1:
            d0, d1, p0, p1, x0, x1 = d1, d0, p1, p0, x1, x0
        count = len(self.idx)
        if x0 < 0 and x1 < 0 and p0 + 1 == p1 and count == self.max_path:
            self.n_cap_skips += 1
            self.events["cap_skip"] += 1
            return False
        wa = wb = False
        if x0 < 0:
            t0 = (d0 - D[p0]) / (D[p0 + 1] - D[p0])
            A, wa = interpolate(self._act(p0), self._act(p0 + 1), t0, self.so2)
        else:
            A = list(self._act(x0))
        if x1 < 0:
            t1 = (d1 - D[p1]) / (D[p1 + 1] - D[p1])
            B, wb = interpolate(self._act(p1), self._act(p1 + 1), t1, self.so2)
        else:
            B = list(self._act(x1))
        if not self.check_points(A, B):
            self.events["fail_ab"] += 1
            return False
        if x0 < 0 and not self.check_points(self._act(p0), A):
            self.events["fail_stub"] += 1
            return False
        if x1 < 0 and not self.check_points(B, self._act(p1 + 1)):
            self.events["fail_stub"] += 1
            return False
        prefix = self.idx[:(x0 if x0 >= 0 else p0) + 1]
        suffix = self.idx[(x1 if x1 >= 0 else p1 + 1):]
        new = []
        for x, pt, w in ((x0, A, wa), (x1, B, wb)):
            if x < 0:
                r = self._append_row(pt)
                new.append(r)
                self.new_rows.append((r, w))
                self.events["seam_row"] += int(w)
        self.idx = prefix + new + suffix
        assert len(self.idx) <= self.max_path
        self.events[("v" if x0 >= 0 else "i") + ("v" if x1 >= 0 else "i")] += 1
        self.events["grow"] += int(len(self.idx) > count)
        self.max_count = max(self.max_count, len(self.idx))
        self.n_splices += 1
        self._set_distances()
        return True

    def run(self, passes=7, max_rounds=16):
        reduce = self.reduce_vertices if passes & 1 else (lambda: False)
        collapse = self.collapse_close_vertices if passes & 2 else (lambda: False)
        try_more = True
        while try_more and self.rounds < max_rounds:
            self.rounds += 1
            if passes & 4:
                times = 0
                while True:
                    m = self.shortcut()
                    times += 1
                    if not (times <= 5 and m):
                        break
            try_more = reduce()
            collapse()
            times = 0
            while try_more and times < 5:
                try_more = reduce()
                times += 1
        return self.idx

    def result_rows(self):
        return self.rows[self.idx]

    def info(self):
        return (self.n_checks, self.n_draws, self.rounds, self.n_splices, self.n_cap_skips, self.max_count)


def path_length(orc, rows, so2=None):
    """L1 length over the active coordinates (SO(2) the short way round)"""
    act = np.asarray(orc.active_idx)
    so2 = so2 if so2 is not None else so2_flags(orc.model, orc.active_idx)
    return sum(dist(rows[k, act], rows[k + 1, act], so2) for k in range(len(rows) - 1))


def shortcut_batch(orc, path, path_len, status=None, seed=0, env_id_base=0, env_ids=None, seeds=None, passes=7, max_rounds=16,
                   resolution=0.005):
    """the batch form of `BatchPlanner.shortcut_paths` on numpy arrays; returns (path', path_len', info [E, 6], simplifier per path
    or None).  Skipped paths (status != 0, path_len < 3, path_len > max_path) come back unchanged with info 0; rows at and beyond
    a new length keep what they held (the device leaves them unspecified: compare the first path_len' rows only)."""
    path = np.array(path, dtype=np.float64, copy=True)
    plen = np.array(path_len, dtype=np.int32, copy=True)
    E, max_path = len(plen), path.shape[1]
    info = np.zeros((E, INFO_COLS), dtype=np.int64)
    runs = [None] * E
    so2 = so2_flags(orc.model, orc.active_idx)
    for e in range(E):
        if (status is not None and int(status[e]) != 0) or plen[e] < 3 or plen[e] > max_path:
            continue
        sid = int(env_ids[e]) if env_ids is not None else int(env_id_base) + e
        sd = int(seeds[e]) if seeds is not None else int(seed)
        s = ShortcutSimplifier(orc, path[e, :plen[e]], sd, sid, resolution, so2, max_path)
        s.run(passes, max_rounds)
        out = s.result_rows()
        path[e, :len(out)] = out
        plen[e] = len(out)
        info[e] = s.info()
        runs[e] = s
    return path, plen, info, runs
