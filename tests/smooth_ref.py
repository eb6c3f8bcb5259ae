"""Sequential reference of K9's smoothBSpline (csrc/mopa_k9.inc, DESIGN.md "K9 path simplification: smoothBSpline") for
test_smooth_host.py and test_smooth_gpu.py: OMPL's PathSimplifier::smoothBSpline restated over `OracleScene.check_motion` and
`OracleScene.is_valid_batch`, between shortcut_ref.py's shortcutPath loop and the vertex passes of a round.  Every new state is
made by `interpolate` (one fma per coordinate); the pass draws nothing.  Three deviations from OMPL keep every segment of a
result one that has itself passed checkMotion in path direction: a vertex moves only if the outer halves of its two
neighbouring segments pass, a step that moves nothing is undone, and a midpoint between two unmoved vertices stays only if both
its halves pass.  This form is the definition: the kernel has to reproduce it exactly."""
import numpy as np

from shortcut_ref import ShortcutSimplifier, interpolate
from simplify_ref import dist, so2_flags

MAX_STEPS = 3
INFO_COLS = 10       # shortcut_ref's six, then: smoothing steps subdivided, vertices moved, idle midpoints dropped, state checks


class SmoothSimplifier(ShortcutSimplifier):
    """One path.  `rows` grows by the midpoints of a subdivision and by the moved forms of vertices (a moved vertex keeps its own
    row's passive entries); `idx` holds indices into it."""

    def __init__(self, orc, rows, seed, stream_id, resolution=0.005, so2=None, max_path=None):
        super().__init__(orc, rows, seed, stream_id, resolution, so2, max_path)
        self.n_steps = 0
        self.n_moved = 0
        self.n_dropped = 0
        self.n_state_checks = 0
        self.events.update({"moved": 0, "below_min": 0, "fail_first": 0, "fail_second": 0, "invalid_mid": 0, "outer_fail": 0,
                            "mid_kept": 0, "mid_dropped": 0, "seam_eval": 0, "no_move": 0, "smooth_cap": 0})

    def is_valid(self, act_values):
        """the state check the motion check uses, against env row 0"""
        self.n_state_checks += 1
        v, _ = self.orc.is_valid_batch(np.asarray(act_values, dtype=np.float64)[None], self.rows[0][None], want_min_dist=False)
        return bool(v[0])

    def _interp(self, a, b):
        out, wrapped = interpolate(a, b, 0.5, self.so2)
        self.events["seam_eval"] += int(wrapped)
        return out

    def _segments_pass(self, idx):
        return all(self.orc.check_motion(self.rows[0], self.rows[idx[k], self.act], self.rows[idx[k + 1], self.act], self.res)[0]
                   for k in range(len(idx) - 1))

    def smooth(self):
        if len(self.idx) < 3:
            return
        min_change = self._cumulative()[-1] / 100.0
        for _ in range(MAX_STEPS):
            if not self._smooth_step(min_change):
                return

    def _smooth_step(self, min_change):
        """one step of smooth(): False iff the smoothing ends with it"""
        P = list(self.idx)
        cnt = len(P)
        if 2 * cnt - 1 > self.max_path:
            self.n_cap_skips += 1
            self.events["smooth_cap"] += 1
            return False
        checked_before = self._segments_pass(P)
        # subdivide
        Q = []
        for k in range(cnt - 1):
            Q.append(P[k])
            Q.append(self._append_row(self._interp(self.rows[P[k], self.act], self.rows[P[k + 1], self.act])))
        Q.append(P[-1])
        n = len(Q)
        self.n_steps += 1
        self.max_count = max(self.max_count, n)
        verdict = [None] * (n - 1)          # of segment (Q[k], Q[k + 1]) as it stands
        moved = [False] * n
        act = lambda k: self.rows[Q[k], self.act]

        def seg(k):
            if verdict[k] is None:
                verdict[k] = self.check_points(act(k), act(k + 1))
            return verdict[k]

        u = 0
        for i in range(2, n - 1, 2):
            if not self.is_valid(act(i - 1)):
                self.events["invalid_mid"] += 1
                continue
            t1 = self._interp(act(i - 1), act(i))
            t2 = self._interp(act(i), act(i + 1))
            t = self._interp(t1, t2)
            if not self.check_points(act(i - 1), t):
                self.events["fail_first"] += 1
                continue
            if not self.check_points(t, act(i + 1)):
                self.events["fail_second"] += 1
                continue
            if not dist(act(i), t, self.so2) > min_change:
                self.events["below_min"] += 1
                continue
            if not (seg(i - 2) and seg(i + 1)):
                self.events["outer_fail"] += 1
                continue
            row = self.rows[Q[i]].copy()          # the vertex's own row, its active entries overwritten
            row[self.act] = t
            self.rows = np.vstack([self.rows, row[None]])
            Q[i] = len(self.rows) - 1
            moved[i] = True
            verdict[i - 1] = verdict[i] = True          # their new forms are the two checks just made
            u += 1
        if u == 0:
            self.events["no_move"] += 1
            return False                      # self.idx is P still: the subdivision is dropped
        self.n_moved += u
        self.events["moved"] += u
        out = []
        for k in range(cnt - 1):
            out.append(Q[2 * k])
            if moved[2 * k] or moved[2 * k + 2] or (seg(2 * k) and seg(2 * k + 1)):
                out.append(Q[2 * k + 1])
                self.events["mid_kept"] += int(not (moved[2 * k] or moved[2 * k + 2]))
            else:
                self.n_dropped += 1
                self.events["mid_dropped"] += 1
        out.append(Q[-1])
        self.idx = out
        assert out[0] == P[0] and out[-1] == P[-1], "an endpoint moved"
        assert not checked_before or self._segments_pass(out), "a step left a segment that does not pass checkMotion"
        return True

    def run(self, passes=15, max_rounds=16):
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
            if passes & 8:
                self.smooth()
            try_more = reduce()
            collapse()
            times = 0
            while try_more and times < 5:
                try_more = reduce()
                times += 1
        return self.idx

    def info(self):
        return super().info() + (self.n_steps, self.n_moved, self.n_dropped, self.n_state_checks)


def smooth_batch(orc, path, path_len, status=None, seed=0, env_id_base=0, env_ids=None, seeds=None, passes=15, max_rounds=16,
                 resolution=0.005):
    """the batch form of `BatchPlanner.smooth_paths` on numpy arrays; returns (path', path_len', info [E, 10], simplifier per path
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
        s = SmoothSimplifier(orc, path[e, :plen[e]], sd, sid, resolution, so2, max_path)
        s.run(passes, max_rounds)
        out = s.result_rows()
        path[e, :len(out)] = out
        plen[e] = len(out)
        info[e] = s.info()
        runs[e] = s
    return path, plen, info, runs
