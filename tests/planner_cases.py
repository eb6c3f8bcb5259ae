"""The planner queries test_random_planners_host.py and test_random_planners_gpu.py share: scenes of random_scenes.py (none of the
shipped ones), a steering range per scene, and per scene the query sets below, all on ONE env row -- the row of
random_scenes.env_rows(pi, 5, 7) on which the oracle accepts most of random_scenes.sample(pi, 1500, 13).  Valid states of that sample
are paired (0, 1), (2, 3), ... in the order of the sample.

  blocked   the first pairs whose straight line fails check_motion (the case in which the rollout plans at all); where a scene has
            fewer than N_BLOCKED of them (FREE_FILL: no_pairs has no candidate pair, and on no env row does one_active's single
            hinge reach a collision) the first pairs whose line is free fill the set
  near      the goal of a pair pulled towards its start along the (seam-aware) straight line to an L1 distance of NEAR_RANGES
            ranges, kept if it is valid: RRT* solves these and rewires
  seam      (scenes with an SO(2) coordinate, SEAM) starts whose coordinate is above 2.2 paired with goals below -2.2: the short way
            leads across the +-pi seam
  invalid   the first invalid state of the sample as a goal, and as a start

connect_set = blocked + seam + invalid goal + invalid start (RRT-Connect, the race, K9); star_set = near + seam + the two invalid
queries (RRT*).  Stream id = query index within its set, one seed per planner family.  Every reference is computed once per process
and never modified."""
import numpy as np

import race_ref
import random_scenes as RS
import rrtstar_ref
import shortcut_ref
import simplify_ref
import smooth_ref
import star_clearance_ref
from simplify_ref import so2_flags
from star_cases import VARIANT

#: key -> steering range.  The scenes' own 0.1 solves too little within a test-sized budget from 8 active coordinates on.
RANGE = {"one_active": 0.1, "serial": 0.1, "tile_posed": 0.1, "mesh": 0.1, 3: 0.6, "full": 0.3, "deep_branches": 0.3, "long_chain": 0.6,
         22: 0.3, "no_pairs": 0.1, "slab_centres": 0.6}
KEYS = list(RANGE)
RACE_KEYS = [k for k in KEYS if k not in ("one_active", "no_pairs")]          # the race / K9 set
CAPACITY_KEYS = ["full", "small_entry_cap", "slab_centres", "crowded_owner", "long_chain", "one_active", "no_pairs"]
#: key -> active index of the SO(2) coordinate the seam queries cross
SEAM = {"serial": 3, 3: 5, 22: 9, "slab_centres": 6}
FREE_FILL = ("one_active", "no_pairs")
N_BLOCKED, N_NEAR, N_SEAM, NEAR_RANGES = 6, 6, 6, 4.0

#: (max_path: the smoothing level of K9 holds 117 rows on slab_centres; the longest path of these sets has 109)
CONNECT = dict(max_iters=400, max_nodes=512, max_path=112)
CONNECT_SEED, RACE_SEED, STAR_SEED, K9_SEED = 123, 23, 7, 7
PORTFOLIO = 3
STAR_ITERS, STAR_PATH = 250, 64
#: the clearance objective: key -> queries (the first ones of the star set).  22: 10 coordinates, SO(2) at 9; mesh: two can hulls
#: on free bodies (three queries: the sequential form takes 5.5 s for four at 1 cm)
CLEAR_QUERIES = {22: 4, "mesh": 3}
CLEAR_ITERS, CLEAR_BANDS = 100, (0.0, 0.01)
#: keep_state / resume: key -> budgets of the first launch (a quarter of CONNECT's, and one below the iterations most queries need)
FIRST_ITERS = {"long_chain": (100, 16), 22: (100, 8), "one_active": (100, 0)}

_cache = {}


class World:
    def __init__(self, O, key):
        self.key = key
        self.m, self.pi = RS.scene(key)
        pi = self.pi
        self.range = RANGE.get(key, 0.1)
        self.args = (self.m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
        self.orc = O.OracleScene(*self.args)
        self.act = np.asarray(self.orc.active_idx, dtype=np.int64)
        self.na = len(self.act)
        self.so2 = so2_flags(self.m, self.orc.active_idx)
        rows = RS.env_rows(pi, 5, 7)
        qa = RS.sample(pi, 1500, 13)
        share = []
        for r in range(len(rows)):
            v, _ = self.orc.is_valid_batch(qa, rows[r:r + 1], samples_per_env=len(qa), nthreads=0, want_min_dist=False)
            share.append(v)
        r = int(np.argmax([v.mean() for v in share]))
        self.row = rows[r].copy()
        self.good, self.bad = qa[share[r] == 1], qa[share[r] == 0]

    def full(self, q):
        return RS.full_state(self.pi, q, self.row)

    def free(self, a, b):
        return bool(self.orc.check_motion(self.row, a, b)[0])

    def valid(self, q):
        return bool(self.orc.is_valid(self.full(q))[0])

    def dist(self, a, b):
        return simplify_ref.dist(a, b, self.so2)


def world(O, key):
    if ("w", key) not in _cache:
        _cache["w", key] = World(O, key)
    return _cache["w", key]


def _rows(w, pairs):
    return np.array([w.full(a) for a, _ in pairs]), np.array([w.full(b) for _, b in pairs])


def blocked(O, key):
    """-> (start [n, nq], goal [n, nq])"""
    if ("blocked", key) not in _cache:
        w = world(O, key)
        g = w.good
        pairs = [(g[k], g[k + 1]) for k in range(0, len(g) - 1, 2)]
        out = [p for p in pairs if not w.free(*p)][:N_BLOCKED]
        if key in FREE_FILL:
            out = out[:N_BLOCKED // 2]
            out += [p for p in pairs if w.free(*p)][:N_BLOCKED - len(out)]
        assert len(out) == N_BLOCKED, (key, len(out))
        _cache["blocked", key] = _rows(w, out)
    return _cache["blocked", key]


def near(O, key):
    if ("near", key) not in _cache:
        w = world(O, key)
        g = w.good
        out = []
        for k in range(0, len(g) - 1, 2):
            d = w.dist(g[k], g[k + 1])
            if d <= NEAR_RANGES * w.range:
                continue
            q = np.array(shortcut_ref.interpolate(g[k], g[k + 1], NEAR_RANGES * w.range / d, w.so2)[0])
            if w.valid(q):
                out.append((g[k], q))
            if len(out) == N_NEAR:
                break
        assert len(out) == N_NEAR, (key, len(out))
        _cache["near", key] = _rows(w, out)
    return _cache["near", key]


def seam(O, key):
    if ("seam", key) not in _cache:
        w = world(O, key)
        c = SEAM[key]
        assert w.so2[c], (key, c, w.so2)
        hi, lo = w.good[w.good[:, c] > 2.2], w.good[w.good[:, c] < -2.2]
        n = min(len(hi), len(lo), N_SEAM)
        assert n == N_SEAM, (key, len(hi), len(lo))
        _cache["seam", key] = _rows(w, list(zip(hi[:n], lo[:n])))
    return _cache["seam", key]


def _with_invalid(w, parts):
    start, goal = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if len(w.bad):
        s0, g0 = start[0].copy(), goal[0].copy()
        bad = w.full(w.bad[0])
        start, goal = np.concatenate([start, s0[None], bad[None]]), np.concatenate([goal, bad[None], g0[None]])
    return start, goal


def connect_set(O, key):
    """-> (start, goal, names [E]): blocked, seam, then (where the scene has an invalid state) invalid goal and invalid start"""
    if ("cs", key) not in _cache:
        w = world(O, key)
        parts = [blocked(O, key)] + ([seam(O, key)] if key in SEAM else [])
        s, g = _with_invalid(w, parts)
        names = ["blocked"] * N_BLOCKED + (["seam"] * N_SEAM if key in SEAM else [])
        names += ["invalid_goal", "invalid_start"][:len(s) - len(names)]
        _cache["cs", key] = (s, g, names)
    return _cache["cs", key]


def star_set(O, key):
    if ("ss", key) not in _cache:
        w = world(O, key)
        parts = [near(O, key)] + ([seam(O, key)] if key in SEAM else [])
        s, g = _with_invalid(w, parts)
        names = ["near"] * N_NEAR + (["seam"] * N_SEAM if key in SEAM else [])
        names += ["invalid_goal", "invalid_start"][:len(s) - len(names)]
        _cache["ss", key] = (s, g, names)
    return _cache["ss", key]


# ---------------- references ----------------
def connect_ref(O, key):
    """orc.plan of the connect set -> (path [E, max_path, nq], path_len, status, n_checks)"""
    if ("cr", key) not in _cache:
        w = world(O, key)
        s, g, _ = connect_set(O, key)
        E, mp = len(s), CONNECT["max_path"]
        path, plen, st, chk = np.zeros((E, mp, w.orc.nq)), np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int64)
        for e in range(E):
            st[e], rows, chk[e], _ = w.orc.plan(s[e], g[e], w.range, 0.005, CONNECT["max_iters"], CONNECT["max_nodes"], seed=CONNECT_SEED,
                                                env_id=e, max_path=mp)
            plen[e] = len(rows)
            path[e, :len(rows)] = rows
        _cache["cr", key] = (path, plen, st, chk)
    return _cache["cr", key]


def race_reference(O, key):
    """list of race_ref.Race over the connect set, PORTFOLIO members"""
    if ("rr", key) not in _cache:
        w = world(O, key)
        s, g, _ = connect_set(O, key)
        _cache["rr", key] = race_ref.race_batch(w.orc, s, g, w.range, PORTFOLIO, CONNECT["max_iters"], CONNECT["max_nodes"], CONNECT["max_path"],
                                                seed=RACE_SEED)
    return _cache["rr", key]


def star_ref(O, key, variant=False):
    """rrtstar_ref.plan_star_batch of the star set (variant: threshold 0.15, bias 0.2)"""
    if ("sr", key, variant) not in _cache:
        w = world(O, key)
        s, g, _ = star_set(O, key)
        _cache["sr", key, variant] = rrtstar_ref.plan_star_batch(w.orc, s, g, w.range, STAR_ITERS, None, STAR_PATH, seed=STAR_SEED,
                                                                 **(VARIANT if variant else {}))
    return _cache["sr", key, variant]


def star_synthetic(O, key):
    """name -> (start, goal, keywords of plan_star): the longest solved path of the key's star set with a tree of 48 nodes and
    with max_path 2; stream id = that query's"""
    ref = star_ref(O, key)
    s, g, _ = star_set(O, key)
    e = int(np.argmax(ref[1]))
    assert ref[1][e] >= 3, (key, ref[1])
    return {"full_tree": (s[e], g[e], dict(max_nodes=48)), "short_max_path": (s[e], g[e], dict(max_path=2))}, e


K9 = {0: (simplify_ref.simplify_batch, 3), 1: (shortcut_ref.shortcut_batch, 7), 2: (smooth_ref.smooth_batch, 15)}


def k9_ref(O, key, level):
    """the level's *_batch reference over the oracle's paths of the connect set -> (path', path_len', info, ...)"""
    if ("k9", key, level) not in _cache:
        w = world(O, key)
        path, plen, st, _ = connect_ref(O, key)
        fn, passes = K9[level]
        _cache["k9", key, level] = fn(w.orc, path, plen, st, seed=K9_SEED, passes=passes)
    return _cache["k9", key, level]


def clear_set(O, key):
    s, g, _ = star_set(O, key)
    return s[:CLEAR_QUERIES[key]], g[:CLEAR_QUERIES[key]]


def clear_ref(O, key, band):
    if ("cl", key, band) not in _cache:
        w = world(O, key)
        s, g = clear_set(O, key)
        _cache["cl", key, band] = star_clearance_ref.plan_star_clearance_batch(w.pi, w.orc, s, g, w.range, band, CLEAR_ITERS, None, STAR_PATH,
                                                                              seed=STAR_SEED, **VARIANT)
    return _cache["cl", key, band]
