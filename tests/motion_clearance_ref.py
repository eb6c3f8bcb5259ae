"""Sequential reference of the clearance report (csrc/mopa_motion_clearance.inc, DESIGN.md section 4 "Clearance report") for
test_motion_clearance_host.py and test_motion_clearance_gpu.py: OMPL's MinimaxObjective::motionCost(s1, s2) under the state cost of
maximize_min_clearance, and the path cost built on it, restated state by state.  It shares no code with the kernels: it composes the
two sequential forms that exist, unchanged -- the states of a segment from motion_report_ref.segment_states, the band-limited
distances of a state from proximity_ref.poses / pair_dists (the oracle's FK, mopa_geom_sep_host per pair with no broad phase) and
proximity_ref.select's rule for the clearance and the nearest pair.  This form is the definition: the kernels reproduce it bit for bit.

Segment qa -> qb, band b >= 0: c = max(nd, 1) states s_1 .. s_c, s_c = qb; qa is not evaluated.  Per state d_k, p_k = the clearance and
the first pair of select(D, b, 1): d_k saturates at b, p_k = -1 when nothing is within the band.  Per segment: clearance = min_k d_k,
n_states = c, n_near = #{k: a pair at dist <= b}, k_min = the smallest k with d_k == clearance and p_k >= 0 (0 when n_near == 0),
t_min = k_min / c, pair_min = p_{k_min} (-1 when k_min == 0), end_clearance = d_c, q_min = s_{k_min} (qb when k_min == 0).

Path [len, nq], len >= 1 (the env row is the path's row 0): v_0 = the state clearance of vertex 0, then the segments j -> j + 1.
clearance = min(v_0, min_j seg_clearance_j); seg_min = -1 when v_0 attains it (which covers "nothing within the band"), else the
smallest j that does; k_min / pair_min are that segment's, or 0 and v_0's pair; mean_vertex_clearance = (v_0 + sum_j end_clearance_j)
/ len, summed left to right in float64 -- OMPL's PathGeometric::clearance(), band-saturated.  len == 0 (an unsolved query): NaN, -1,
0, -1, NaN.  Counting vertex 0 deviates from OMPL's default initialCost on purpose."""
import functools

import numpy as np

import motion_report_ref as MR
import proximity_ref as P
from simplify_ref import so2_flags

#: the per-segment outputs, in the order of the C ABI
OUTPUTS = ("clearance", "n_states", "n_near", "k_min", "t_min", "pair_min", "end_clearance", "q_min")


def state_clearances(pi, orc, states, rows, band):
    """(d [T], p [T] int32, count [T] int32) of the states [T, na] on their own env rows [T, nq]"""
    states = np.ascontiguousarray(states, dtype=np.float64)
    if len(states) == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    gpos, gmat = P.poses(pi, orc, states, rows, 1)
    cl, cnt, pair, _ = P.select(P.pair_dists(pi, gpos, gmat, band), band, 1)
    return cl, pair[:, 0].copy(), cnt


def motion_clearance(pi, orc, qa, qb, rows, band, samples_per_env=None, resolution=MR.RESOLUTION):
    """dict of numpy arrays, the keys of OUTPUTS (clearance / t_min / end_clearance [N] float64, n_states / n_near / k_min / pair_min
    [N] int32, q_min [N, na]) and, for the tests, `d` / `p`: per segment the arrays d_1 .. d_c and p_1 .. p_c"""
    qa, qb, rows = np.asarray(qa, dtype=np.float64), np.asarray(qb, dtype=np.float64), np.atleast_2d(np.asarray(rows, dtype=np.float64))
    N, na = qa.shape
    spe = samples_per_env if samples_per_env is not None else max(1, N // len(rows))
    so2 = so2_flags(pi.model, pi.ref_joint_pos_indexes)
    ext = MR.extents(pi.model, pi.ref_joint_pos_indexes, so2)
    states = [MR.segment_states(qa[i], qb[i], so2, ext, resolution) for i in range(N)]
    env = np.concatenate([np.full(len(s), i // spe) for i, s in enumerate(states)]) if N else np.zeros(0, dtype=np.int64)
    d_all, p_all, n_all = state_clearances(pi, orc, np.concatenate(states) if N else np.zeros((0, na)), rows[env], band)
    rep = {"clearance": np.zeros(N), "n_states": np.zeros(N, dtype=np.int32), "n_near": np.zeros(N, dtype=np.int32),
           "k_min": np.zeros(N, dtype=np.int32), "t_min": np.zeros(N), "pair_min": np.zeros(N, dtype=np.int32),
           "end_clearance": np.zeros(N), "q_min": np.zeros((N, na)), "d": [], "p": []}
    o = 0
    for i in range(N):
        c = len(states[i])
        d, p, n = d_all[o:o + c], p_all[o:o + c], n_all[o:o + c]
        o += c
        clearance = d.min()
        k_min = 0
        for k in range(1, c + 1):           # ascending: the smallest k that attains the minimum with a pair in band
            if d[k - 1] == clearance and p[k - 1] >= 0:
                k_min = k
                break
        assert (k_min == 0) == (not (n > 0).any())
        rep["clearance"][i] = clearance
        rep["n_states"][i] = c
        rep["n_near"][i] = int((n > 0).sum())
        rep["k_min"][i] = k_min
        rep["t_min"][i] = float(k_min) / float(c) if k_min else 0.0
        rep["pair_min"][i] = p[k_min - 1] if k_min else -1
        rep["end_clearance"][i] = d[c - 1]
        rep["q_min"][i] = states[i][k_min - 1] if k_min else qb[i]
        rep["d"].append(d)
        rep["p"].append(p)
    return rep


def path_clearance(pi, orc, path, path_len, band):
    """path [E, max_path, nq], path_len [E] -> dict: clearance / mean_vertex_clearance [E] float64, seg_min / k_min / pair_min [E]
    int32, and `segments`: `motion_clearance` of the compacted segment list (path by path, j ascending) with its `path_index` /
    `seg_index` [M] int64"""
    path = np.asarray(path, dtype=np.float64)
    E = len(path)
    act = np.asarray(pi.ref_joint_pos_indexes)
    out = {"clearance": np.full(E, np.nan), "seg_min": np.full(E, -1, dtype=np.int32), "k_min": np.zeros(E, dtype=np.int32),
           "pair_min": np.full(E, -1, dtype=np.int32), "mean_vertex_clearance": np.full(E, np.nan)}
    pe = np.array([e for e in range(E) for j in range(int(path_len[e]) - 1)], dtype=np.int64)
    pj = np.array([j for e in range(E) for j in range(int(path_len[e]) - 1)], dtype=np.int64)
    seg = motion_clearance(pi, orc, path[pe, pj][:, act].reshape(-1, len(act)), path[pe, pj + 1][:, act].reshape(-1, len(act)),
                           path[pe, 0].reshape(-1, path.shape[2]), band, samples_per_env=1) if len(pe) else \
        motion_clearance(pi, orc, np.zeros((0, len(act))), np.zeros((0, len(act))), path[:1, 0], band, samples_per_env=1)
    seg["path_index"], seg["seg_index"] = pe, pj
    out["segments"] = seg
    solved = [e for e in range(E) if int(path_len[e]) >= 1]
    v0, p0, _ = state_clearances(pi, orc, path[solved, 0][:, act], path[solved, 0], band)
    for n, e in enumerate(solved):
        mine = np.nonzero(pe == e)[0]                      # this path's segments, j ascending
        best, seg_min, k_min, pair_min = v0[n], -1, 0, p0[n]
        for i in mine:
            if seg["clearance"][i] < best:                 # strictly smaller: vertex 0 first, then the smallest j, keeps a tie
                best, seg_min, k_min, pair_min = seg["clearance"][i], int(pj[i]), seg["k_min"][i], seg["pair_min"][i]
        total = np.float64(v0[n])
        for i in mine:
            total = total + np.float64(seg["end_clearance"][i])
        out["clearance"][e], out["seg_min"][e], out["k_min"][e], out["pair_min"][e] = best, seg_min, k_min, pair_min
        out["mean_vertex_clearance"][e] = total / np.float64(int(path_len[e]))
    return out


def classes(rep):
    """the five classes of the mix condition: nothing in band, in overlap, the minimum at k = 1 with c > 1, in the interior, at the end
    state with c > 1 (the second overlaps with the last three)"""
    k, c = rep["k_min"], rep["n_states"]
    return {"far": k == 0, "overlap": rep["clearance"] < 0, "first": (k == 1) & (c > 1), "interior": (k > 1) & (k < c), "end": (k == c) & (c > 1)}


BASE = tuple(range(0, 96)) + tuple(range(256, 352))       # the prefix of motion_report_ref.shared_segments the host test walks
N_DISTAL = 24
N_APART = 24


@functools.lru_cache(maxsize=None)
def mix_segments(env):
    """(pi, orc, qa [n, na], qb [n, na], rows [n, nq], base [n] int64): the segments both test files use, one env row per segment
    (samples_per_env = 1), n >= 300, in an order whose prefixes are mixed (the distal segments at positions 40 .. 40 + N_DISTAL).  `base[i]` is the segment's index in shared_segments, -1
    for the ones added here: shared_segments start at valid states, which leaves "minimum at k = 1" and "in overlap" short on some
    scenes, so the long shared segments are also walked backwards (qb -> qa), and N_DISTAL segments move the most distal joint alone
    (the tie cases: the nearest pair does not move).  Pusher's box rests 4 mm above its target in the shared row, so nothing there
    is ever out of a 1 cm band: N_APART more shared segments run on a row with box and target moved apart and out of the arm's way."""
    pi, orc, qa, qb, row = MR.shared_segments(env)
    idx = np.array(BASE)
    rev = np.array(tuple(range(256, 352)) + tuple(range(64, 96)))
    da = qa[np.arange(N_DISTAL) * 4]
    db = da.copy()
    lo, hi = pi.jnt_minimum[-1], pi.jnt_maximum[-1]
    db[:, -1] = np.where(da[:, -1] + 0.4 <= hi, da[:, -1] + 0.4, np.maximum(lo, da[:, -1] - 0.4))
    A = [qa[idx], qb[rev], da]
    B = [qb[idx], qa[rev], db]
    rows = np.repeat(row, len(idx) + len(rev) + N_DISTAL, axis=0)
    if env == "PusherObstacle-v0":
        apart = np.arange(100, 100 + N_APART)
        A.append(qa[apart])
        B.append(qb[apart])
        far_row = row.copy()
        far_row[0, 12:16] = (0.35, 0.45, 0.45, 0.35)
        rows = np.concatenate([rows, np.repeat(far_row, N_APART, axis=0)])
    A, B = np.concatenate(A), np.concatenate(B)
    base = np.concatenate([idx, np.full(len(A) - len(idx), -1)])
    # a random order, except that the distal segments sit together behind the first 40: inside every prefix of 65 or more, so a
    # batch of the GPU test's size holds the tie cases too
    d0 = len(idx) + len(rev)
    distal = np.arange(d0, d0 + N_DISTAL)
    others = np.concatenate([np.arange(d0), np.arange(d0 + N_DISTAL, len(A))])
    others = others[np.random.default_rng(17).permutation(len(others))]
    order = np.concatenate([others[:40], distal, others[40:]])
    A, B, rows, base = np.ascontiguousarray(A[order]), np.ascontiguousarray(B[order]), np.ascontiguousarray(rows[order]), base[order]
    for a in (A, B, rows, base):
        a.setflags(write=False)
    return pi, orc, A, B, rows, base


@functools.lru_cache(maxsize=None)
def mix_report(env, band):
    """the reference report of mix_segments(env) on its own rows (cached, read-only)"""
    pi, orc, A, B, rows, _ = mix_segments(env)
    rep = motion_clearance(pi, orc, A, B, rows, band, 1)
    for a in rep.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rep
