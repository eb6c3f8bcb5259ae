"""The queries test_star_clearance_host.py and test_star_clearance_gpu.py share, built like star_cases.py: sample_states(pi, 4000, 41,
"near"), the states valid on the case's env row paired (0,1), (2,3), ...; seed 7, stream id = query index, max_nodes = max_iters + 1,
the scene's own range (Pusher: 0.1, see below), goal_threshold 0.15 and goal_bias 0.2 (several goal nodes per query, so the choice among them is exercised).

Chosen sizes (the reference runs at roughly half a second per Pusher query of 300 iterations here, the whole host file in about a
minute): Pusher 8 queries x 300 iterations at band 0, 1 cm and 5 cm; Push 4 queries x 150 iterations at band 0 and 1 cm; Lift 2 queries x 100
iterations at 1 cm, the first of them starting next to the can (LIFT_START_SAMPLE).  Pusher's box rests 4 mm above its target in the default row, which would hold every clearance at 4 mm under any
band above it, so the Pusher cases run on motion_clearance_ref's row with box and target moved apart.  They also steer with range
0.1, the value of the env's simple planner, instead of 0.2: chains then have enough edges for a later route to raise a node's
clearance -- at 0.2, 32 queries of 300 iterations at 1 cm held no such rewire, at 0.1 these 8 hold three, and every other event
of the mix condition (CPU search, the reference's events).  The references are computed
once per process and never modified."""
import numpy as np

from conftest import sample_states

import rrtstar_ref as R
import star_cases as SC
import star_clearance_ref as SR

PUSH, PUSHER, LIFT = SC.PUSH, SC.PUSHER, "SawyerLiftObstacle-v0"
SEED, MAX_PATH = SC.SEED, SC.MAX_PATH
PARAMS = dict(SC.VARIANT)
#: env -> (queries, iterations, bands)
SIZES = {PUSHER: (8, 300, (0.0, 0.01, 0.05)), PUSH: (4, 150, (0.0, 0.01)), LIFT: (2, 100, (0.01,))}

RANGE = {PUSHER: 0.1}
#: Lift: the sample (of the 4000) the first query starts at, the only valid one whose nearest pair within 1 cm is a pair of the can
#: (7.9 mm): the MESH instantiation then evaluates the can in band from the root on (test_star_clearance_host checks the events)
LIFT_START_SAMPLE = 3421

_cache = {}


def range_of(pi, env):
    return RANGE.get(env, pi.spec.range)


def scene_of(O, env):
    return SC.scene_of(O, env)


def queries(O, env):
    """-> (start [n, nq], goal [n, nq])"""
    if ("q", env) not in _cache:
        pi, orc = scene_of(O, env)
        n = SIZES[env][0]
        qa, row = sample_states(pi, 4000, 41, "near")
        if env == PUSHER:
            row = row.copy()
            row[0, 12:16] = (0.35, 0.45, 0.45, 0.35)
        v, _ = orc.is_valid_batch(qa, row, want_min_dist=False)
        good = qa[v == 1][:2 * n]
        assert len(good) == 2 * n
        start, goal = np.repeat(row, n, axis=0), np.repeat(row, n, axis=0)
        start[:, orc.active_idx], goal[:, orc.active_idx] = good[0::2], good[1::2]
        if env == LIFT:
            assert v[LIFT_START_SAMPLE] == 1
            start[0, orc.active_idx] = qa[LIFT_START_SAMPLE]
        _cache["q", env] = (start, goal)
    return _cache["q", env]


def reference(O, env, band):
    """plan_star_clearance_batch of the env's queries at `band`"""
    k = ("ref", env, float(band))
    if k not in _cache:
        pi, orc = scene_of(O, env)
        start, goal = queries(O, env)
        _cache[k] = SR.plan_star_clearance_batch(pi, orc, start, goal, range_of(pi, env), band, SIZES[env][1], None, MAX_PATH, seed=SEED, **PARAMS)
    return _cache[k]


def path_length_reference(O, env):
    """rrtstar_ref.plan_star_batch of the same queries and parameters"""
    k = ("pl", env)
    if k not in _cache:
        pi, orc = scene_of(O, env)
        start, goal = queries(O, env)
        _cache[k] = R.plan_star_batch(orc, start, goal, range_of(pi, env), SIZES[env][1], None, MAX_PATH, seed=SEED, **PARAMS)
    return _cache[k]


def synthetic(O):
    """the four synthetic Pusher cases of star_cases.synthetic on this file's queries: name -> (start, goal, keywords, expected
    status), and the stream id they run under"""
    if "syn" not in _cache:
        pi, orc = scene_of(O, PUSHER)
        start, goal = queries(O, PUSHER)
        qa, _ = sample_states(pi, 4000, 41, "near")
        v, _ = orc.is_valid_batch(qa, start[:1], want_min_dist=False)
        bad = start[0].copy()
        bad[orc.active_idx] = qa[v == 0][0]
        ref = reference(O, PUSHER, 0.01)
        longest = int(np.argmax(ref[1]))
        assert ref[1][longest] >= 3
        _cache["syn"] = ({
            "invalid_goal": (start[0], bad, {}, R.PLAN_INVALID_GOAL),
            "invalid_start": (bad, goal[0], {}, R.PLAN_NO_EXACT),
            "full_tree": (start[longest], goal[longest], dict(max_nodes=64), None),
            "short_max_path": (start[longest], goal[longest], dict(max_path=2), R.PLAN_NO_EXACT),
        }, longest)
    return _cache["syn"]
