"""The race queries test_race_host.py and test_race_gpu.py share.  Construction (as in test_planner_builds_agree):
sample_states(pi, 8000, 91, "uniform"), the first 48 valid states are the starts, the next 48 the goals; seed 23, stream id 5 + query
index, max_nodes 4096, max_path 256, the scene's own range, 8 members.
  pusher48   PusherObstacle-v0, all 48 queries, 2000 iterations
  assembly8  SawyerAssemblyObstacle-v0, queries 1, 12, 23, 38 (members disagree) and 0, 4, 11, 2; 2000 iterations
  push16     SawyerPushObstacle-v0, the first 16 queries, 700 iterations
The references are computed once per process and never modified."""
import numpy as np

from conftest import sample_states

import race_ref as R

PUSHER, ASSEMBLY, PUSH = "PusherObstacle-v0", "SawyerAssemblyObstacle-v0", "SawyerPushObstacle-v0"
N_POOL, SEED, ID_BASE, K, MAX_NODES, MAX_PATH = 48, 23, 5, 8, 4096, 256
CASES = {
    "pusher48": (PUSHER, list(range(48)), 2000),
    "assembly8": (ASSEMBLY, [1, 12, 23, 38, 0, 4, 11, 2], 2000),
    "push16": (PUSH, list(range(16)), 700),
}

_cache = {}


def scene_of(O, env):
    from mopa_rl_amd.scene import planner_inputs
    if ("scene", env) not in _cache:
        pi = planner_inputs(env)
        _cache["scene", env] = (pi, O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold))
    return _cache["scene", env]


def pool(O, env):
    """-> (start [48, nq], goal [48, nq], first invalid sample's active coordinates)"""
    if ("pool", env) not in _cache:
        pi, orc = scene_of(O, env)
        qa, row = sample_states(pi, 8000, 91, "uniform")
        ov, _ = orc.is_valid_batch(qa, row, samples_per_env=len(qa))
        good = qa[ov == 1]
        assert len(good) >= 2 * N_POOL and (ov == 0).any()
        start, goal = np.repeat(row, N_POOL, axis=0), np.repeat(row, N_POOL, axis=0)
        start[:, pi.ref_joint_pos_indexes] = good[:N_POOL]
        goal[:, pi.ref_joint_pos_indexes] = good[N_POOL:2 * N_POOL]
        _cache["pool", env] = (start, goal, qa[ov == 0][0].copy())
    return _cache["pool", env]


def queries(O, case, invalid_goal=False):
    """-> (env, start [E, nq], goal [E, nq], stream ids [E], max_iters); invalid_goal: the LAST query's goal is replaced by an invalid
    state (the GPU cases carry one each)"""
    env, idx, iters = CASES[case]
    pi, _ = scene_of(O, env)
    start, goal, bad = pool(O, env)
    s, g = start[idx].copy(), goal[idx].copy()
    if invalid_goal:
        g[-1, pi.ref_joint_pos_indexes] = bad
    return env, s, g, np.array([ID_BASE + i for i in idx], dtype=np.int64), iters


def reference(O, case, invalid_goal=False, portfolio=K):
    """list of race_ref.Race, one per query of the case"""
    k = ("ref", case, bool(invalid_goal), int(portfolio))
    if k not in _cache:
        env, s, g, ids, iters = queries(O, case, invalid_goal)
        pi, orc = scene_of(O, env)
        base = _cache.get(("ref", case, False, int(portfolio)))
        if invalid_goal and base is not None:      # only the last query differs
            last = R.race(orc, s[-1], g[-1], pi.spec.range, portfolio, iters, MAX_NODES, MAX_PATH, SEED, int(ids[-1]))
            _cache[k] = base[:-1] + [last]
        else:
            _cache[k] = R.race_batch(orc, s, g, pi.spec.range, portfolio, iters, MAX_NODES, MAX_PATH, seed=SEED, env_ids=ids)
    return _cache[k]
