"""The cases of the K9 tests (test_simplify_host.py, test_simplify_gpu.py): blocked planner queries on Push and Pusher, their
oracle plans, and synthetic paths in free space."""
import numpy as np

from conftest import sample_states

PLAN_SEED = 7
MAX_NODES = 4096
MAX_PATH = 256
# (sampling mode, queries, planner iterations): Push as the issue names them; Pusher needs more of both to solve a few
QUERY_SETS = {"SawyerPushObstacle-v0": ("near", 24, 1000), "PusherObstacle-v0": ("uniform", 48, 3000)}


def scene_of(O, env):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(env)
    return pi, O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)


def blocked_queries(pi, orc, env):
    """sample_states(pi, 4000, 41, mode), the valid states paired (0,1), (2,3), ...: the first pairs whose straight line fails
    check_motion -- the case in which the rollout calls the planner at all.  -> (start [n, nq], goal [n, nq])"""
    mode, n, _ = QUERY_SETS[env]
    qa, row = sample_states(pi, 4000, 41, mode)
    v, _ = orc.is_valid_batch(qa, row, want_min_dist=False)
    good = qa[v == 1]
    start, goal = [], []
    for k in range(0, len(good) - 1, 2):
        if not orc.check_motion(row[0], good[k], good[k + 1])[0]:
            s, g = row[0].copy(), row[0].copy()
            s[orc.active_idx], g[orc.active_idx] = good[k], good[k + 1]
            start.append(s)
            goal.append(g)
            if len(start) == n:
                break
    assert len(start) == n
    return np.array(start), np.array(goal)


def oracle_plans(pi, orc, env, start, goal):
    """-> (status [n] int32, list of path rows [len, nq]; empty for unsolved queries); query e samples stream (PLAN_SEED, e)"""
    iters = QUERY_SETS[env][2]
    st, paths = [], []
    for e in range(len(start)):
        s, p, _, _ = orc.plan(start[e], goal[e], pi.spec.range, 0.005, iters, MAX_NODES, seed=PLAN_SEED, env_id=e, max_path=MAX_PATH)
        st.append(s)
        paths.append(p if s == 0 else np.zeros((0, orc.nq)))
    return np.array(st, dtype=np.int32), paths


def push_out_and_back(pi, orc, n=6):
    """Push, free space: n rows along a free straight line between two valid states near the initial pose, then n rows back
    towards the first without reaching it, so that non-adjacent rows lie close together"""
    from simplify_ref import out_and_back
    qa, row = sample_states(pi, 400, 43, "near")
    v, _ = orc.is_valid_batch(qa, row, want_min_dist=False)
    good = qa[v == 1]
    for k in range(0, len(good) - 1, 2):
        if orc.check_motion(row[0], good[k], good[k + 1])[0] and np.abs(good[k] - good[k + 1]).sum() > 0.5:
            return out_and_back(good[k], good[k + 1], n, np.asarray(orc.active_idx), row[0])
    raise AssertionError("no free straight line among the sampled Push states")


def pusher_wrap_path(pi, orc):
    """Pusher, free space: four rows that differ in joint0 only and cross its +-pi seam (3.05, 2.6 | -3.1, -2.6).  With the SO(2)
    wrap rows 0 and 2 are the closest pair two apart (0.13), without it rows 1 and 3 would be (5.2)."""
    from mopa_rl_amd.scene import default_qpos
    row = default_qpos(pi.spec.env, pi.model)
    rows = np.repeat(row[None], 4, axis=0)
    act = np.asarray(orc.active_idx)
    for k, j0 in enumerate((3.05, 2.6, -3.1, -2.6)):
        rows[k, act] = (j0, 2.6, -2.39, 2.54)
    for k in range(3):
        assert orc.check_motion(rows[0], rows[k, act], rows[k + 1, act])[0], "the synthetic Pusher path is not in free space"
    return rows
