"""The planner-job state machine (mopa_rl_amd/plan_jobs.py) on the CPU: CPU tensors, no stream, `device_paths=False`, with the CPU
oracle (or canned planners) standing in for the two `BatchPlanner`s.

Tests 1-3 run the reference's `SACAgent.plan` recordings (tests/golden/ref_py_agent_push*.npz, tools/gen_ref_py_golden.py) through
`PlannerJobs`: the recording the GPU leg of test_ref_py_agent.py uses, the same cases with a planner range of 0.5 (every RRT-Connect path
has steps longer than ac_scale, so the densification does real work), and those cases twice over in one job (more than 64 rows: the
split by path length).  Test 4 drives the fallback stages, which no recording reaches, with canned planners and a validity rule, against
a plain per-segment loop that restates rl/sac_agent.py:216-233 and the fallback order of :300-306."""
import os

import numpy as np

from oracle_bp import OracleBP, bits

ENV = "SawyerPushObstacle-v0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_RUNS = {}


def _oracle_jobs(oracle_mod, G):
    """`PlannerJobs` over the oracle with the recording's parameters (and the generator's stream convention: E = its 64 cases)"""
    from mopa_rl_amd.agent_planning import JointLimits
    from mopa_rl_amd.plan_jobs import PlannerJobs
    from mopa_rl_amd.planner import ITERS_PER_SECOND
    from mopa_rl_amd.rollout import RolloutConfig
    from mopa_rl_amd.scene import planner_inputs, qpos_joint_arrays
    timelimit, max_nodes, max_path, seed, ac_scale = G["params"][:5]
    over = {"range": float(G["params"][5])} if len(G["params"]) > 5 else {}
    cfg = RolloutConfig(timelimit=float(timelimit), max_nodes=int(max_nodes), max_path=int(max_path), seed=int(seed), ac_scale=float(ac_scale),
                        device_paths=False, **over)
    pi = planner_inputs(ENV)
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, cfg.contact_threshold)
    idx, lo, hi, lim = qpos_joint_arrays(pi.model)
    bp, n = OracleBP(orc, cfg.range), len(pi.ref_joint_pos_indexes)
    valid = lambda q: bp.is_valid(q[:, :n].contiguous(), q.contiguous(), samples_per_env=1).bool()
    iters = lambda t: max(1, int(round(t * ITERS_PER_SECOND)))
    return PlannerJobs(cfg, bp, OracleBP(orc, cfg.simple_planner_range), JointLimits(lo[idx], hi[idx], lim[idx], cfg.joint_margin), valid, n,
                       pi.model.nq, [], 0, len(G["cur"]), iters(cfg.timelimit), iters(cfg.simple_planner_timelimit), "cpu")


def _check_plan(G, traj, lens, success, interpolation, valid, exact):
    """the assertions of test_ref_py_agent.py::test_plan_batch_equals_reference_gpu"""
    traj, lens = traj.numpy(), lens.numpy()
    F = G["plan_flags"]
    for k in range(len(G["cur"])):
        assert (bool(success[k]), bool(valid[k]), bool(exact[k])) == (bool(F[k, 0]), bool(F[k, 2]), bool(F[k, 3])), k
        if success[k]:
            assert bool(interpolation[k]) == bool(F[k, 1]), k
            assert lens[k] == G["plan_len"][k], k
            assert np.array_equal(bits(traj[k, :lens[k]]), bits(G["plan_traj"][k, :lens[k]])), k
    assert (F[:, 0] & (1 - F[:, 1])).sum() >= 5 and (F[:, 2] == 0).sum() >= 5      # RRT paths and invalid goals both present


def _plan_recording(oracle_mod, name):
    import torch
    G = np.load(os.path.join(GOLDEN, name))
    jobs = _oracle_jobs(oracle_mod, G)
    K = len(G["cur"])
    out = jobs.plan(torch.tensor(G["cur"]), torch.tensor(G["tgt"]), torch.arange(K), torch.zeros(K, dtype=torch.int64))
    _check_plan(G, *out)
    return G, jobs


def _long_rows(oracle_mod, copies):
    """all 64 cases of the long-range recording, `copies` times over, as ONE planner job (every row gets its case's stream and seed);
    computed once per `copies`, read-only afterwards"""
    import torch
    if copies not in _RUNS:
        G = np.load(os.path.join(GOLDEN, "ref_py_agent_push_long.npz"))
        jobs = _oracle_jobs(oracle_mod, G)
        K = len(G["cur"])
        rep = lambda x: torch.cat([x] * copies).contiguous()
        cur = jobs.limits.clip_state(torch.tensor(G["cur"]))
        job = jobs.launch(rep(cur), rep(torch.tensor(G["tgt"])), rep(torch.arange(K)), rep(torch.zeros(K, dtype=torch.int64)))
        _RUNS[copies] = (job, jobs.finish(job))
    return _RUNS[copies]


def test_reference_plan_through_planner_jobs(oracle_mod):
    _plan_recording(oracle_mod, "ref_py_agent_push.npz")


def test_reference_plan_with_densified_paths(oracle_mod):
    G, _ = _plan_recording(oracle_mod, "ref_py_agent_push_long.npz")
    assert float(G["params"][5]) == 0.5
    job, (tr, ln, ok, _, _) = _long_rows(oracle_mod, 1)
    # the rows plan() handed to RRT-Connect are among these 64; their trajectories are the recording's
    rrt = np.nonzero(G["plan_flags"][:, 0] & (1 - G["plan_flags"][:, 1]))[0]
    for k in rrt:
        assert ok[k] and np.array_equal(bits(tr[k, :ln[k]]), bits(G["plan_traj"][k, :G["plan_len"][k]])), k
    cut = int(np.isin(job.host.good[job.host.seg_r], rrt).sum())          # long segments cut in those paths
    assert cut >= 40, cut                       # (a floor: the fixture exercises the densification)


def test_bucket_split_equals_the_unsplit_job(oracle_mod):
    job1, one = _long_rows(oracle_mod, 1)
    job2, two = _long_rows(oracle_mod, 2)
    assert job1.subs is None and len(job2.subs) >= 2
    K = len(one[1])
    for c in range(2):
        for k in range(K):
            r = c * K + k
            assert two[1][r] == one[1][k] and [bool(f[r]) for f in two[2:]] == [bool(f[k]) for f in one[2:]], r
            assert np.array_equal(bits(two[0][r, :two[1][r]]), bits(one[0][k, :one[1][k]])), r


# ---- the fallback stages ------------------------------------------------------------------------------------------------------
NQ, N, AC_SCALE, BAND = 4, 3, 0.05, (0.30, 0.45)          # BAND: invalid where frac(2 * joint 0) lies inside


def _state_ok(q):
    return not (BAND[0] < (2.0 * q[0]) % 1.0 < BAND[1])


def _first_path(s, g, k):
    """what the canned main planner answers to the query of env k: a sentinel, or five rows with three long steps and a short last one"""
    from mopa_rl_amd import _lib
    if k % 8 == 6:
        return _lib.PLAN_INVALID_GOAL
    if k % 8 == 7:
        return _lib.PLAN_NO_EXACT
    d = g - s
    a = s + 0.3 * d + 0.07 * np.sin(5 * s + 1)
    b = s + 0.7 * d - 0.06 * np.cos(3 * g)
    near = g - 0.02 * np.cos(7 * s)
    rows = np.stack([s, a, b, near, g])
    rows[:, N:] = s[N:]
    return rows


def _simple_path(s, g):
    if int(abs(s[1]) * 100) % 2:
        return None
    mid = 0.5 * (s + g)
    mid[0] += 0.2
    return np.stack([s, mid, g])


def _main_path(s, g):
    if int(abs(s[2]) * 100) % 2:
        return None
    return np.stack([s, s + 0.25 * (g - s) + 0.1, s + 0.75 * (g - s) - 0.1, g])


class CannedBP:
    """answers planner launches from a rule (start row, goal row, stream id) -> rows | status | None; every query must arrive with
    the seed `seed_of(stream id)`"""

    def __init__(self, rule, seed_of):
        self.rule, self.seed_of = rule, seed_of

    def plan(self, start, goal, max_path=256, env_ids=None, seeds=None, **kw):
        import torch
        from mopa_rl_amd import _lib
        E = len(start)
        path = np.full((E, max_path, NQ), np.nan)          # (the tail of a row is whatever the allocator left)
        plen, status = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
        for k in range(E):
            assert int(seeds[k]) == self.seed_of(int(env_ids[k])), (k, int(env_ids[k]), int(seeds[k]))
            got = self.rule(start[k].numpy(), goal[k].numpy(), int(env_ids[k]))
            if isinstance(got, np.ndarray):
                path[k, :len(got)], plen[k] = got, len(got)
            else:
                status[k] = _lib.PLAN_NO_EXACT if got is None else got
        return tuple(torch.from_numpy(x) for x in (path, plen, status, np.zeros(E, dtype=np.int64)))


def _rebuilt(start, rows):
    """SamplingBasedPlanner.plan + PlannerAgent.plan: start + the running sum of successive differences, without row 0"""
    out, acc = [], start.copy()
    for k in range(1, len(rows)):
        acc = acc + (rows[k] - rows[k - 1])
        out.append(acc.copy())
    return out


LO, HI, LIMITED = np.full(NQ, -10.0), np.array([10.0, 0.6, 10.0, 10.0]), np.array([True, True, False, True])


def _clip_qpos(q, margin):
    """SACAgent.clip_qpos (rl/sac_agent.py:237-260) against the agents' float32 limits"""
    lo, hi = LO.astype(np.float32), HI.astype(np.float32)
    if np.any(q[LIMITED] < lo[LIMITED]) or np.any(q[LIMITED] > hi[LIMITED]):
        new = np.clip(q.copy(), lo + np.float32(margin), hi - np.float32(margin))
        new[~LIMITED] = q[~LIMITED]
        return new
    return q


def _expected(cur, tgt, k, clip, seen):
    """rl/sac_agent.py:212-233 (with simple_interpolate(use_planner=True), :262-318) for one query, as a loop"""
    first = _first_path(cur, tgt, k)
    if not isinstance(first, np.ndarray):
        return None
    traj, new, start, bound = _rebuilt(cur, first), [], cur, AC_SCALE * 0.8
    for wp in traj:
        diff = wp - start
        if np.any(diff[:N] < -AC_SCALE) or np.any(diff[:N] > AC_SCALE):
            s = clip(start)
            moved = not np.array_equal(s, start)
            seen["clipped"] += moved
            d = wp[:N] - s[:N]
            scales = [d[j] / bound if d[j] > bound else d[j] / -bound for j in range(N) if d[j] > bound or d[j] < -bound]
            factor = max(max(scales), 1.0) if scales else 1.0
            step, q, inner, ok = d / factor, s.copy(), [], True
            for _ in range(int(factor)):
                q[:N] += step
                if not _state_ok(q):
                    ok = False
                    break
                inner.append(q.copy())
            if ok:
                new += inner + [wp]
                seen["cut"] += 1
            else:
                rows = _simple_path(s, wp)
                kind = "simple"
                if rows is None:
                    rows, kind = _main_path(s, wp), "main"
                new += _rebuilt(s, rows) if rows is not None else [wp]
                seen[kind if rows is not None else "end"] += 1
                seen["clipped_fallback"] += moved
        else:
            new.append(wp)
            seen["waypoint"] += 1
        start = wp
    return np.array(new)


def test_fallback_stages_equal_the_per_segment_loop():
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.agent_planning import JointLimits
    from mopa_rl_amd.plan_jobs import PlannerJobs
    from mopa_rl_amd.rollout import RolloutConfig
    M = 40
    rng = np.random.default_rng(5)
    cur = np.concatenate([rng.uniform(-1, 1, (M, N)), np.full((M, NQ - N), 0.5)], axis=1)
    tgt = cur.copy()
    tgt[:, :N] += rng.uniform(-0.9, 0.9, (M, N))
    cfg = RolloutConfig(ac_scale=AC_SCALE, device_paths=False, seed=3)
    # joint 1 has a limit inside the paths' range: segment starts beyond it are clipped (rl/sac_agent.py:266) before they are cut
    limits = JointLimits(LO, HI, LIMITED, cfg.joint_margin)
    clip = lambda q: _clip_qpos(q, cfg.joint_margin)
    cur = np.array([clip(q) for q in cur])                  # (SACAgent.plan clips the current state first, :205)
    steps = np.arange(M) % 5 + 1                            # every env at its own step count: seed + steps keys all three planners
    seed_of = lambda sid: cfg.seed + int(steps[sid % M])
    valid = lambda q: torch.tensor([_state_ok(r) for r in q.numpy()])
    main = CannedBP(lambda s, g, sid: _first_path(s, g, sid) if sid < M else (_main_path(s, g) if sid >= 2 * M else 1 / 0), seed_of)
    simple = CannedBP(lambda s, g, sid: _simple_path(s, g) if M <= sid < 2 * M else 1 / 0, seed_of)
    jobs = PlannerJobs(cfg, main, simple, limits, valid, N, NQ, [], 0, M, 300, 30, "cpu")
    job = jobs.launch(torch.tensor(cur), torch.tensor(tgt), torch.arange(M), torch.tensor(steps))
    tr, ln, ok, v, e = jobs.finish(job)
    seen = dict(waypoint=0, cut=0, simple=0, main=0, end=0, clipped=0, clipped_fallback=0)
    for k in range(M):
        want = _expected(cur[k], tgt[k], k, clip, seen)
        first = _first_path(cur[k], tgt[k], k)
        assert (bool(ok[k]), bool(v[k]), bool(e[k])) == (want is not None, first != _lib.PLAN_INVALID_GOAL if want is None else True,
                                                        first != _lib.PLAN_NO_EXACT if want is None else True), k
        if want is None:
            assert ln[k] == 0, k
            continue
        assert ln[k] == len(want), k
        assert np.array_equal(bits(tr[k, :ln[k]]), bits(want)), k
    assert min(seen.values()) >= 2, seen       # every outcome, and clipped starts among the cut and the fallback segments
