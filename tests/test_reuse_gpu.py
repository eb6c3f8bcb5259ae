"""The reuse_data relabelling on the device (mopa_reuse_batch behind `reuse_transitions_device`) against the host loop
`reuse_transitions` on the same record with the same draws.  Both sides do the same IEEE operations in the same order
(no contraction), so every comparison is on bit patterns: a one-ULP difference is a contracted multiply-add or
a reordered division -- a bug, not a tolerance."""
import functools
import os

import numpy as np
import pytest

from reuse_ref import as_out, classify_draws, counter_rng, synthetic_record

pytestmark = pytest.mark.gpu

KEYS_INT = ("env", "start", "goal", "done", "intra_steps")
KEYS_F64 = ("ob", "ac", "ob_next")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(got, want, msg=""):
    assert len(got) == len(want), f"{msg}: {len(got)} transitions, the host function has {len(want)}"
    for k in KEYS_INT:
        assert [int(g[k]) for g in got] == [int(w[k]) for w in want], f"{msg}: {k}"
    assert np.array_equal(_bits([g["rew"] for g in got]), _bits([w["rew"] for w in want])), f"{msg}: rew"
    for k in KEYS_F64:
        for r, (g, w) in enumerate(zip(got, want)):
            assert g[k].shape == w[k].shape and np.array_equal(_bits(g[k]), _bits(w[k])), f"{msg}: {k} of row {r}"
    assert [g.get("ac_type") for g in got] == [w.get("ac_type") for w in want], f"{msg}: ac_type"


def _cfg(env_name, **kw):
    from mopa_rl_amd.rollout import RolloutConfig
    return RolloutConfig.for_env(env_name, **kw)


# name -> (env whose constants are used, n_arm, gripper index, D, L, R, overrides of the config, ac_type column)
CASES = {
    "push-d5-r15": ("SawyerPushObstacle-v0", 7, None, 5, 12, 15, {}, False),
    "lift-d40-r15-grip": ("SawyerLiftObstacle-v0", 7, 7, 40, 12, 15, {"discrete_action": True}, True),
    "push-d5-r1-normal": ("SawyerPushObstacle-v0", 7, None, 5, 12, 1, {"ac_space_type": "normal"}, False),
    "push-d5-r64-l70": ("SawyerPushObstacle-v0", 7, None, 5, 70, 64, {}, False),
    "lift-d40-r64-l70-normal-grip": ("SawyerLiftObstacle-v0", 7, 8, 40, 70, 64, {"ac_space_type": "normal"}, False),
    "pusher-d40-r15-sharded": ("PusherObstacle-v0", 4, None, 40, 12, 15, {"env_id_base": 100, "env_id_total": 1000}, False),
}
T_KEY = 3      # agent-step count that enters the draws' key


def _case(name, E=67):
    """(cfg, n_arm, grip, R, record as numpy, ac_type, rng factory, host list) of a case: the reference is computed once"""
    return _case_cached(name, E)


@functools.lru_cache(maxsize=None)
def _case_cached(name, E):
    from mopa_rl_amd.rollout import reuse_transitions
    env_name, n_arm, grip, D, L, R, over, with_type = CASES[name]
    cfg = _cfg(env_name, **over)
    nq = n_arm + 2
    # (normal map: ac = displacement / action_range, a planner action needs |displacement| > omega * action_range -- wider steps)
    scales = (0.02, 0.08, 0.35) if cfg.ac_space_type == "piecewise" else (0.05, 0.2, 0.5)
    if L > 12:
        scales = tuple(s / 3.0 for s in scales)
    rec = synthetic_record(E, L, D, nq, seed=len(name) + 100, n_exec_max=L, scales=scales)
    ac_type = (np.arange(E) * 7 + 1) % 5 if with_type else None
    rng = lambda: counter_rng(cfg.seed + T_KEY, cfg.env_id_total or E, cfg.env_id_base)
    want = reuse_transitions(as_out(rec, n_arm + (grip is not None), ac_type=ac_type), cfg, n_arm, rng(), max_reuse_data=R, grip_qpos_idx=grip)
    return cfg, n_arm, grip, R, rec, ac_type, rng, want


def _device(name, E=67, **kw):
    from mopa_rl_amd.rollout import reuse_transitions_device
    cfg, n_arm, grip, R, rec, ac_type, _, _ = _case(name, E)
    out = as_out(rec, n_arm + (grip is not None), device="cuda", ac_type=ac_type)
    return reuse_transitions_device(out, cfg, n_arm, max_reuse_data=R, grip_qpos_idx=grip, t=T_KEY, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_drawn_mode_equals_host_loop_with_counter_rng(name):
    """E = 67 (not a multiple of the four envs of a workgroup), n_exec covering 0, 1, 3, 4 .. L; the draws come from the device's RNG"""
    cfg, n_arm, grip, R, rec, _, rng, want = _case(name)
    tally = classify_draws(rec, cfg, n_arm, rng(), R, grip_qpos_idx=grip)
    print(name, tally)
    assert tally["kept"] == len(want) and tally["kept"] > 0 and tally["not_planner"] + tally["out_of_box"] > 0
    if R >= 15:
        assert tally["duplicate"] > 0
    if R == 64:
        assert int(rec["n_exec"].max()) > 64        # the draw count is clipped by R
    got = _device(name)
    assert int(got.count.cpu()[0]) == len(want) and got.cap == 67 * R
    _assert_same(got.to_list(), want, name)


class TableDraw:
    """rng object that replays one env's row of a pair table through the host loop: a (-1, -1) entry answers `start` with the
    value that makes the loop skip the draw (no room for a goal)"""

    def __init__(self, row, n_exec):
        self.it = iter(row)
        self.n, self.goal = int(n_exec), None

    def randint(self, low, high):
        if self.goal is not None:
            g, self.goal = self.goal, None
            return g
        s, g = (int(x) for x in next(self.it))
        if s < 0:
            return self.n - 1
        self.goal = g
        return s


def test_given_pairs_equal_host_loop_with_the_same_random_states():
    from mopa_rl_amd.rollout import draw_reuse_pairs, reuse_transitions
    name = "lift-d40-r15-grip"
    cfg, n_arm, grip, R, rec, ac_type, _, _ = _case(name)
    per_env = lambda e: np.random.RandomState(1000 * e + 2)
    pairs = draw_reuse_pairs(rec["n_exec"], R, per_env)
    host_out = as_out(rec, n_arm + 1, ac_type=ac_type)
    want = reuse_transitions(host_out, cfg, n_arm, per_env, max_reuse_data=R, grip_qpos_idx=grip)
    assert len(want) > 30
    _assert_same(_device(name, pairs=pairs).to_list(), want, "RandomState pairs")
    # a table with explicit repeats (the kernel's own dedup), blanks and entries out of range
    n_exec = rec["n_exec"]
    table = pairs.copy()
    big = np.where(n_exec > 3)[0]
    for e in big:
        table[e, 5] = table[e, 0]                                     # a repeat of draw 0 (whatever it is)
        table[e, 9] = (-1, -1)
    clean = table.copy()
    bad = [(-1, 2), (2, 2), (3, 1), (0, None), (None, None), (-1, 0), (1, 2 ** 31 - 1), (-2 ** 31, 1)]      # None: n_exec of the env
    for k, e in enumerate(big):
        s, g = bad[k % len(bad)]
        table[e, 3] = (n_exec[e] if s is None else s, n_exec[e] if g is None else g)
        clean[e, 3] = (-1, -1)
    small = np.where(n_exec <= 3)[0]
    table[small, 0] = (0, 1)                                          # envs that take no part, whatever their entries say
    want = reuse_transitions(host_out, cfg, n_arm, lambda e: TableDraw(clean[e], n_exec[e]), max_reuse_data=R, grip_qpos_idx=grip)
    assert 0 < len(want)
    _assert_same(_device(name, pairs=clean).to_list(), want, "table with blanks and repeats")
    import torch
    _assert_same(_device(name, pairs=torch.tensor(table, device="cuda")).to_list(), want, "table with out-of-range entries")
    nothing = _device(name, pairs=np.full_like(pairs, -1))
    assert int(nothing.count.cpu()[0]) == 0 and nothing.to_list() == []


def test_golden_fixture_of_the_reference_runner():
    """the run of test_gpu_rollout.py::test_reuse_data_relabelling_equals_reference: the draws of the reference's RandomState(1000 e + t)
    reach the device as a pair table; the device list is the host list bit for bit, and the fixture's at that test's tolerances"""
    import torch
    from test_gpu_rollout import GOLD, _load_state, _make
    from mopa_rl_amd.rollout import draw_reuse_pairs
    G = np.load(os.path.join(GOLD, "ref_py_rollout_push_reuse.npz"))
    E, T = G["ac"].shape[:2]
    env, ro = _make(G, E)
    n_checked = 0
    for t in range(T):
        _load_state(env, G["qpos_start"][:, t], G["ep_len_start"][:, t])
        ro.t = t
        out = ro.agent_step(torch.tensor(G["ac"][:, t], device=env.device), record=True)
        rs = lambda e: np.random.RandomState(1000 * e + t)
        want = ro.reuse_transitions(out, rs)
        got = ro.reuse_transitions_device(out, pairs=draw_reuse_pairs(out["record"]["n_exec"], 30, rs)).to_list()
        _assert_same(got, want, f"step {t}")
        sel = G["x_t"] == t
        assert [g["env"] for g in got] == list(G["x_env"][sel]), f"step {t}"
        assert [g["intra_steps"] for g in got] == list(G["x_intra"][sel]) and [g["done"] for g in got] == list(G["x_done"][sel])
        if len(got):
            np.testing.assert_allclose(np.array([g["ac"] for g in got]), G["x_ac"][sel], rtol=0, atol=1e-12, err_msg=f"step {t}: relabelled actions")
            np.testing.assert_allclose([g["rew"] for g in got], G["x_rew"][sel], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(np.array([g["ob"] for g in got]), G["x_ob"][sel], rtol=0, atol=1e-12)
            np.testing.assert_allclose(np.array([g["ob_next"] for g in got]), G["x_ob_next"][sel], rtol=0, atol=1e-12)
        n_checked += len(got)
    assert n_checked == len(G["x_env"]) and n_checked > 30
    ro.close()


def test_lift_rollout_drawn_mode_with_gripper_and_ac_type():
    """a real record: Lift (gripper entry), three agent steps with blocked straight lines in the second, the discrete head's ac_type"""
    import torch
    from mopa_rl_amd.kinematic_env import make_env
    from mopa_rl_amd.rollout import BatchMoPARollout
    env_name, E, T = "SawyerLiftObstacle-v0", 64, 3
    rng = np.random.default_rng(4)
    AC = rng.uniform(-1, 1, size=(E, T, 8)) * rng.choice([0.6, 0.9, 1.0], size=(E, T, 1))
    AC[: E // 2, 1, 1], AC[: E // 2, 1, 3] = 1.0, -1.0           # blocked straight lines: RRT-Connect queries
    TYPE = (np.abs(AC[:, :, :7]) > 0.7).any(axis=2).astype(np.int64)
    env = make_env(env_name, E, seed=12, max_episode_steps=1000)
    env.reset()
    ro = BatchMoPARollout(env, _cfg(env_name, timelimit=0.15, max_nodes=512, max_path=128, num_trials=10, discrete_action=True))
    assert ro.ac_dim == 8
    n = 0
    for t in range(T):
        out = ro.agent_step(torch.tensor(AC[:, t], device="cuda"), record=True, ac_type=torch.tensor(TYPE[:, t], device="cuda"))
        want = ro.reuse_transitions(out, counter_rng(ro.cfg.seed + ro.t, E), max_reuse_data=15)
        got = ro.reuse_transitions_device(out, max_reuse_data=15)
        assert got.ac.shape[1] == 8 and got.ac_type is not None
        got = got.to_list()
        _assert_same(got, want, f"step {t}")
        assert all(g["ac_type"] == int(TYPE[g["env"], t]) for g in got)
        n += len(got)
    assert n > 30
    ro.close()


def test_many_envs_cross_the_scans_chunks():
    """E = 4099: five chunks of the 1024-wide scan, the last with three envs; the last workgroup with three of its four waves"""
    cfg, n_arm, grip, R, rec, _, _, want = _case("push-d5-r15", 4099)
    got = _device("push-d5-r15", 4099)
    assert int(got.count.cpu()[0]) == len(want) > 4096
    assert np.array_equal(got.env[:len(want)].cpu().numpy(), [w["env"] for w in want])
    _assert_same(got.to_list(), want, "E = 4099")


def _sentinel_batch(rows, D, dof, with_type=False):
    """a ReuseBatch over buffers filled with 0xA5 bytes (+ the buffers)"""
    import torch
    from mopa_rl_amd.rollout import ReuseBatch

    def mk(*sh, dt=torch.float64):
        width = sh[-1] * torch.empty(0, dtype=dt).element_size()
        return torch.full(sh[:-1] + (width,), 0xA5, dtype=torch.uint8, device="cuda").view(dt)

    i32 = torch.int32
    return ReuseBatch(count=mk(1, dt=torch.int64), env=mk(rows, dt=i32), start=mk(rows, dt=i32), goal=mk(rows, dt=i32), ob=mk(rows, D), ac=mk(rows, dof),
                      rew=mk(rows), done=mk(rows, dt=torch.uint8), intra_steps=mk(rows, dt=i32), ob_next=mk(rows, D),
                      ac_type=mk(rows, dt=i32) if with_type else None)


COLUMNS = ("env", "start", "goal", "ob", "ac", "rew", "done", "intra_steps", "ob_next", "ac_type")


def _raw(batch):
    """every column's bytes"""
    return {k: getattr(batch, k).cpu().numpy().view(np.uint8).reshape(batch.cap, -1) for k in COLUMNS if getattr(batch, k) is not None}


def test_capacity_below_the_kept_count():
    from mopa_rl_amd.rollout import ReuseBatch
    name = "lift-d40-r15-grip"
    _, _, _, R, _, _, _, want = _case(name)
    K, rows = len(want), 67 * R
    full = _sentinel_batch(rows, 40, 8, True)
    assert _device(name, into=full) is full
    assert int(full.count.cpu()[0]) == K and 8 < K < rows
    raw_full = _raw(full)
    for k, v in raw_full.items():
        assert (v[K:] == 0xA5).all(), f"{k}: rows beyond the count were written"
    _assert_same(full.to_list(), want, "sentinel-filled buffers")
    for cap in (K - 1, K // 2, 1, 0):
        big = _sentinel_batch(K + 3, 40, 8, True)
        part = ReuseBatch(count=big.count, **{k: getattr(big, k)[:cap] for k in COLUMNS})
        _device(name, cap=cap, into=part)
        assert int(big.count.cpu()[0]) == K, "count is the true number kept, also beyond the capacity"
        for k, v in _raw(big).items():
            assert np.array_equal(v[:cap], raw_full[k][:cap]), f"cap {cap}: {k}"
            assert (v[cap:] == 0xA5).all(), f"cap {cap}: {k} written beyond the capacity"
        assert len(part.to_list()) == cap


def test_env_mask():
    import torch
    name = "lift-d40-r15-grip"
    _, _, _, _, _, _, _, want = _case(name)
    mask = np.random.default_rng(2).uniform(size=67) < 0.5
    sub = [w for w in want if mask[w["env"]]]
    assert 0 < len(sub) < len(want)
    _assert_same(_device(name, env_mask=torch.tensor(mask, device="cuda")).to_list(), sub, "bool mask")
    _assert_same(_device(name, env_mask=torch.tensor(mask.astype(np.uint8), device="cuda")).to_list(), sub, "byte mask")
    _assert_same(_device(name, env_mask=torch.ones(67, dtype=torch.bool, device="cuda")).to_list(), want, "mask of ones")
    assert _device(name, env_mask=torch.zeros(67, dtype=torch.bool, device="cuda")).to_list() == []


def test_two_runs_and_two_streams_write_the_same_bytes_without_reading_back():
    """the call only enqueues: it runs between two events on side streams with every output preallocated and torch's
    synchronisation check armed; nothing is read before the one explicit synchronise"""
    import torch
    from mopa_rl_amd.rollout import reuse_transitions_device
    name = "lift-d40-r15-grip"
    cfg, n_arm, grip, R, rec, ac_type, _, want = _case(name, 1031)
    out = as_out(rec, 8, device="cuda", ac_type=ac_type)
    batches = [_sentinel_batch(1031 * R, 40, 8, True) for _ in range(3)]
    call = lambda b: reuse_transitions_device(out, cfg, n_arm, max_reuse_data=R, grip_qpos_idx=grip, t=T_KEY, into=b)
    call(batches[0])                                   # (the first call of a record length uploads the discount table)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    events = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s, b in zip(streams, batches[1:]):
            with torch.cuda.stream(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                call(b)
                e1.record(s)
                events.append((e0, e1))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(e0.elapsed_time(e1) > 0.0 for e0, e1 in events)
    raws = [_raw(b) for b in batches]
    for other in raws[1:]:
        for k, v in raws[0].items():
            assert np.array_equal(v, other[k]), f"{k}: runs differ"
    assert [int(b.count.cpu()[0]) for b in batches] == [len(want)] * 3
    _assert_same(batches[2].to_list(), want, "side stream")
