"""Host side of the device relabelling (mopa_rl_amd/rollout.py::reuse_transitions_device): the counter-RNG draw rule, the pair
table `draw_reuse_pairs` hands to the device, the synthetic record of the GPU tests, the C ABI's argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from reuse_ref import CounterDraw, as_out, classify_draws, counter_rng, reuse_stream, rng_key, rng_uniform_k, synthetic_record


def test_counter_draw_stays_in_range():
    for L in (4, 5, 12, 70, 257):
        d = CounterDraw(1234, reuse_stream(64, L))
        for _ in range(200):
            start = d.randint(low=0, high=L - 1)
            goal = d.randint(low=start + 1, high=L)
            assert 0 <= start < goal < L
    # the two ends of the uniform's range, through the same expression
    for u, want in ((0.0, 3), (1.0 - 2.0 ** -53, 8)):
        assert 3 + min(int(u * 6), 5) == want
    assert 0.0 <= rng_uniform_k(rng_key(0, 0), 0) < 1.0
    # a one-wide range has one value
    assert CounterDraw(5, 7).randint(low=3, high=4) == 3


def test_counter_draw_uses_counters_2i_and_2i_plus_1():
    key = rng_key(99, reuse_stream(10, 4))
    d, L = CounterDraw(99, reuse_stream(10, 4)), 9
    for i in range(6):
        start = d.randint(0, L - 1)
        goal = d.randint(start + 1, L)
        s = min(int(rng_uniform_k(key, 2 * i) * (L - 1)), L - 2)
        g = s + 1 + min(int(rng_uniform_k(key, 2 * i + 1) * (L - 1 - s)), L - 2 - s)
        assert (start, goal) == (s, g)


def test_draws_depend_on_the_global_env_id_only():
    """two shards of 32 envs draw what the 64 unsharded envs draw"""
    from mopa_rl_amd.rollout import draw_reuse_pairs
    n_exec = np.random.default_rng(3).integers(0, 13, size=64)
    whole = draw_reuse_pairs(n_exec, 15, counter_rng(1234 + 7, 64))
    for base in (0, 32):
        shard = draw_reuse_pairs(n_exec[base:base + 32], 15, counter_rng(1234 + 7, 64, env_id_base=base))
        assert np.array_equal(shard, whole[base:base + 32])
    assert (whole[n_exec > 3][:, 0, 0] >= 0).all() and (whole[n_exec <= 3] == -1).all()


def _inline_draws(n_exec, R, rng):
    """the draw / skip logic of the host loop of `reuse_transitions`, written out"""
    table = np.full((len(n_exec), R, 2), -1, dtype=np.int32)
    for e in np.where(n_exec > 3)[0]:
        draw = rng(int(e)) if callable(rng) else rng
        L = int(n_exec[e])
        seen = set()
        for i in range(min(L, R)):
            start = draw.randint(low=0, high=L - 1)
            if start + 1 > L - 1:
                continue
            goal = draw.randint(low=start + 1, high=L)
            if (start, goal) in seen:
                continue
            seen.add((start, goal))
            table[e, i] = (start, goal)
    return table


@pytest.mark.parametrize("R", [1, 15, 64])
def test_draw_reuse_pairs_equals_the_host_loops_draws(R):
    from mopa_rl_amd.rollout import draw_reuse_pairs
    n_exec = np.random.default_rng(5).integers(0, 80 if R == 64 else 13, size=67)
    # one shared RandomState (the reference's global np.random), one per env, and the counter RNG
    got = draw_reuse_pairs(n_exec, R, np.random.RandomState(11))
    assert got.dtype == np.int32 and got.shape == (67, R, 2)
    assert np.array_equal(got, _inline_draws(n_exec, R, np.random.RandomState(11)))
    per_env = lambda e: np.random.RandomState(1000 * e + 2)
    assert np.array_equal(draw_reuse_pairs(n_exec, R, per_env), _inline_draws(n_exec, R, per_env))
    assert np.array_equal(draw_reuse_pairs(n_exec, R, counter_rng(8, 67)), _inline_draws(n_exec, R, counter_rng(8, 67)))
    import torch
    assert np.array_equal(draw_reuse_pairs(torch.tensor(n_exec), R, counter_rng(8, 67)), _inline_draws(n_exec, R, counter_rng(8, 67)))
    live = got[:, :, 0] >= 0
    assert live.any() and (got[live][:, 0] < got[live][:, 1]).all()
    assert (got[live][:, 1] < np.broadcast_to(n_exec[:, None], live.shape)[live]).all()


@pytest.mark.parametrize("env_name,n_arm,grip", [("SawyerPushObstacle-v0", 7, None), ("SawyerLiftObstacle-v0", 7, 7), ("PusherObstacle-v0", 4, None)])
def test_synthetic_record_reaches_every_outcome(env_name, n_arm, grip):
    """the record the GPU tests relabel makes a draw end each of the four ways, and the host function keeps what the tally keeps"""
    from mopa_rl_amd.rollout import RolloutConfig, reuse_transitions
    cfg = RolloutConfig.for_env(env_name)
    nq = n_arm + 2
    rec = synthetic_record(67, 12, 5, nq, seed=21)
    tally = classify_draws(rec, cfg, n_arm, counter_rng(cfg.seed, 67), 15, grip_qpos_idx=grip)
    assert min(tally.values()) >= 3, tally
    got = reuse_transitions(as_out(rec, n_arm + (grip is not None)), cfg, n_arm, counter_rng(cfg.seed, 67), max_reuse_data=15, grip_qpos_idx=grip)
    assert len(got) == tally["kept"]
    assert all(rec["n_exec"][g["env"]] > 3 for g in got)


def test_argument_errors_are_status_codes_before_any_launch():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    assert "mopa_reuse_batch" in _lib.EXPORTED_SYMBOLS

    def call(R=15, n_arm=7, dof=7, cap=10, buf=None):
        p = [buf] * 7
        return L.mopa_reuse_batch(4, 12, 5, 9, n_arm, dof, -1, *p, 0.05, 0.7, 14.0, 0.47, 3.2, 0.5, 0, buf, R, None, 0, 0, 0, cap, *([buf] * 12), None)

    for R in (0, -1, 65):
        assert call(R=R) == 1 and b"1..64" in L.mopa_last_error()
    assert call(n_arm=8, dof=7) == 1 and b"n_arm > dof" in L.mopa_last_error()
    assert call(cap=-1) == 1 and b"cap" in L.mopa_last_error()
    assert call() == 1 and b"null" in L.mopa_last_error()
    # (with every buffer named the size checks come next: still no launch)
    keep = (C.c_double * 8)()
    assert call(dof=9, buf=C.cast(keep, C.c_void_p)) == 1 and b"sizes" in L.mopa_last_error()


def test_device_form_refuses_what_it_cannot_do():
    """no CPU fallback (a record on the host is an error, not a slow path); the IK action space raises as the host function documents"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.rollout import RolloutConfig, reuse_transitions_device
    out = as_out(synthetic_record(8, 12, 5, 9, seed=1), 7)
    with pytest.raises(NotImplementedError, match="IK action space"):
        reuse_transitions_device(out, RolloutConfig(use_ik_target=True), 7)
    with pytest.raises(_lib.MopaError, match="not on a GPU"):
        reuse_transitions_device(out, RolloutConfig(), 7)
