"""Axis extents in the baked pass A on the GPU: the axis table shares the wave's LDS with the entry buffer, whose capacity it
lowers (Push: 896 -> 512 entries, with depths 768 -> 384).  Tiles made of 64 copies of ONE state build 64 entries per kept pair,
so the states the host predicate finds with the most kept static pairs overflow the buffer and are drained in the middle of
their tile, several times; others alternate uniform / near-init.  N = 36 n_cu + 37: the lane-per-state threshold plus a ragged
last tile.  Verdicts and depths must equal the oracle's bit for bit, with and without want_min_dist."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = "SawyerPushObstacle-v0"


def _batch(pi, n_cu):
    from conftest import sample_states
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import default_qpos
    n = 36 * n_cu + 37
    tiles = (n + 63) // 64
    act = np.asarray(pi.ref_joint_pos_indexes)
    row = default_qpos(ENV, pi.model)
    pool = np.concatenate([sample_states(pi, 2048, 71, "uniform")[0], sample_states(pi, 2048, 72, "near")[0]])
    q = np.repeat(row[None], len(pool), axis=0)
    q[:, act] = pool
    L = _lib.lib()
    n_ent = C.c_int32(0)
    assert L.mopa_k1_baked_static_host(1, 0, None, None, None, None, None, C.byref(n_ent)) == 0
    kn, ko = np.zeros((len(pool), n_ent.value), np.uint8), np.zeros((len(pool), n_ent.value), np.uint8)
    axis = np.zeros((len(pool), len(pi.model.geom_type), 3), np.float32)      # (at least [nmg][3])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mopa_k1_baked_static_host(1, len(pool), vp(np.ascontiguousarray(pool)), vp(q), vp(kn), vp(ko), vp(axis), None) == 0
    kept = (kn == 1).sum(axis=1)
    pick = np.empty(tiles, np.int64)
    crowded = np.argsort(-kept, kind="stable")[: len(pick[0::3])]
    assert kept[crowded].min() >= 8, "no state with 8 kept static pairs: 64 copies would not overflow a 512-entry buffer"
    pick[0::3] = crowded
    pick[1::3] = np.arange(len(pick[1::3]))                    # uniform states
    pick[2::3] = 2048 + np.arange(len(pick[2::3]))             # near-init states
    return np.ascontiguousarray(np.repeat(pool[pick], 64, axis=0)[:n]), row


def test_crowded_tiles_equal_the_oracle_bitwise():
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    pi = planner_inputs(ENV)
    args = (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    dev = torch.device("cuda", 0)
    sc = _lib.Scene(*args, range_=pi.spec.range, seed=0, device=0)
    assert _lib.lib().mopa_scene_k1_baked(sc.handle) >= 1
    qa, row = _batch(pi, torch.cuda.get_device_properties(0).multi_processor_count)
    n = len(qa)
    assert n % 64 != 0, "the last tile is meant to be ragged"
    ov, omd = O.OracleScene(*args).is_valid_batch(qa, row[None], samples_per_env=n)
    assert 0 < ov.sum() < n
    bp = BatchPlanner(sc)
    tq, tr = torch.from_numpy(qa).to(dev), torch.from_numpy(row[None].copy()).to(dev)
    v = bp.is_valid(tq, tr, samples_per_env=n)
    v2, md = bp.is_valid(tq, tr, samples_per_env=n, want_min_dist=True)
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), ov), "verdicts differ from the oracle"
    assert np.array_equal(v2.cpu().numpy(), ov), "verdicts (with depths) differ from the oracle"
    assert np.array_equal(md.cpu().numpy().view(np.uint64), omd.view(np.uint64)), "depths differ from the oracle"
    sc.close()
