"""Lean staging of a baked scene (k_is_valid_v5 copies to LDS only what its narrow phase reads there: geom records and types, the
moving geoms' geom ids, word 7 of the pair table's entries).  Tiles of 64 copies of ONE state, every third one a state with the
most kept static pairs of a pool of 4096 (tests/test_k1_axis_cull_gpu.py's recipe), the others uniform / near-init: every pair
class the pool reaches, the deferred portal ring and drains in the middle of a tile all read the trimmed LDS image.  Verdicts
and depths must equal the oracle's bit for bit, with and without want_min_dist."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = "SawyerPushObstacle-v0"


def _batch(pi, n_cu):
    from conftest import sample_states
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import default_qpos
    n = 36 * n_cu + 37                       # the lane-per-state threshold plus a ragged last tile
    tiles = (n + 63) // 64
    act = np.asarray(pi.ref_joint_pos_indexes)
    row = default_qpos(ENV, pi.model)
    pool = np.concatenate([sample_states(pi, 2048, 171, "uniform")[0], sample_states(pi, 2048, 172, "near")[0]])
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


@pytest.fixture(scope="module")
def case():
    import torch
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    pi = planner_inputs(ENV)
    args = (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    qa, row = _batch(pi, torch.cuda.get_device_properties(0).multi_processor_count)
    assert len(qa) % 64 != 0, "the last tile is meant to be ragged"
    ov, omd = O.OracleScene(*args).is_valid_batch(qa, row[None], samples_per_env=len(qa))
    assert 0 < ov.sum() < len(qa)
    return pi, args, qa, row, ov, omd


@pytest.mark.parametrize("want_min_dist", [False, True])
def test_lean_staging_crowded_tiles_equal_the_oracle_bitwise(case, want_min_dist):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    pi, args, qa, row, ov, omd = case
    dev = torch.device("cuda", 0)
    sc = _lib.Scene(*args, range_=pi.spec.range, seed=0, device=0)
    assert _lib.lib().mopa_scene_k1_baked(sc.handle) >= 1
    assert sc.valid_kernel(len(qa)) == "k_is_valid_v5"
    bp = BatchPlanner(sc)
    tq, tr = torch.from_numpy(qa).to(dev), torch.from_numpy(row[None].copy()).to(dev)
    r = bp.is_valid(tq, tr, samples_per_env=len(qa), want_min_dist=want_min_dist)
    torch.cuda.synchronize()
    v, md = r if want_min_dist else (r, None)
    assert np.array_equal(v.cpu().numpy(), ov), "verdicts differ from the oracle"
    if want_min_dist:
        assert np.array_equal(md.cpu().numpy().view(np.uint64), omd.view(np.uint64)), "depths differ from the oracle"
    sc.close()
