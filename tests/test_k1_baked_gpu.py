"""Baked K1 (k_is_valid_v5 on a scene compiled into the kernel) vs the generic instantiation on the same library: identical
verdict bytes and depth bits on the bench batch and on states bisected to the contact threshold.  Each side runs in a fresh
child process (MOPA_K1_BAKED is read at scene creation)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENV = "SawyerPushObstacle-v0"

CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mopa_rl_amd import _lib
from mopa_rl_amd.batch import BatchPlanner
from mopa_rl_amd.scene import planner_inputs
import bench
env, qfile, out = sys.argv[2], sys.argv[3], sys.argv[4]
pi = planner_inputs(env)
dev = torch.device("cuda", 0)
sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
bp = BatchPlanner(sc)
res = {"baked": np.array([_lib.lib().mopa_scene_k1_baked(sc.handle)])}
E, S = 4096, 256                                        # the bench batch
qa, rows = bench.make_inputs(torch, pi, E, S, 0, dev)
for md in (False, True):
    r = bp.is_valid(qa, rows, samples_per_env=S, want_min_dist=md)
    v, d = (r if md else (r, None))
    torch.cuda.synchronize()
    res[f"valid_md{int(md)}"] = v.cpu().numpy()
    if md:
        res["min_dist"] = d.cpu().numpy().view(np.uint64)
z = np.load(qfile)                                      # threshold-bisected states
qb, rb = torch.from_numpy(z["qa"]).to(dev), torch.from_numpy(z["rows"]).to(dev)
v, d = bp.is_valid(qb, rb, samples_per_env=z["qa"].shape[0] // z["rows"].shape[0], want_min_dist=True)
res["bis_valid_md"] = v.cpu().numpy(); res["bis_min_dist"] = d.cpu().numpy().view(np.uint64)
res["bis_valid"] = bp.is_valid(qb, rb, samples_per_env=z["qa"].shape[0] // z["rows"].shape[0]).cpu().numpy()
np.savez(out, **res)
"""


def _bisected(tmp_path):
    """states on both sides of the contact threshold: up to 64 (valid, invalid) pairs bisected 30 times with the CPU oracle,
    repeated to a batch the lane-per-state kernel serves"""
    from mopa_rl_amd.scene import default_qpos, planner_inputs
    from oracle import oracle as O
    pi = planner_inputs(ENV)
    orc = O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    rng = np.random.default_rng(5)
    row = default_qpos(ENV, pi.model)
    n = 512
    qa = rng.uniform(pi.jnt_minimum, pi.jnt_maximum, size=(n, len(pi.jnt_minimum)))
    v, _ = orc.is_valid_batch(qa, row[None], samples_per_env=n)
    good, bad = qa[v == 1][:64], qa[v == 0][:64]
    k = min(len(good), len(bad))
    lo, hi = good[:k].copy(), bad[:k].copy()
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        vm, _ = orc.is_valid_batch(mid, row[None], samples_per_env=k)
        ok = vm == 1
        lo[ok], hi[~ok] = mid[ok], mid[~ok]
    n_st = 16384                                        # enough states for the lane-per-state kernel (>= 36 per CU)
    states = np.tile(np.concatenate([lo, hi]), (n_st // (2 * k) + 1, 1))[:n_st]
    f = tmp_path / "bisected.npz"
    np.savez(f, qa=np.ascontiguousarray(states), rows=row[None].copy())
    return f


def _run(tmp_path, qfile, baked):
    out = tmp_path / f"k1_{baked}.npz"
    env = dict(os.environ, MOPA_K1_BAKED=str(baked))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, ENV, str(qfile), str(out)], env=env, check=True, timeout=600)
    return np.load(out)


def test_baked_equals_generic_bitwise(tmp_path):
    qfile = _bisected(tmp_path)
    g, b = _run(tmp_path, qfile, 0), _run(tmp_path, qfile, 1)
    assert int(g["baked"][0]) == 0 and int(b["baked"][0]) >= 1, "the bench scene did not select its baked instantiation"
    for key in ("valid_md0", "valid_md1", "min_dist", "bis_valid", "bis_valid_md", "bis_min_dist"):
        assert np.array_equal(g[key], b[key]), key


def test_other_scenes_select_the_generic_kernel():
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(ENV)
    args = (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    L = _lib.lib()
    sc = _lib.Scene(*args, range_=pi.spec.range, device=0)
    assert L.mopa_scene_k1_baked(sc.handle) >= 1
    full = sc.full()                                    # sibling with the full pair list
    assert full is not sc and L.mopa_scene_k1_baked(full.handle) == 0
    m = pi.model
    g = 0
    old = m.geom_size[g, 0]
    try:                                                # one constant moved by one ULP
        m.geom_size[g, 0] = np.nextafter(old, np.inf)
        sp = _lib.Scene(*args, range_=pi.spec.range, device=0)
        assert L.mopa_scene_k1_baked(sp.handle) == 0
        sp.close()
    finally:
        m.geom_size[g, 0] = old
    sc.close()
