"""Resident pairs of the baked K1 kernel on the GPU: a Push batch just above the lane-kernel threshold with a partial last tile,
against the CPU oracle and against the generic kernel (fresh child process, MOPA_K1_BAKED=0) -- verdict bytes and depth bits;
two launches back to back (the self-resetting tile counter comes back to zero); a device-side state count."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENV = "SawyerPushObstacle-v0"
SPE = 64

CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mopa_rl_amd import _lib
from mopa_rl_amd.batch import BatchPlanner
from mopa_rl_amd.scene import planner_inputs
env, qfile, out = sys.argv[2], sys.argv[3], sys.argv[4]
pi = planner_inputs(env)
dev = torch.device("cuda", 0)
sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
bp = BatchPlanner(sc)
z = np.load(qfile)
qa, rows = torch.from_numpy(z["qa"]).to(dev), torch.from_numpy(z["rows"]).to(dev)
v0 = bp.is_valid(qa, rows, samples_per_env=int(z["spe"]))
v1, d1 = bp.is_valid(qa, rows, samples_per_env=int(z["spe"]), want_min_dist=True)
torch.cuda.synchronize()
np.savez(out, baked=np.array([_lib.lib().mopa_scene_k1_baked(sc.handle)]), kernel=np.array([sc.valid_kernel(qa.shape[0])]),
         valid=v0.cpu().numpy(), valid_md=v1.cpu().numpy(), min_dist=d1.cpu().numpy().view(np.uint64))
"""


@pytest.fixture(scope="module")
def batch():
    """The batch, the oracle's verdicts / depths and the composition facts, computed once."""
    import torch
    from conftest import sample_states
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    from test_k1_baked_fk_host import _states
    from test_k1_resident_host import committed_resident, pair_index
    import bake_k1_scenes as B
    pi = planner_inputs(ENV)
    m = pi.model
    args = (m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    thr = pi.spec.contact_threshold
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 36 * cus + 64 + 37                               # just above the lane-kernel threshold; the last tile holds 37 states
    n_lim = 256
    act = np.asarray(pi.ref_joint_pos_indexes)
    qu, row = sample_states(pi, (N - n_lim) // 2, 31, "uniform")
    qn, _ = sample_states(pi, N - n_lim - len(qu), 32, "near")
    ql = _states(pi, 4 * n_lim, 33)[:n_lim][:, act]      # its first quarter: every joint at a limit, then one ULP past it
    qa = np.ascontiguousarray(np.concatenate([qu, ql, qn]))
    assert len(qa) == N
    E = (N + SPE - 1) // SPE
    rng = np.random.default_rng(34)
    rows = np.repeat(row, E, axis=0)
    for name in ("rc_close", "lc_close"):
        j = m.joint_name2id(name)
        a, (r0, r1) = int(m.jnt_qposadr[j]), m.jnt_range[j]
        rows[:, a] = rng.uniform(r0, r1, size=E)
    orc = O.OracleScene(*args)
    ov, omd = orc.is_valid_batch(qa, rows, samples_per_env=SPE)
    # composition, on the oracle: per state the non-ignored pairs at or under the threshold, the resident pair's distance, pass A's sphere test
    ex = _lib.k1_export(*args)
    o = B.hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + ex["nmg"]]]
    res = committed_resident()
    M, K, s1, s2 = res[0][:4]
    ridx = pair_index(m, mg[s1], mg[s2])
    ign = set(tuple(p) for p in pi.ignored_contacts)
    live = np.array([(min(int(m.geom_mjid[a]), int(m.geom_mjid[b])), max(int(m.geom_mjid[a]), int(m.geom_mjid[b]))) not in ign for a, b in m.pair_geom])
    tab = ex["tab"].astype("<i4")
    n5 = (len(tab) - 3 * ex["nmg"]) // 8
    e = int(tab[8 * n5 + ex["nmg"] + 2 * M]) + K
    rs2 = tab[8 * e + 3: 8 * e + 4].view("<f4")[0]
    only = np.zeros(N, bool)
    near_miss = np.zeros(N, bool)
    for i in range(N):
        q = rows[i // SPE].copy()
        q[act] = qa[i]
        pd = orc.pair_dist(q)
        viol = live & (pd <= thr)
        only[i] = viol[ridx] and viol.sum() == 1
        c = orc.fk(q)[0][[mg[s1], mg[s2]]].astype(np.float32)
        d = c[0] - c[1]
        kept = not ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] > rs2)
        near_miss[i] = kept and not viol[ridx]
    return {"pi": pi, "N": N, "qa": qa, "rows": rows, "ov": ov, "omd": omd, "only": only, "near_miss": near_miss}


@pytest.fixture(scope="module")
def gpu(batch):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    pi = batch["pi"]
    dev = torch.device("cuda", 0)
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    yield sc, BatchPlanner(sc), torch.from_numpy(batch["qa"]).to(dev), torch.from_numpy(batch["rows"]).to(dev)
    sc.close()


def test_batch_composition(batch):
    """the batch exercises what the change touches: states only the resident pair makes invalid, states in which it passes the
    sphere test and does not violate, and valid states -- at least a tile's worth of each"""
    assert np.count_nonzero(batch["only"]) >= 64
    assert np.count_nonzero(batch["near_miss"]) >= 64
    assert np.count_nonzero(batch["ov"] == 1) >= 64


def test_verdicts_and_depths_equal_the_oracle(batch, gpu):
    import torch
    from mopa_rl_amd import _lib
    sc, bp, qa, rows = gpu
    assert _lib.lib().mopa_scene_k1_baked(sc.handle) >= 1
    assert sc.valid_kernel(batch["N"]) == "k_is_valid_v5"
    v0 = bp.is_valid(qa, rows, samples_per_env=SPE)
    v1, d1 = bp.is_valid(qa, rows, samples_per_env=SPE, want_min_dist=True)
    torch.cuda.synchronize()
    assert np.array_equal(v0.cpu().numpy(), batch["ov"])
    assert np.array_equal(v1.cpu().numpy(), batch["ov"])
    assert np.array_equal(d1.cpu().numpy().view(np.uint64), batch["omd"].view(np.uint64))


def test_baked_equals_generic_bitwise(batch, gpu, tmp_path):
    qfile, out = tmp_path / "batch.npz", tmp_path / "generic.npz"
    np.savez(qfile, qa=batch["qa"], rows=batch["rows"], spe=np.array(SPE))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, ENV, str(qfile), str(out)], env=dict(os.environ, MOPA_K1_BAKED="0"), check=True, timeout=300)
    g = np.load(out)
    assert int(g["baked"][0]) == 0 and str(g["kernel"][0]) == "k_is_valid_v5"
    _, bp, qa, rows = gpu
    v0 = bp.is_valid(qa, rows, samples_per_env=SPE)
    v1, d1 = bp.is_valid(qa, rows, samples_per_env=SPE, want_min_dist=True)
    assert np.array_equal(v0.cpu().numpy(), g["valid"])
    assert np.array_equal(v1.cpu().numpy(), g["valid_md"])
    assert np.array_equal(d1.cpu().numpy().view(np.uint64), g["min_dist"])


def test_back_to_back_launches(batch, gpu):
    """the second launch finds the self-resetting tile counter at zero: same output, every state written"""
    import torch
    _, bp, qa, rows = gpu
    a = torch.full((batch["N"],), 7, dtype=torch.uint8, device=qa.device)
    b = torch.full((batch["N"],), 7, dtype=torch.uint8, device=qa.device)
    bp.is_valid(qa, rows, samples_per_env=SPE, out=a)
    bp.is_valid(qa, rows, samples_per_env=SPE, out=b)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), batch["ov"]) and np.array_equal(b.cpu().numpy(), batch["ov"])


def test_device_side_count(batch, gpu):
    """n_dev < N (still a count the lane-per-state kernel serves, ending inside a tile): the prefix's verdicts, the rest untouched"""
    import torch
    _, bp, qa, rows = gpu
    N = batch["N"]
    n = N - 64 - 11
    out = torch.full((N,), 7, dtype=torch.uint8, device=qa.device)
    bp.is_valid(qa, rows, samples_per_env=SPE, out=out, n_dev=torch.tensor([n], dtype=torch.int64, device=qa.device))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], batch["ov"][:n])
    assert np.all(got[n:] == 7)
