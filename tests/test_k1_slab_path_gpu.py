"""The baked K1 kernel's pose slab and cold walk, addressed as global memory (typed pointers behind the empty asms that keep the
walk's 98 store addresses out of the tile loop's registers), and the baked scenes' lean staging: the baked kernel, the generic
kernel (MOPA_K1_BAKED=0) and the CPU oracle on verdicts and want_min_dist depths, bit for bit.  Each kernel runs in a fresh child
process (MOPA_K1_BAKED and MOPA_VALID_KERNEL are read at scene creation; v5: the lane-per-state kernel from 64 states on, so
the batches of 1 and 63 states are the wave-per-state kernel's).  MOPA_K1_PAIR_TAIL_TILES is read per call:
  n1 .. n193   N = 1, 63, 64, 65, 129, 3 x 64 + 1 states, with every pull a pair of tiles (tail 0: one pair, a pair and a single
               tile of an odd count, two pairs the second of which ends in a tile of one lane) and with the default single-tile
               tail (every pull one tile)
  guard        N = 128: a plain tile, then a tile in which SOME lanes trip the sparse walk's guard (all joints zero; one joint at
               +-pi; a gripper slide at 0 in the state's env row) -- the cold dense walk then loads its inputs again and stores
               over what the sparse walk stored, for every lane of that tile; as a pair (second half) and as single tiles"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENV = "SawyerPushObstacle-v0"
SIZES = (1, 63, 64, 65, 129, 3 * 64 + 1)
CASES = tuple(f"n{n}" for n in SIZES) + ("guard",)
TAILS = ("0", "default")

CHILD = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mopa_rl_amd import _lib
from mopa_rl_amd.batch import BatchPlanner
from mopa_rl_amd.scene import planner_inputs
env, qfile, out = sys.argv[2], sys.argv[3], sys.argv[4]
pi = planner_inputs(env)
dev = torch.device("cuda", 0)
sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
bp = BatchPlanner(sc)
res = {"baked": np.array([_lib.lib().mopa_scene_k1_baked(sc.handle)]), "lane_kernel": np.array([sc.valid_kernel(64) == "k_is_valid_v5"])}
z = np.load(qfile)
for tail in z["tails"]:
    if tail == "default":
        os.environ.pop("MOPA_K1_PAIR_TAIL_TILES", None)
    else:
        os.environ["MOPA_K1_PAIR_TAIL_TILES"] = str(tail)
    for case in z["cases"]:
        qa, rows = torch.from_numpy(z[f"{case}_qa"]).to(dev), torch.from_numpy(z[f"{case}_rows"]).to(dev)
        spe = qa.shape[0] // rows.shape[0]
        v = bp.is_valid(qa, rows, samples_per_env=spe)
        v2, d = bp.is_valid(qa, rows, samples_per_env=spe, want_min_dist=True)
        torch.cuda.synchronize()
        res[f"{case}_{tail}_valid_md0"] = v.cpu().numpy(); res[f"{case}_{tail}_valid_md1"] = v2.cpu().numpy()
        res[f"{case}_{tail}_min_dist"] = d.cpu().numpy().view(np.uint64)
sc.close()
np.savez(out, **res)
"""


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_flags(pi, qa, rows):
    """the guard's flag per state, from the host run of the sparse walk (rows: one env row per state)"""
    from mopa_rl_amd import _lib
    q = rows.copy()
    q[:, np.asarray(pi.ref_joint_pos_indexes)] = qa
    out, flag = np.zeros((len(qa), len(pi.model.geom_type), 7)), np.zeros(len(qa), np.uint8)      # (at least [nmg][7])
    assert _lib.lib().mopa_k1_baked_fk_sparse_host(1, len(qa), _vp(np.ascontiguousarray(qa)), _vp(np.ascontiguousarray(q)), _vp(out), _vp(flag)) == 0
    return flag.astype(bool)


def _batches(pi):
    from conftest import sample_states
    from mopa_rl_amd.scene import default_qpos
    row = default_qpos(ENV, pi.model)
    mixed = lambda n, seed: np.ascontiguousarray(np.concatenate([sample_states(pi, n - n // 2, seed, "uniform")[0], sample_states(pi, n // 2, seed + 1, "near")[0]]))
    qa = {f"n{n}": mixed(n, 100 + n) for n in SIZES}
    rows = {f"n{n}": row[None].copy() for n in SIZES}
    # the guard batch: one env row per state (samples_per_env = 1), the second tile's lanes in turn zero / +-pi / slide at 0 / plain
    g = mixed(128, 41)
    gr = np.repeat(row[None], 128, axis=0)
    m = pi.model
    slides = [int(m.jnt_qposadr[m.joint_name2id(nm)]) for nm in ("rc_close", "lc_close") if nm in m.jnt_names]
    assert slides, "the Push scene has gripper slides in its env row"
    for lane in range(64):
        s, kind = 64 + lane, lane % 4
        if kind == 0:
            g[s] = 0.0
        elif kind == 1:
            g[s, (lane // 4) % g.shape[1]] = np.pi if (lane // 4) % 2 == 0 else -np.pi
        elif kind == 2:
            gr[s, slides[(lane // 4) % len(slides)]] = 0.0
    flags = _host_flags(pi, g, gr)
    assert not flags[:64].any(), "the first tile is meant to stay on the sparse walk"
    assert 0 < np.count_nonzero(flags[64:]) < 64, "the guard is meant to trip in some lanes of the second tile only"
    qa["guard"], rows["guard"] = g, gr
    return qa, rows


def _run(tmp_path, qfile, baked):
    out = tmp_path / f"k1_slab_{baked}.npz"
    env = dict(os.environ, MOPA_K1_BAKED=str(baked), MOPA_VALID_KERNEL="v5")
    env.pop("MOPA_K1_PAIR_TAIL_TILES", None)
    subprocess.run([sys.executable, "-c", CHILD, ROOT, ENV, str(qfile), str(out)], env=env, check=True, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every batch through the generic and the baked kernel, one child process each; the oracle's answers, once"""
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    pi = planner_inputs(ENV)
    qa, rows = _batches(pi)
    tmp = tmp_path_factory.mktemp("k1_slab")
    qfile = tmp / "batches.npz"
    np.savez(qfile, cases=np.array(CASES), tails=np.array(TAILS), **{f"{c}_qa": qa[c] for c in CASES}, **{f"{c}_rows": rows[c] for c in CASES})
    g, b = _run(tmp, qfile, 0), _run(tmp, qfile, 1)
    assert int(g["baked"][0]) == 0 and int(b["baked"][0]) >= 1, "the bench scene did not select its baked instantiation"
    assert bool(g["lane_kernel"][0]) and bool(b["lane_kernel"][0]), "64 states did not go to the lane-per-state kernel"
    orc = O.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    ref = {c: orc.is_valid_batch(qa[c], rows[c], samples_per_env=len(qa[c]) // len(rows[c])) for c in CASES}
    return g, b, ref


@pytest.mark.parametrize("want_min_dist", [False, True])
def test_slab_path_baked_generic_oracle_bitwise(runs, want_min_dist):
    g, b, ref = runs
    md = int(want_min_dist)
    for c in CASES:
        ov, omd = ref[c]
        for tail in TAILS:
            key = f"{c}_{tail}_valid_md{md}"
            assert np.array_equal(g[key], b[key]), f"baked and generic kernels differ: {key}"
            assert np.array_equal(b[key], ov), f"{key}: verdicts differ from the oracle"
            if want_min_dist:
                key = f"{c}_{tail}_min_dist"
                assert np.array_equal(g[key], b[key]), f"baked and generic kernels differ: {key}"
                assert np.array_equal(b[key], omd.view(np.uint64)), f"{key}: depths differ from the oracle"
    assert 0 < ref["guard"][0].sum() < 128 or 0 < ref["n193"][0].sum() < 193, "neither verdict occurs in the batches"
