"""Pair drain of the baked K1 kernel on the GPU (DESIGN.md "Pair drain"): a wave walks and culls two consecutive 64-state tiles
and evaluates the entries of both in one narrow-phase drain.  One Push batch, built and screened on the CPU, whose tiles are
laid out so that every way the two halves could be confused shows in the verdict bytes; every comparison is bit for bit against
the CPU oracle, no tolerance.  The depth-reporting instantiations stay at one tile per drain: their bytes must equal the generic
kernel's (and the oracle's).

Layout (tiles of 64 states, env row t for tile t: samples_per_env = 64):
  tiles 0-3    (64 states only the resident pair makes invalid, 64 free states), then the reverse
  tiles 4-9    crowded pairs: 64 copies of ONE state per tile, chosen so that one tile alone stays under the entry buffer's drain
               mark and the two of a pair exceed it -- a drain in the middle of the second half, over entries of both halves
  tiles 11, 13 second halves: states in which a cylinder (convex-class) pair violates and no cheaper class does
  the rest     uniform and near-init states; from tile 14 on every env row has its own gripper opening

The launch plan pulls the last tiles of a launch one at a time, one per wave -- which is every tile of a batch this small.  The tests
therefore run with MOPA_K1_PAIR_TAIL_TILES=0 (every pull a pair; the knob is read per call), and test_single_tile_tail covers the
plan's own tail, an odd one and a tail of one tile.
"""
import ctypes as C
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
N_SPECIAL = 14          # tiles whose env row keeps the default values (their states are screened on that row)
G_CYLINDER = 5

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


@pytest.fixture(autouse=True)
def _pairs_everywhere(monkeypatch):
    monkeypatch.setenv("MOPA_K1_PAIR_TAIL_TILES", "0")


def drain_plan(sc, n, want_md):
    """(tiles per drain, entry capacity) of the launch plan for n states"""
    from mopa_rl_amd import _lib
    t, cap = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().mopa_scene_k1_drain_plan(sc.handle, int(n), int(want_md), C.byref(t), C.byref(cap)))
    return t.value, cap.value


@pytest.fixture(scope="module")
def scene():
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(ENV)
    sc = _lib.Scene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold, range_=pi.spec.range, seed=0, device=0)
    yield pi, sc
    sc.close()


def entry_counts(pi, ex, res, pool, q, kept_static, res_bad):
    """Entries per state that pass A / pass B of the verdict-only baked kernel build (the model of the kernel's FP32 cull): geoms in
    slot order; moving partners by the sphere test on the FP32 centres (a partner inside the inscribed-ball bound makes the lane
    dead from there on), static partners as the host predicate of the kernel's own arithmetic reports them (kept_static), planes by
    the plane test; the resident pair builds none, and a state it makes invalid builds none at all."""
    from oracle import oracle as O
    m = pi.model
    args = (m, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    orc = O.OracleScene(*args)
    import bake_k1_scenes as B
    nmg = ex["nmg"]
    o = B.hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + nmg]]
    tab = np.ascontiguousarray(ex["tab"]).astype("<i4")
    n5 = (len(tab) - 3 * nmg) // 8
    cnt = tab[8 * n5: 8 * n5 + nmg]
    padr = [int(tab[8 * n5 + nmg + 2 * M]) for M in range(nmg)]
    f = tab[: 8 * n5].view("<f4").reshape(n5, 8)
    flags = tab[: 8 * n5].reshape(n5, 8)[:, 7]
    resident = {(r[0], r[1]) for r in res}
    out = np.zeros(len(pool), np.int64)
    f32 = np.float32
    for i in range(len(pool)):
        if res_bad[i]:
            continue
        cen = orc.fk(q[i])[0][mg].astype(np.float32)
        n, dead = 0, False
        for M in range(nmg):
            n_mov, n_stat, n_pl = int(cnt[M]) & 0xff, (int(cnt[M]) >> 8) & 0xff, (int(cnt[M]) >> 16) & 0xff
            keep, deep = 0, False
            for K in range(n_mov + n_stat + n_pl):
                if (M, K) in resident:
                    continue
                e = padr[M] + K
                if K < n_mov:
                    d = cen[M] - cen[(int(flags[e]) >> 14) & 0xff]
                    d2 = f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])
                    deep = deep or (tab[8 * e] != 0 and d2 < f[e, 0])
                    keep += not (d2 > f[e, 3])
                elif K < n_mov + n_stat:
                    keep += int(kept_static[i, e] == 1)
                else:
                    d = cen[M] - f[e, 0:3]
                    keep += not (f32(f32(d[0] * f[e, 4]) + f32(d[1] * f[e, 5])) + f32(d[2] * f[e, 6]) > f[e, 3])
            dead = dead or deep
            if not dead:
                n += keep
        out[i] = n
    return out


@pytest.fixture(scope="module")
def batch(scene):
    """The batch, the oracle's verdicts / depths and the composition facts, computed once on the CPU."""
    import torch
    from conftest import sample_states
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import default_qpos
    from oracle import oracle as O
    from test_k1_resident_host import committed_resident, pair_index
    import bake_k1_scenes as B
    pi, sc = scene
    m = pi.model
    thr = pi.spec.contact_threshold
    args = (m, pi.passive_joint_idx, pi.ignored_contacts, thr)
    orc = O.OracleScene(*args)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lane_min = max(64, 36 * cus)                     # k1_lane_min: the smallest batch the lane-per-state kernel accepts
    tiles = (lane_min + 63) // 64 + 4
    tiles += tiles % 2                               # the pool: an even number of tiles; the cases take prefixes of it
    assert tiles >= N_SPECIAL + 8
    act = np.asarray(pi.ref_joint_pos_indexes)
    row = default_qpos(ENV, m)

    # ---- the screening pool, on the default env row
    pool = np.concatenate([sample_states(pi, 3072, 41, "uniform")[0], sample_states(pi, 3072, 42, "near")[0]])
    q = np.repeat(row[None], len(pool), axis=0)
    q[:, act] = pool
    ex = _lib.k1_export(*args)
    o = B.hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + ex["nmg"]]]
    res = committed_resident()
    ridx = pair_index(m, mg[res[0][2]], mg[res[0][3]])
    ign = set(tuple(p) for p in pi.ignored_contacts)
    live = np.array([(min(int(m.geom_mjid[a]), int(m.geom_mjid[b])), max(int(m.geom_mjid[a]), int(m.geom_mjid[b]))) not in ign for a, b in m.pair_geom])
    convex = np.array([G_CYLINDER in (int(m.geom_type[a]), int(m.geom_type[b])) and 0 not in (int(m.geom_type[a]), int(m.geom_type[b]))
                       and 2 not in (int(m.geom_type[a]), int(m.geom_type[b])) for a, b in m.pair_geom])   # cylinder with capsule / cylinder / box
    viol = np.array([live & (orc.pair_dist(r) <= thr) for r in q])
    res_bad = viol[:, ridx]
    res_only = res_bad & (viol.sum(axis=1) == 1)
    free = ~viol.any(axis=1)
    convex_only = (viol & convex).any(axis=1) & ~(viol & ~convex).any(axis=1)

    L = _lib.lib()
    n_ent = C.c_int32(0)
    assert L.mopa_k1_baked_static_host(1, 0, None, None, None, None, None, C.byref(n_ent)) == 0
    kn, ko = np.zeros((len(pool), n_ent.value), np.uint8), np.zeros((len(pool), n_ent.value), np.uint8)
    axis = np.zeros((len(pool), len(m.geom_type), 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mopa_k1_baked_static_host(1, len(pool), vp(np.ascontiguousarray(pool)), vp(q), vp(kn), vp(ko), vp(axis), None) == 0
    ents = entry_counts(pi, ex, res, pool, q, kn, res_bad)

    # ---- the entry buffer of the verdict-only launch, as the launch plan sizes it; a drain runs once more than cap - 64 entries wait
    tpd, cap = drain_plan(sc, 64 * tiles, False)
    mark = cap - 64
    one = 64 * ents                                   # entries of a tile made of 64 copies of the state
    crowded = np.flatnonzero((one <= mark) & (2 * one > mark))
    crowded = crowded[np.argsort(-ents[crowded], kind="stable")]

    # ---- the layout
    sel = np.empty(tiles * 64, np.int64)
    rest = np.flatnonzero(~res_only & ~convex_only)
    sel[:] = np.resize(rest, len(sel))
    i_res, i_free, i_cvx = np.flatnonzero(res_only), np.flatnonzero(free), np.flatnonzero(convex_only)
    facts = {"n_res_only": len(i_res), "n_free": len(i_free), "n_convex_only": len(i_cvx), "n_crowded": len(crowded), "cap": cap, "tpd": tpd,
             "tpd_md": drain_plan(sc, 64 * tiles, True)[0]}
    if len(i_res) and len(i_free):
        sel[0:64] = np.resize(i_res, 64); sel[64:128] = np.resize(i_free, 64)
        sel[128:192] = np.resize(i_free[::-1], 64); sel[192:256] = np.resize(i_res[::-1], 64)
    pairs = []
    for k in range(3):
        if len(crowded) >= 2:
            a, b = crowded[(2 * k) % len(crowded)], crowded[(2 * k + 1) % len(crowded)]
            sel[64 * (4 + 2 * k): 64 * (5 + 2 * k)] = a
            sel[64 * (5 + 2 * k): 64 * (6 + 2 * k)] = b
            pairs.append((int(one[a]), int(one[b])))
    facts["crowded_pairs"] = pairs
    for t in (11, 13):
        if len(i_cvx):
            sel[64 * t + 5: 64 * t + 5 + min(len(i_cvx), 32)] = i_cvx[:32]
    qa = np.ascontiguousarray(pool[sel])
    rows = np.repeat(row[None], tiles, axis=0)
    rng = np.random.default_rng(43)
    for name in ("rc_close", "lc_close"):
        j = m.joint_name2id(name)
        a, (r0, r1) = int(m.jnt_qposadr[j]), m.jnt_range[j]
        rows[N_SPECIAL:, a] = rng.uniform(r0, r1, size=tiles - N_SPECIAL)
    ov, omd = orc.is_valid_batch(qa, rows, samples_per_env=SPE)
    return {"pi": pi, "tiles": tiles, "lane_min": lane_min, "qa": qa, "rows": rows, "ov": ov, "omd": omd, "facts": facts, "sel": sel,
            "res_only": res_only, "free": free, "convex_only": convex_only}


@pytest.fixture(scope="module")
def gpu(scene, batch):
    import torch
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    _, sc = scene
    dev = torch.device("cuda", 0)
    assert _lib.lib().mopa_scene_k1_baked(sc.handle) >= 1, "the baked kernel is not selected"
    return sc, BatchPlanner(sc), torch.from_numpy(batch["qa"]).to(dev), torch.from_numpy(batch["rows"]).to(dev)


def _verdicts(bp, qa, rows, n, **kw):
    import torch
    out = torch.full((len(qa),), 7, dtype=torch.uint8, device=qa.device)
    bp.is_valid(qa[:n], rows, samples_per_env=SPE, out=out[:n], **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def drain_plan_md_is_one(batch):
    return batch["facts"]["tpd_md"] == 1


def test_batch_composition(batch):
    """the screens found what the layout needs; a crowded pair drains in the middle of its second half (CPU model of the entry counts)"""
    f = batch["facts"]
    assert f["n_res_only"] >= 1 and f["n_free"] >= 1, f
    assert f["n_convex_only"] >= 1, "no state in which only a cylinder pair violates"
    assert f["tpd"] == 2 and drain_plan_md_is_one(batch), "the verdict-only launch drains per two tiles, the depth-reporting one per tile"
    assert f["n_crowded"] >= 2 and len(f["crowded_pairs"]) == 3, f
    mark = f["cap"] - 64
    for a, b in f["crowded_pairs"]:
        assert a <= mark and b <= mark and a + b > mark, (a, b, f["cap"])
    sel = batch["sel"]
    assert batch["res_only"][sel[0:64]].all() and batch["free"][sel[64:128]].all()
    assert batch["free"][sel[128:192]].all() and batch["res_only"][sel[192:256]].all()
    assert batch["convex_only"][sel[64 * 11 + 5]] and batch["convex_only"][sel[64 * 13 + 5]]
    ov = batch["ov"]
    assert not ov[0:64].any() and ov[64:192].all() and not ov[192:256].any(), "the oracle disagrees with the screen on tiles 0-3"
    assert ov[64 * 11 + 5] == 0 and ov[64 * 13 + 5] == 0


@pytest.mark.parametrize("shape", ["odd_partial", "even_one"])
def test_tile_counts(batch, gpu, shape):
    """an odd tile count with a partial last tile (the last wave's second half is skipped), and an even count whose last tile holds one
    state; the states behind N are not written.  With depths (one tile per drain): verdicts and depth bits equal the oracle's too."""
    import torch
    sc, bp, qa, rows = gpu
    t = batch["tiles"] - 1 if shape == "odd_partial" else batch["tiles"]
    n = 64 * (t - 1) + (37 if shape == "odd_partial" else 1)
    assert t % 2 == (1 if shape == "odd_partial" else 0) and n >= batch["lane_min"]
    assert sc.valid_kernel(n) == "k_is_valid_v5"
    got = _verdicts(bp, qa, rows, n)
    assert np.array_equal(got[:n], batch["ov"][:n]), "verdicts differ from the oracle"
    assert np.all(got[n:] == 7)
    v1, d1 = bp.is_valid(qa[:n], rows, samples_per_env=SPE, want_min_dist=True)
    torch.cuda.synchronize()
    assert np.array_equal(v1.cpu().numpy(), batch["ov"][:n])
    assert np.array_equal(d1.cpu().numpy().view(np.uint64), batch["omd"][:n].view(np.uint64))


def test_env_rows_per_half(batch, gpu):
    """samples_per_env = 64: the halves of every pair read different env rows.  The same states as segments of zero length through
    check_motion, which hands the kernel an explicit env index per state: the same verdicts."""
    import torch
    sc, bp, qa, rows = gpu
    n = 64 * batch["tiles"]
    got = _verdicts(bp, qa, rows, n)
    assert np.array_equal(got, batch["ov"])
    diff = np.any(batch["rows"][N_SPECIAL:-1:2] != batch["rows"][N_SPECIAL + 1::2], axis=1)
    assert diff.all(), "the env rows of a pair's halves are meant to differ"
    assert sc.motion_kernel(n) == "k_motion_expand"        # (a segment of zero length expands into its end state alone)
    mv = bp.check_motion(qa, qa, rows, samples_per_env=SPE)
    torch.cuda.synchronize()
    assert np.array_equal(mv.cpu().numpy().astype(np.uint8), batch["ov"])


@pytest.mark.parametrize("tail", [None, "37", "1"])
def test_single_tile_tail(batch, gpu, monkeypatch, tail):
    """the last tiles of a launch are pulled one at a time: the plan's own tail (a batch of no more tiles than waves: every tile), an odd
    tail (the paired part is rounded down to an even count) and a tail of one tile, on an odd tile count -- the oracle's verdicts each time"""
    sc, bp, qa, rows = gpu
    if tail is None:
        monkeypatch.delenv("MOPA_K1_PAIR_TAIL_TILES")
    else:
        monkeypatch.setenv("MOPA_K1_PAIR_TAIL_TILES", tail)
    n = 64 * (batch["tiles"] - 2) + 37
    got = _verdicts(bp, qa, rows, n)
    assert np.array_equal(got[:n], batch["ov"][:n]), "verdicts differ from the oracle"
    assert np.all(got[n:] == 7)


def test_device_side_count(batch, gpu):
    """the count lives on the device and ends inside the first half of a pair, then inside the second: the prefix's verdicts, nothing else written"""
    import torch
    sc, bp, qa, rows = gpu
    tiles = batch["tiles"]
    for n in (64 * (tiles - 4) + 19, 64 * (tiles - 3) + 45):
        assert ((n - 1) // 64) % 2 == (0 if n == 64 * (tiles - 4) + 19 else 1) and n >= batch["lane_min"]
        got = _verdicts(bp, qa, rows, 64 * tiles, n_dev=torch.tensor([n], dtype=torch.int64, device=qa.device))
        assert np.array_equal(got[:n], batch["ov"][:n])
        assert np.all(got[n:] == 7)


def test_launches_repeat_and_streams(batch, gpu):
    """two launches back to back (the self-resetting tile counter), and launches on two streams (each with its own slab): identical bytes"""
    import torch
    sc, bp, qa, rows = gpu
    n = 64 * batch["tiles"] - 27
    a = _verdicts(bp, qa, rows, n)
    b = _verdicts(bp, qa, rows, n)
    assert np.array_equal(a, b) and np.array_equal(a[:n], batch["ov"][:n])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    o1 = torch.full((n,), 7, dtype=torch.uint8, device=qa.device)
    o2 = torch.full((n,), 7, dtype=torch.uint8, device=qa.device)
    bp.is_valid(qa[:n], rows, samples_per_env=SPE, out=o1, stream=s1)
    bp.is_valid(qa[:n], rows, samples_per_env=SPE, out=o2, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(o1.cpu().numpy(), a[:n]) and np.array_equal(o2.cpu().numpy(), a[:n])


def test_baked_equals_generic_bitwise(batch, gpu, tmp_path):
    """a fresh process with MOPA_K1_BAKED=0: the generic kernel writes the same bytes (verdicts, and the depth-reporting kernel's verdicts and depths)"""
    import torch
    n = 64 * batch["tiles"] - 27
    qfile, out = tmp_path / "batch.npz", tmp_path / "generic.npz"
    np.savez(qfile, qa=batch["qa"][:n], rows=batch["rows"], spe=np.array(SPE))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, ENV, str(qfile), str(out)], env=dict(os.environ, MOPA_K1_BAKED="0"), check=True, timeout=300)
    g = np.load(out)
    assert int(g["baked"][0]) == 0 and str(g["kernel"][0]) == "k_is_valid_v5"
    sc, bp, qa, rows = gpu
    v0 = bp.is_valid(qa[:n], rows, samples_per_env=SPE)
    v1, d1 = bp.is_valid(qa[:n], rows, samples_per_env=SPE, want_min_dist=True)
    torch.cuda.synchronize()
    assert np.array_equal(v0.cpu().numpy(), g["valid"])
    assert np.array_equal(v1.cpu().numpy(), g["valid_md"])
    assert np.array_equal(d1.cpu().numpy().view(np.uint64), g["min_dist"])
