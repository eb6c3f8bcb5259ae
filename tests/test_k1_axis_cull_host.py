"""Axis extents in the baked pass A, host side (no GPU): the static-partner test of the baked Push kernel run on the host
(mopa_k1_baked_static_host: the kernel's own predicate, FP32 centres and packed axis words out of the baked walk) under the
per-axis rule and under the bounding-radius rule, on 10^5 seeded states against the oracle's pair distances.

  (a) a culled pair is separated: every static pair of an axis owner whose oracle distance is <= the threshold is kept;
  (b) the new survivors are a subset of the bounding-radius rule's;
  (c) the |axis| magnitudes pass A unpacks (FP32 arithmetic, 10 bits, rounded up) are never below the FP64 values and exceed
      them by less than kAxisSlack = 1e-3 (mopa_valid_v5.inc, "Axis extents")."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENV = "SawyerPushObstacle-v0"
TRAITS = "K1Baked_SawyerPushObstacle"
K_AXIS_SLACK = 1.0e-3
N_UNIFORM, N_NEAR, N_LIMIT, N_CUBE = 40_000, 40_000, 1_000, 1_500      # 40 000 + 40 000 + 14 x 1 000 + 4 x 1 500 = 10^5


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        monkeypatch.delenv(k)


def _trait_ints(name):
    import bake_k1_scenes as B
    inc = open(B.OUT).read()
    body = inc[inc.index(f"struct {TRAITS} "):]
    return [int(x, 0) for x in re.search(rf"static constexpr \w+ {name}\[\w+\] = \{{([^{{}}]*)\}};", body).group(1).replace("u", "").split(",")]


def _states(pi):
    """Full qpos rows: uniform, near the initial pose, every joint at each limit (the others uniform / near, alternating), and
    the cube at the four corners of its +-0.05 box (states uniform / near, alternating)."""
    from conftest import sample_states
    from mopa_rl_amd.scene import default_qpos
    m = pi.model
    act = np.asarray(pi.ref_joint_pos_indexes)
    lo, hi = np.asarray(pi.jnt_minimum), np.asarray(pi.jnt_maximum)
    row = default_qpos(ENV, m)

    def mixed(n, seed):
        qa = sample_states(pi, n, seed, "uniform")[0]
        qa[1::2] = sample_states(pi, n, seed + 1, "near")[0][1::2]
        return qa

    parts = [sample_states(pi, N_UNIFORM, 101, "uniform")[0], sample_states(pi, N_NEAR, 102, "near")[0]]
    for j in range(len(act)):
        for k, lim in enumerate((lo[j], hi[j])):
            qa = mixed(N_LIMIT, 200 + 4 * j + 2 * k)
            qa[:, j] = lim
            parts.append(qa)
    n_plain = sum(len(p) for p in parts)
    parts += [mixed(N_CUBE, 300 + 2 * c) for c in range(4)]
    qa = np.concatenate(parts)
    q = np.repeat(row[None], len(qa), axis=0)
    q[:, act] = qa
    free = [int(m.jnt_qposadr[j]) for j in range(len(m.jnt_names)) if int(m.jnt_type[j]) == 0]
    assert free, "Push has a free-jointed cube"
    for c, (sx, sy) in enumerate(((-1, -1), (-1, 1), (1, -1), (1, 1))):
        q[n_plain + c * N_CUBE: n_plain + (c + 1) * N_CUBE, free[0]: free[0] + 2] += 0.05 * np.array([sx, sy])
    assert len(q) == 100_000
    return np.ascontiguousarray(qa), np.ascontiguousarray(q)


@pytest.fixture(scope="module")
def run():
    """(pi, exported tables, slot -> geom, oracle, states, keep_new, keep_old, axis): one host run shared by the tests"""
    import bake_k1_scenes as B
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    pi = planner_inputs(ENV)
    args = (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    ex = _lib.k1_export(*args)
    o = B.hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + ex["nmg"]]]
    qa, q = _states(pi)
    L = _lib.lib()
    n_ent = C.c_int32(-1)
    assert L.mopa_k1_baked_static_host(99, 0, None, None, None, None, None, None) != 0
    assert L.mopa_k1_baked_static_host(1, 0, None, None, None, None, None, C.byref(n_ent)) == 0
    assert n_ent.value == (len(ex["tab"]) - 3 * ex["nmg"]) // 8
    n = len(q)
    kn, ko = np.full((n, n_ent.value), 255, np.uint8), np.full((n, n_ent.value), 255, np.uint8)
    axis = np.full((n, ex["nmg"], 3), np.nan, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mopa_k1_baked_static_host(1, n, vp(qa), vp(q), vp(kn), vp(ko), vp(axis), None) == 0
    return pi, ex, mg, O.OracleScene(*args), q, kn, ko, axis


def _axis_pairs(pi, ex, mg):
    """(table entry, oracle pair index) of every static non-plane pair of an axis owner"""
    m = pi.model
    tab = ex["tab"].astype("<i4").view("<u4")
    nmg = ex["nmg"]
    n5 = (len(tab) - 3 * nmg) // 8
    slot = _trait_ints("ax_slot")
    out = []
    for M in range(nmg):
        if slot[M] < 0:
            continue
        padr, cnt = int(tab[8 * n5 + nmg + 2 * M]), int(tab[8 * n5 + M])
        for K in range(cnt & 0xFF, (cnt & 0xFF) + ((cnt >> 8) & 0xFF)):
            pg = int(tab[8 * (padr + K) + 7]) & 0xFF
            hit = [k for k, (a, b) in enumerate(m.pair_geom) if {int(a), int(b)} == {mg[M], pg}]
            assert len(hit) == 1
            out.append((padr + K, hit[0]))
    return out


def test_axis_owners_are_the_capsules_and_cylinders_with_static_partners(run):
    pi, ex, mg, *_ = run
    slot = _trait_ints("ax_slot")
    nstat = _trait_ints("nstat")
    T = pi.model.geom_type
    assert [s >= 0 for s in slot] == [int(T[mg[M]]) in (3, 5) and nstat[M] > 0 for M in range(ex["nmg"])]
    assert [s for s in slot if s >= 0] == list(range(sum(s >= 0 for s in slot)))
    assert len(_axis_pairs(pi, ex, mg)) == 52         # of Push's 92 static pairs


def test_entries_outside_the_static_group_are_not_touched(run):
    pi, ex, mg, _, _, kn, ko, _ = run
    tab = ex["tab"].astype("<i4").view("<u4")
    nmg = ex["nmg"]
    n5 = (len(tab) - 3 * nmg) // 8
    static = np.zeros(n5, bool)
    for M in range(nmg):
        padr, cnt = int(tab[8 * n5 + nmg + 2 * M]), int(tab[8 * n5 + M])
        static[padr + (cnt & 0xFF): padr + (cnt & 0xFF) + ((cnt >> 8) & 0xFF)] = True
    assert static.sum() == 92
    assert np.all(kn[:, ~static] == 2) and np.all(ko[:, ~static] == 2)
    assert np.all(kn[:, static] <= 1) and np.all(ko[:, static] <= 1)
    # box and sphere owners keep the bounding-radius rule: the same verdicts
    ents = [e for e, _ in _axis_pairs(pi, ex, mg)]
    other = static.copy()
    other[ents] = False
    assert np.array_equal(kn[:, other], ko[:, other])


def test_a_culled_pair_is_separated_and_survivors_are_a_subset(run):
    pi, ex, mg, orc, q, kn, ko, _ = run
    thr = pi.spec.contact_threshold
    pairs = _axis_pairs(pi, ex, mg)
    ents, idx = [e for e, _ in pairs], [k for _, k in pairs]
    n_new = n_old = n_touch = 0
    for s, row in enumerate(q):
        touching = orc.pair_dist(row)[idx] <= thr
        n_touch += int(touching.sum())
        missed = touching & (kn[s, ents] == 0)
        assert not missed.any(), f"state {s}: pair {np.asarray(idx)[missed]} within the threshold is culled"       # (a)
    assert np.all(kn[:, ents] <= ko[:, ents]), "a pair the bounding-radius rule culls survives the axis rule"       # (b)
    n_new, n_old = int(kn[:, ents].sum()), int(ko[:, ents].sum())
    print(f"static pairs of axis owners kept per state: {n_old / len(q):.2f} -> {n_new / len(q):.2f}; within the threshold: {n_touch / len(q):.3f}")
    assert n_touch > 0 and n_new < n_old


def test_unpacked_axis_encloses_the_fp64_axis(run):
    pi, ex, mg, orc, q, _, _, axis = run
    slot = _trait_ints("ax_slot")
    own = [M for M in range(ex["nmg"]) if slot[M] >= 0]
    assert np.all(axis[:, [M for M in range(ex["nmg"]) if slot[M] < 0]] == -1.0)
    got = axis[:, own].astype(np.float64)
    want = np.stack([np.abs(orc.fk(row)[1][[mg[M] for M in own], :, 2]) for row in q])
    assert np.all(got >= want), f"unpacked |axis| below the FP64 value by {np.max(want - got):.3e}"                # (c)
    assert np.all(got <= want + K_AXIS_SLACK), f"unpacked |axis| above the FP64 value by {np.max(got - want):.3e}"
    print(f"unpacked - FP64 |axis|: min {np.min(got - want):.3e}, max {np.max(got - want):.3e}")
