"""Resident pairs of the baked K1 walk, host side (no GPU): which pairs the Push traits list, that pass A really keeps them
in most states, and that the walk's in-place evaluation gives the oracle's distance for the pair bit for bit."""
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


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MOPA_") and k != "MOPA_HIP_LIB"]:
        monkeypatch.delenv(k)


def committed_resident():
    """rows (M, K, slot 1, slot 2, class, type 1, type 2) of the committed traits' resident list"""
    import bake_k1_scenes as B
    inc = open(B.OUT).read()
    body = inc[inc.index(f"struct {TRAITS} "):]
    n = int(re.search(r"static constexpr int n_res = (\d+);", body).group(1))
    rows = re.search(r"static constexpr int res\[\d+\]\[7\] = \{(.*)\};", body).group(1)
    rows = [[int(x) for x in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", rows)]
    return rows[:n]


@pytest.fixture(scope="module")
def scene():
    from mopa_rl_amd import _lib
    from mopa_rl_amd.scene import planner_inputs
    from oracle import oracle as O
    import bake_k1_scenes as B
    pi = planner_inputs(ENV)
    args = (pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    ex = _lib.k1_export(*args)
    o = B.hdr_int(ex, "o_mg_geom")
    mg = [int(g) for g in ex["ints"][o: o + ex["nmg"]]]          # moving geom slot -> model geom id
    return pi, ex, mg, O.OracleScene(*args)


def pair_index(m, ga, gb):
    hit = [k for k, (a, b) in enumerate(m.pair_geom) if {int(a), int(b)} == {ga, gb}]
    assert len(hit) == 1
    return hit[0]


def test_push_lists_the_head_l2_pair(scene):
    pi, ex, mg, _ = scene
    m = pi.model
    res = committed_resident()
    assert 1 <= len(res) <= 2
    bodies = [{m.body_names[int(m.geom_body[mg[r[2]]])], m.body_names[int(m.geom_body[mg[r[3]]])]} for r in res]
    assert {"head", "right_l2"} in bodies
    tab = ex["tab"].astype("<i4").view("<u4")
    n5 = (len(tab) - 3 * ex["nmg"]) // 8
    for M, K, s1, s2, code, t1, t2 in res:
        # the row restates the table entry it replaces: owner, partner, class, order of the two geoms
        padr, cnt = int(tab[8 * n5 + ex["nmg"] + 2 * M]), int(tab[8 * n5 + M])
        assert K < (cnt & 0xFF), "not an entry of the owner's moving group"
        fl = int(tab[8 * (padr + K) + 7])
        assert (fl >> 13) & 1 and ((fl >> 8) & 0xF) == code and code in (4, 5, 8)
        partner, owner_is_g2 = (fl >> 14) & 0xFF, (fl >> 12) & 1
        assert (s1, s2) == ((partner, M) if owner_is_g2 else (M, partner))
        assert (fl & 0xFF) == mg[partner]
        assert (t1, t2) == (int(m.geom_type[mg[s1]]), int(m.geom_type[mg[s2]])) and t1 <= t2
    # the generator's choice is what is committed (the file being current is tests/test_k1_baked_host.py's check)
    assert len({(r[0], r[1]) for r in res}) == len(res)


def test_resident_pairs_survive_pass_a_in_most_states(scene):
    """An independently seeded sample of 4096 states (half uniform, half near the initial pose): the FP32 centres against the
    table's FP32 squared cull radius, as pass A tests them."""
    from conftest import sample_states
    pi, ex, mg, orc = scene
    qu, row = sample_states(pi, 2048, 4242, "uniform")
    qn, _ = sample_states(pi, 2048, 4243, "near")
    qa = np.concatenate([qu, qn])
    q = np.repeat(row, len(qa), axis=0)
    q[:, np.asarray(pi.ref_joint_pos_indexes)] = qa
    cen = np.stack([orc.fk(r)[0][mg] for r in q]).astype(np.float32)
    tab = ex["tab"].astype("<i4")
    n5 = (len(tab) - 3 * ex["nmg"]) // 8
    for M, K, s1, s2, *_ in committed_resident():
        e = int(tab[8 * n5 + ex["nmg"] + 2 * M]) + K
        rs2 = tab[8 * e + 3: 8 * e + 4].view("<f4")[0]
        d = cen[:, s1] - cen[:, s2]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        kept = np.count_nonzero(~(d2 > rs2)) / len(q)
        assert kept >= 0.75, f"pair ({M}, {K}) kept in {kept:.3f} of the states"


def test_resident_distances_equal_the_oracle_bitwise(scene):
    """10^4 states of the families of tests/test_k1_baked_fk_host.py: every joint at a limit, one ULP beyond, zero, the default
    pose, gripper slides across their range, the cube at varied poses with non-unit quaternions."""
    from mopa_rl_amd import _lib
    from test_k1_baked_fk_host import _states
    pi, ex, mg, orc = scene
    L = _lib.lib()
    res = committed_resident()
    n_res = C.c_int32(-1)
    assert L.mopa_k1_baked_resident_host(1, 0, None, None, None, C.byref(n_res)) == 0
    assert n_res.value == len(res)
    assert L.mopa_k1_baked_resident_host(99, 0, None, None, None, None) != 0
    n = 10_000
    q = _states(pi, n, 11)
    qa = np.ascontiguousarray(q[:, np.asarray(pi.ref_joint_pos_indexes)])
    out = np.full((n, len(res)), np.nan)
    assert L.mopa_k1_baked_resident_host(1, n, qa.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None) == 0
    idx = [pair_index(pi.model, mg[r[2]], mg[r[3]]) for r in res]
    want = np.stack([orc.pair_dist(row)[idx] for row in q])
    # pair_dist reports ORC_FAR, not a distance, for a pair whose bounding spheres the oracle's own broad phase finds apart
    # (bp_cull, zero margin): there the walk's distance has nothing to equal bit for bit -- it must say "apart" (> 0: no part in
    # verdict or depth).  Everywhere else: the same bits.
    from oracle import oracle as O
    far = want == O.ORC_FAR
    bad = np.count_nonzero(want.view(np.uint64)[~far] != out.view(np.uint64)[~far])
    assert bad == 0, f"{bad} of {np.count_nonzero(~far)} distances differ"
    assert np.all(out[far] > 0.0)
    assert np.count_nonzero(~far) > n // 2
    thr = pi.spec.contact_threshold
    assert np.count_nonzero(want <= thr) > 100 and np.count_nonzero(want[~far] > thr) > 100      # both sides of the threshold are met
