"""Witness points of the proximity report, host form (mopa_geom_witness_host: the host compile of geom_witness and gjk_witness): the
distance has the bits of the exact route's, the two points lie in their shapes and are that far apart, the normal is their
direction, the other order of a pair exchanges them bit for bit -- on the whole case set of gjk_cases at both bands, on random
separated pairs of every closed-form class and on overlapping pairs of every class.  The properties and their slacks are
witness_ref's: nothing of them shares code with the functions under test.  No GPU.

Measured on this case set (printed by test_attainment...): the largest |p2 - p1| - d over all 34 families is 3.6e-15 (capsule-mesh
edge), nine orders below the kGjkTol the bound grants; the largest excess of a witness point over its shape is 3.9e-16."""
import ctypes as C
import types as pytypes

import numpy as np
import pytest

import frames_ref as F
import gjk_cases as G
import proximity_exact_ref as X
import proximity_ref as P
import witness_ref as W
from geom_ref import CAPSULE, MESH, PLANE, SPHERE

bits = W.bits


@pytest.fixture(scope="module")
def can():
    from mopa_rl_amd.scene import load_scene
    return P.can_of(load_scene("sawyer_lift_obstacle"))


@pytest.fixture(scope="module")
def solved(can):
    """the items and, per band, (witness table [M, 10], support evaluations [M], the exact route's distances [M])"""
    its = G.items(can)
    cs = [it.case for it in its]
    return its, cs, {b: W.host_witness(cs, can, b, iters=True) + (X.host_sep(cs, can, b),) for b in X.BANDS}


def test_same_distance_and_same_bits_at_both_bands(solved):
    its, cs, ex = solved
    assert len(its) > 6000 and len(G.families(its)) == 34                     # the whole case set, nothing skipped
    for band in X.BANDS:
        w, n, d = ex[band]
        assert w.shape == (len(its), 10)
        assert np.array_equal(bits(w[:, 0]), bits(d)), band                    # FAR included
        rep = d != F.FAR
        assert rep.sum() > 3000 and (n[rep] > 0).all(), band                   # every reported one went through the walk, none to its cap
    a, b = ex[0.01][0], ex[0.05][0]
    both = (a[:, 0] != F.FAR) & (b[:, 0] != F.FAR)
    assert both.sum() > 2000 and np.array_equal(bits(a[both]), bits(b[both]))


def test_membership(solved, can):
    its, cs, ex = solved
    scale = np.array([it.scale for it in its])
    for band in X.BANDS:
        print("band", band, "largest excess of a witness point over its shape:", W.check_membership(cs, ex[band][0], scale, can))


def test_attainment_and_the_reconstruction_error_per_family(solved):
    its, cs, ex = solved
    scale, true = np.array([it.scale for it in its]), np.array([it.true for it in its])
    fam = np.array([it.family for it in its])
    for band in X.BANDS:
        gap = W.check_attainment(cs, ex[band][0], true, scale)
        assert np.isfinite(gap).sum() == (ex[band][0][:, 0] != F.FAR).sum()     # every reported pair of this set is separated, and was checked
        for f in G.families(its):
            print(f"band {band}: largest |p2 - p1| - d, {f}: {np.nanmax(gap[fam == f]):+.3e}")
        assert np.nanmax(gap) <= X.K_GJK_TOL


def test_normal(solved):
    its, cs, ex = solved
    scale = np.array([it.scale for it in its])
    for band in X.BANDS:
        W.check_normal(cs, ex[band][0], scale)


def test_the_other_order_exchanges_the_points_bit_for_bit(solved, can):
    its, cs, ex = solved
    w = ex[0.05][0]
    # the `swapped` items against the items they were made from: the same base case three places earlier (built, moved1, moved2, swapped)
    n_sw = 0
    for i, it in enumerate(its):
        if it.form == "swapped":
            assert its[i - 3].form == "built" and its[i - 3].family == it.family
            assert np.array_equal(bits(w[i]), bits(W.exchanged(w[i - 3:i - 2])[0])), (it.family, it.scale, it.gap, it.variant)
            n_sw += 1
    assert n_sw > 1000
    # ... and every item without a mesh given the other way round
    pick = [i for i, it in enumerate(its) if it.case.t2 != MESH]
    rev = W.host_witness([cs[i].swapped() for i in pick], can, 0.05)
    bad = (bits(rev) != bits(W.exchanged(w[pick]))).any(axis=1)
    assert not bad.any(), [(its[pick[k]].family, its[pick[k]].form) for k in np.nonzero(bad)[0][:8]]
    assert (rev[:, 0] != F.FAR).sum() > 3000


def test_far_pairs_are_all_zero(solved):
    its, cs, ex = solved
    for band in X.BANDS:
        w = ex[band][0]
        far = w[:, 0] == F.FAR
        assert far.sum() > 100 and not w[far, 1:].any() and not np.signbit(w[far, 1:]).any()


@pytest.fixture(scope="module")
def closed(can):
    cs = W.closed_cases(can)
    band = 0.05
    return cs, band, W.host_witness(cs, can, band), X.host_sep(cs, can, band)


def test_closed_form_classes(closed, can):
    cs, band, w, d = closed
    assert len(cs) == len(W.CLOSED_CLASSES) * W.N_CLOSED * len(G.GAPS)
    assert np.array_equal(bits(w[:, 0]), bits(d))                               # 1: the distance, FAR included
    w1 = W.host_witness(cs, can, 0.5)
    rep = w[:, 0] != F.FAR
    assert np.array_equal(bits(w[rep]), bits(w1[rep]))                           # ... and the same triple at another band
    sep = rep & (w[:, 0] > 0)
    for t1, t2 in W.CLOSED_CLASSES:                                              # "a few hundred" of every class, most of them in band
        m = np.array([(c.t1, c.t2) == (t1, t2) for c in cs])
        assert m.sum() == W.N_CLOSED * len(G.GAPS) and (m & sep).sum() >= 100, (t1, t2, int((m & sep).sum()))
    # 2 - 4 with true := d
    worst, gap = W.check_all(cs, w, np.where(rep, w[:, 0], 0.0), W.RANDOM_SCALE, can)
    print("closed-form classes: largest excess", worst, "largest | |p2 - p1| - d |", np.nanmax(np.abs(gap)))
    assert far_rows_zero(w)
    # 5: the other order.  Capsule-capsule is left out of the bit comparison: its distance function evaluates the two axes in the order
    # given, so d itself differs in the last bit between the two orders; there the witness is compared to E_m
    pick = [i for i, c in enumerate(cs) if c.t2 != MESH]
    rev = W.host_witness([cs[i].swapped() for i in pick], can, band)
    want = W.exchanged(w[pick])
    kk = np.array([(cs[i].t1, cs[i].t2) == (CAPSULE, CAPSULE) for i in pick])
    bad = (bits(rev) != bits(want)).any(axis=1) & ~kk
    assert not bad.any(), [(cs[pick[k]].cls, rev[k], want[k]) for k in np.nonzero(bad)[0][:4]]
    both = kk & (rev[:, 0] != F.FAR) & (want[:, 0] != F.FAR)
    assert both.sum() >= 100 and np.abs(rev[both] - want[both]).max() <= W.e_m(W.RANDOM_SCALE)
    # the one-line formulas
    e = W.e_m(W.RANDOM_SCALE)
    n_f = 0
    for i, c in enumerate(cs):
        if not sep[i]:
            continue
        if (c.t1, c.t2) == (SPHERE, SPHERE):
            u = (c.p2 - c.p1) / np.linalg.norm(c.p2 - c.p1)
            a, b = c.p1 + c.s1[0] * u, c.p2 - c.s2[0] * u
        elif (c.t1, c.t2) == (PLANE, SPHERE):
            u = c.m1[:, 2]
            b = c.p2 - c.s2[0] * u
            a = b - (u @ (b - c.p1)) * u
        else:
            continue
        assert np.abs(w[i, 1:4] - u).max() <= e and np.abs(w[i, 4:7] - a).max() <= e and np.abs(w[i, 7:10] - b).max() <= e, (c.cls, i)
        n_f += 1
    assert n_f >= 200


def far_rows_zero(w):
    far = w[:, 0] == F.FAR
    return far.any() and not w[far, 1:].any()


def test_overlap_is_the_contact_frame_read_the_other_way_round(can):
    cs = F.random_cases() + F.degenerate_cases()
    w = W.host_witness(cs, can, 0.05)
    fr = F.host_frames(cs, can)
    ov = w[:, 0] <= 0.0
    for t1, t2 in F.PRIMITIVE_CLASSES + F.MESH_CLASSES:
        assert sum(1 for c, o in zip(cs, ov) if o and (c.t1, c.t2) == (t1, t2)) >= 2, (t1, t2)
    assert np.array_equal(bits(w[ov, 0]), bits(fr[ov, 0])) and np.array_equal(bits(w[ov, 1:4]), bits(fr[ov, 1:4]))
    p1, p2, pos, n, d = w[ov, 4:7], w[ov, 7:10], fr[ov, 4:7], fr[ov, 1:4], w[ov, 0]
    # p1, p2 are one rounding each of pos -/+ (d/2) n and their sum is one more: one ulp of the largest of them, per component
    ulp = np.spacing(np.maximum(np.maximum(np.abs(p1), np.abs(p2)), np.abs(pos)))
    assert (np.abs(0.5 * (p1 + p2) - pos) <= ulp).all()
    assert (np.abs(np.einsum("ij,ij->i", p2 - p1, n) - d) <= 1e-12).all()
    # the other order of an overlapping pair
    pick = [i for i, c in enumerate(cs) if ov[i] and c.t2 != MESH and (c.t1, c.t2) != (CAPSULE, CAPSULE)]
    rev = W.host_witness([cs[i].swapped() for i in pick], can, 0.05)
    same_type = np.array([cs[i].t1 == cs[i].t2 for i in pick])
    # (two shapes of one type in overlap are evaluated as given: geom_frame's own rule; the mixed-type pairs are exchanged exactly)
    assert np.array_equal(bits(rev[~same_type]), bits(W.exchanged(w[pick])[~same_type]))


def test_the_check_can_fail(solved, can):
    its, cs, ex = solved
    w = ex[0.05][0]
    scale, true = np.array([it.scale for it in its]), np.array([it.true for it in its])
    rows = [i for i in np.nonzero(w[:, 0] != F.FAR)[0] if its[i].scale == 1.0][:200]
    W.check_all(cs, w, true, scale, can, rows)
    n = w[:, 1:4]
    # p2 moved by 1e-5 along n: the two points are further apart than d + kGjkTol
    moved = w.copy()
    moved[:, 7:10] += 1e-5 * n
    with pytest.raises(AssertionError):
        W.check_attainment(cs, moved, true, scale, rows)
    # p1 and p2 exchanged: n points from p2 to p1
    moved = w.copy()
    moved[:, 4:7], moved[:, 7:10] = w[:, 7:10], w[:, 4:7]
    with pytest.raises(AssertionError):
        W.check_normal(cs, moved, scale, rows)
    # a point moved 1e-6 out of its shape: p1 along +n (n points away from shape 1; -n leads into it), p2 along -n
    for sl, sg in ((slice(4, 7), 1.0), (slice(7, 10), -1.0)):
        moved = w.copy()
        moved[:, sl] += sg * 1e-6 * n
        with pytest.raises(AssertionError):
            W.check_membership(cs, moved, scale, can, rows)
    # ... and two points 1e-5 inside their shapes are closer than the true distance
    moved = w.copy()
    moved[:, 4:7] += 1e-5 * n
    with pytest.raises(AssertionError):
        W.check_attainment(cs, moved, true, scale, rows)


def test_argument_rules():
    from mopa_rl_amd import _lib
    L = _lib.lib()
    for sym in ("mopa_proximity_witness_batch", "mopa_proximity_witness_state", "mopa_geom_witness_batch", "mopa_geom_witness_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(L, sym)
    host = L.mopa_geom_witness_host
    t = np.array([[2, 2]], dtype=np.int32)
    r = np.zeros((1, 2, 15))
    r[0, :, 3] = r[0, :, 7] = r[0, :, 11] = 1.0
    r[0, :, 12] = 0.1
    r[0, 1, 0] = 0.21
    o = np.full(10, 7.0)
    tp, rp, op = t.ctypes.data_as(_lib._ip), r.ctypes.data_as(_lib._dp), o.ctypes.data_as(_lib._dp)
    assert host(0, None, None, None, 0, 0.01, None, None) == 0
    assert host(-1, tp, rp, None, 0, 0.01, op, None) == 1                       # MOPA_ERR_INVALID_ARG
    assert host(1, None, rp, None, 0, 0.01, op, None) == 1 and host(1, tp, None, None, 0, 0.01, op, None) == 1
    assert host(1, tp, rp, None, 0, 0.01, None, None) == 1
    assert host(1, tp, rp, None, 3, 0.01, op, None) == 1 and b"null" in L.mopa_last_error()
    for band in (-0.01, float("nan"), float("inf")):
        assert host(1, tp, rp, None, 0, band, op, None) == 1 and b"band" in L.mopa_last_error()
    assert (o == 7.0).all()                                                      # a refusal writes nothing
    assert host(1, tp, rp, None, 0, 0.05, op, None) == 0
    assert np.allclose(o, [0.01, 1, 0, 0, 0.1, 0, 0, 0.11, 0, 0], atol=1e-15)    # two spheres 1 cm apart along x
    t[0] = (0, 0)
    assert host(1, tp, rp, None, 0, 0.05, op, None) == 0 and o[0] == F.FAR and not o[1:].any()      # (plane, plane): not a pair the narrow phase serves
    assert L.mopa_geom_witness_batch(0, -1, None, None, None, 0, 0.01, None, None) == 1
    assert L.mopa_geom_witness_batch(0, 1, None, None, None, 0, 0.01, None, None) == 1
    nul = [None] * 3
    assert L.mopa_proximity_witness_batch(None, None, None, 1, 1, 0.01, 4, None, None, None, None, *nul, None) == 1
    assert L.mopa_proximity_witness_state(None, None, 0.01, 4, None, None, None, None, *nul) == 1
    with pytest.raises(_lib.MopaError):
        _lib.geom_witness_host(np.zeros((2, 2)), np.zeros((1, 2, 15)), 0.01)


def test_python_refusals_precede_any_device_call():
    """witness=True without exact=True is a ValueError, a glued scene a NotImplementedError: both before anything reaches the library
    (the stand-ins below have no handle to reach it with)"""
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner
    from mopa_rl_amd.planner import PyKinematicPlanner
    class Stub:
        na, nq = 7, 9
        proximity_state_raw = _lib.Scene.proximity_state_raw

        def __init__(self, glue):
            self.glue = glue

    plain, glued = Stub(None), Stub(object())
    for sc in (plain, glued):
        with pytest.raises(ValueError, match="exact=True"):
            BatchPlanner(sc).proximity(None, None, band=0.05, witness=True)
        with pytest.raises(ValueError, match="exact=True"):
            _lib.Scene.proximity_state_raw(sc, None, 0.05, witness=True)
        with pytest.raises(ValueError, match="exact=True"):
            _lib.Scene.proximity_state(sc, None, 0.05, witness=True)
    with pytest.raises(NotImplementedError):
        BatchPlanner(glued).proximity(None, None, band=0.05, exact=True, witness=True)
    with pytest.raises(NotImplementedError):
        _lib.Scene.proximity_state_raw(glued, None, 0.05, exact=True, witness=True)
    for gb in (False, True):
        with pytest.raises(ValueError, match="exact=True"):
            PyKinematicPlanner.proximity(pytypes.SimpleNamespace(glue_bodies=gb), None, 0.05, witness=True)
    with pytest.raises(NotImplementedError):
        PyKinematicPlanner.proximity(pytypes.SimpleNamespace(glue_bodies=True), None, 0.05, exact=True, witness=True)


def test_scene_level_sequential_form(oracle_mod):
    """witness_ref.proximity_witness on a few Lift states (mesh pairs among them): the report rows are proximity_ref.select's on the exact
    pair table, every record's witness passes the checks, unused slots are zero"""
    from conftest import sample_states
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs("SawyerLiftObstacle-v0")
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    qa, rows = sample_states(pi, 24, 5, "near")
    poses = P.poses(pi, orc, qa, rows, 24)
    band, K = 0.05, 6
    got = W.proximity_witness(pi, poses, band, K)
    want = P.select(X.pair_dists(pi, *poses, band), band, K)
    for g, w in zip((got[k] for k in W.OUTPUTS[:4]), want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    m = pi.model
    pg, gt, size = np.asarray(m.pair_geom).reshape(-1, 2), np.asarray(m.geom_type), np.asarray(m.geom_size, dtype=np.float64)
    cs, tab = [], []
    for i in range(len(qa)):
        k = min(int(got["count"][i]), K)
        assert not got["normal"][i, k:].any() and not got["p1"][i, k:].any() and not got["p2"][i, k:].any()
        for j in range(k):
            a, b = pg[got["pair"][i, j]]
            cs.append(F.Case(int(gt[a]), size[a], poses[0][i, a], poses[1][i, a].reshape(3, 3), int(gt[b]), size[b], poses[0][i, b], poses[1][i, b].reshape(3, 3)))
            tab.append(np.concatenate([[got["dist"][i, j]], got["normal"][i, j], got["p1"][i, j], got["p2"][i, j]]))
    tab = np.array(tab)
    assert len(cs) > 30 and (tab[:, 0] > 0).sum() > 10
    # (membership is a property of separated pairs: in overlap p1 / p2 are the contact frame's witness points by definition, and the
    #  portal's are not on the shapes' surfaces)
    W.check_membership(cs, tab, W.RANDOM_SCALE, P.can_of(m), rows=np.nonzero(tab[:, 0] > 0)[0])
    W.check_attainment(cs, tab, np.where(tab[:, 0] > 0, tab[:, 0] - X.K_GJK_TOL, 0.0), W.RANDOM_SCALE)     # (true >= d - kGjkTol: the exact route's contract)
    W.check_normal(cs, tab, W.RANDOM_SCALE)
