"""Proximity report, host form (mopa_geom_sep_host: the host compile of the kernels' geom_sep): the contact report's bits in
overlap, the independent signed distance of geom_ref on separated shapes, band membership, order of the two geoms, rigid motion,
the margin broad phase restated from the scenes' bounds, ABI.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import frames_ref as F
import proximity_ref as P
from conftest import SUPPORTED_ENVS, sample_states
from geom_ref import rand_rot

# Largest shortfall ref - d of an inflated-route class measured with the host compile on this case set: 1.049e-2 (box-mesh at band
# 0.05; per class and band the figures are printed by test_truth_on_separated_shapes and quoted in DESIGN.md section 4 -- the portal
# depth is the depth along the centre line's portal, not the least one, so the shortfall grows with the band and is far above 1e-4
# for every inflated class but box-box).  The cap is 4 x that, the project's usual margin over a measured deviation.
SHORTFALL_MEASURED = 1.049e-2
SHORTFALL_CAP = 4 * SHORTFALL_MEASURED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def can():
    from mopa_rl_amd.scene import load_scene
    return P.can_of(load_scene("sawyer_lift_obstacle"))


@pytest.fixture(scope="module")
def solved(can):
    cs, ref = P.sep_cases(can)
    return cs, ref, {b: P.host_sep(cs, can, b) for b in P.BANDS}


def test_overlap_carries_the_contact_reports_bits(solved, can):
    cs, ref, got = solved
    d0 = F.host_frames(cs, can)[:, 0]           # geom_dist's bits (test_contact_frames_host pins them to the oracle)
    pen = d0 <= 0
    per_class = {}
    for c, p in zip(cs, pen):
        per_class[c.cls] = per_class.get(c.cls, 0) + int(p)
    assert len(per_class) == len(F.PRIMITIVE_CLASSES) + len(F.MESH_CLASSES) and all(v >= 2 for v in per_class.values()), per_class
    for band in P.BANDS:
        assert np.array_equal(_bits(got[band][pen]), _bits(d0[pen])), band
    # band = 0: nothing but overlaps is reported (a closed-form class at distance exactly 0 is one)
    assert (got[0.0][~pen] == F.FAR).all()


def test_truth_on_separated_shapes(solved):
    cs, ref, got = solved
    worst = 0.0
    for band in (0.01, 0.05):
        short = {}
        for c, r, d in zip(cs, ref, got[band]):
            if np.isnan(r) or not r > 0 or d == F.FAR:
                continue
            if P.closed(c):
                assert abs(d - r) <= 1e-6, (c.cls, band, d, r)
            else:
                assert d <= r + 1e-6 + 2e-7, (c.cls, band, d, r)       # the conservative side
                short.setdefault(c.cls, []).append(r - d)
        assert len(short) == 8, sorted(short)
        for cls, e in sorted(short.items()):
            print(f"band {band}: shortfall ref - d, {cls}: n = {len(e)}, median = {np.median(e):.3e}, max = {max(e):.3e}")
            worst = max(worst, max(e))
    print(f"largest shortfall {worst:.3e}")
    assert worst <= SHORTFALL_CAP


def test_band_membership(solved):
    cs, ref, got = solved
    for band in (0.01, 0.05):
        stat = {}
        for c, r, d in zip(cs, ref, got[band]):
            if np.isnan(r) or not r > 0:
                continue
            s = stat.setdefault(c.cls, {"n": 0, "skipped": 0, "reported": 0, "rejected": 0})
            s["n"] += 1
            if r <= band - 1e-5:
                assert d != F.FAR, (c.cls, band, r)
                s["reported"] += 1
            elif r >= band + 1e-5:
                assert d == F.FAR, (c.cls, band, r, d)
                s["rejected"] += 1
            else:
                s["skipped"] += 1
        assert len(stat) == len(F.PRIMITIVE_CLASSES) + len(F.MESH_CLASSES)
        for cls, s in stat.items():
            assert s["reported"] >= 8 and s["rejected"] >= 4 and s["skipped"] <= 0.05 * s["n"], (cls, band, s)


def test_order_of_the_two_geoms(solved, can):
    """A pair of two different types is evaluated in the narrow phase's canonical order whichever way it is given, and two separated
    shapes of one type (of different sizes) enter the inflated route by the order of their sizes: the same bits.  Two shapes of one type are
    otherwise evaluated as given: a closed form moves by rounding; an overlap found by the portal refinement (cylinder-cylinder) has
    geom_dist's value, which depends on the order by more than that -- the contact report's property, not asserted here."""
    cs, ref, got = solved
    rev = P.host_sep([c.swapped() for c in cs], can, 0.05)
    n = {"types": 0, "inflated": 0, "closed": 0}
    for c, a, b in zip(cs, got[0.05], rev):
        if c.t1 != c.t2:
            assert _bits(a) == _bits(b), (c.cls, c.what)
            n["types"] += int(a != F.FAR)
        elif not P.closed(c) and a > 0 and b > 0:
            assert _bits(a) == _bits(b), (c.cls, c.what, a, b)
            n["inflated"] += int(a != F.FAR)
        elif P.closed(c) or not c.mpr:
            assert (a == F.FAR) == (b == F.FAR) and (a == F.FAR or abs(a - b) <= 1e-12), (c.cls, c.what, a, b)
            n["closed"] += int(a != F.FAR)
    assert n["types"] >= 150 and n["inflated"] >= 20 and n["closed"] >= 30, n


def test_rigid_motion(solved, can):
    """1e-12 on the closed-form classes, 1e-9 on the inflated route.  (An OVERLAP of a class that goes through the portal refinement
    carries geom_dist's value, whose path through the portals a rigid motion may change: test_contact_frames_host leaves those out
    of its rigid-motion test for that reason, and so does this one.)"""
    cs, ref, got = solved
    rng = np.random.default_rng(17)
    # (a case within 1e-8 of the band's edge may change sides under rounding: none is placed there)
    pick = [i for i, c in enumerate(cs) if got[0.05][i] != F.FAR and c.what == "random" and not (c.mpr and got[0.05][i] <= 0)]
    moved = [cs[i].moved(rand_rot(rng), rng.uniform(-1, 1, 3)) for i in pick]
    out = P.host_sep(moved, can, 0.05)
    n = {True: 0, False: 0}
    for i, d in zip(pick, out):
        c = cs[i]
        assert abs(d - got[0.05][i]) <= (1e-12 if P.closed(c) else 1e-9), (c.cls, d, got[0.05][i])
        n[P.closed(c)] += 1
    assert n[True] >= 150 and n[False] >= 80, n


@pytest.mark.parametrize("env", SUPPORTED_ENVS)
def test_margin_broad_phase_keeps_every_pair_in_band(env, oracle_mod):
    from mopa_rl_amd.scene import planner_inputs
    pi = planner_inputs(env)
    m = pi.model
    orc = oracle_mod.OracleScene(pi.model, pi.passive_joint_idx, pi.ignored_contacts, pi.spec.contact_threshold)
    qa = np.concatenate([sample_states(pi, 200, 3, "near")[0], sample_states(pi, 200, 4, "uniform")[0]])
    rows = sample_states(pi, 1, 3)[1]
    gpos, gmat = P.poses(pi, orc, qa, rows, len(qa))
    static = np.array([(gpos[:, g] == gpos[0, g]).all() for g in range(gpos.shape[1])])
    assert static.any() and not static.all()
    rb = P.rbound(m)
    kept = culled = 0
    for band in P.BANDS:
        D = P.pair_dists(pi, gpos, gmat, band)          # no cull of any kind in front
        for i in range(len(qa)):
            cull = P.culled_band(m, rb, static, gpos[i], gmat[i], band)
            hit = D[i] != F.FAR
            assert not (hit & cull).any(), (env, band, i, np.nonzero(hit & cull)[0])
            kept += int(hit.sum())
            culled += int(cull.sum())
    print(env, "pairs in band", kept, "pairs culled", culled)
    assert kept > 400 and culled > 400


def test_abi_symbols_and_status_codes():
    from mopa_rl_amd import _lib
    from mopa_rl_amd.batch import BatchPlanner, ProximityReport
    from mopa_rl_amd.planner import PyKinematicPlanner
    L = _lib.lib()
    for sym in ("mopa_proximity_batch", "mopa_proximity_state", "mopa_geom_sep_batch", "mopa_geom_sep_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and getattr(L, sym) is not None
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    t = np.zeros((1, 2), dtype=np.int32)
    r = np.zeros((1, 30))
    o = np.zeros(1)
    tp, rp, op = t.ctypes.data_as(ip), r.ctypes.data_as(dp), o.ctypes.data_as(dp)
    assert L.mopa_geom_sep_host(0, None, None, None, 0, 0.01, None) == 0
    assert L.mopa_geom_sep_host(-1, tp, rp, None, 0, 0.01, op) == 1                        # MOPA_ERR_INVALID_ARG
    assert L.mopa_geom_sep_host(1, None, rp, None, 0, 0.01, op) == 1 and L.mopa_geom_sep_host(1, tp, rp, None, 0, 0.01, None) == 1
    assert L.mopa_geom_sep_host(1, tp, rp, None, 3, 0.01, op) == 1 and b"null" in L.mopa_last_error()
    for band in (-1e-9, float("nan"), float("inf")):
        assert L.mopa_geom_sep_host(1, tp, rp, None, 0, band, op) == 1 and b"band" in L.mopa_last_error()
    assert L.mopa_geom_sep_host(1, tp, rp, None, 0, 0.01, op) == 0 and o[0] == F.FAR       # (plane, plane): not a pair the narrow phase serves
    assert L.mopa_geom_sep_batch(0, -1, None, None, None, 0, 0.01, None, None) == 1
    assert L.mopa_geom_sep_batch(0, 1, None, None, None, 0, 0.01, None, None) == 1
    assert L.mopa_proximity_batch(None, None, None, 1, 1, 0.01, 4, None, None, None, None, None) == 1
    assert L.mopa_proximity_state(None, None, 0.01, 4, None, None, None, None) == 1
    with pytest.raises(_lib.MopaError):
        _lib.geom_sep_host(np.zeros((2, 2)), np.zeros((1, 2, 15)), 0.01)
    assert tuple(ProximityReport(1, 2, 3, 4, None)) == (1, 2, 3, 4)
    # glue_bodies raises at all three levels, decided before the scene is touched
    pl = PyKinematicPlanner.__new__(PyKinematicPlanner)
    pl.glue_bodies = ["a", "b"]
    with pytest.raises(NotImplementedError):
        pl.proximity(np.zeros(3), 0.01)
    sc = _lib.Scene.__new__(_lib.Scene)
    sc.glue = (1, 2)
    with pytest.raises(NotImplementedError):
        sc.proximity_state(np.zeros(3), 0.01)
    bp = BatchPlanner.__new__(BatchPlanner)
    bp.scene = sc
    with pytest.raises(NotImplementedError):
        bp.proximity(None, None, band=0.01)
