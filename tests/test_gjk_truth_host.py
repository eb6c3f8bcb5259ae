"""gjk_distance's contract on the pairs whose distance is a formula (gjk_cases.py), host form (mopa_geom_sep_exact_host): a reported
value d satisfies  true <= d <= true + kGjkTol  -- one-sided, which is what makes band membership exact -- on parallel faces and
edges, curved on curved, plates, needles and coplanar hull vertices, at sizes from 5 mm to more than a metre; no case ends at the
iteration cap, and the cap is at least twice the largest number of support evaluations seen; a reported value has the same bits at both
bands and in either order of the pair.  The formulas themselves are checked against geom_ref.signed_dist on a sample.  No GPU.

E, the slack of every comparison with `true`, is derived, not measured: it is the rounding of building and moving the poses.  A case's
coordinates stay below 1 m (the translation) + 4 x 0.3 m (the largest shape) + 0.3 m (the gap) < 3 m, so one rounding is at most
2^-53 x 3 m = 3.3e-16 m; a pose is a handful of sums and products of such numbers (R p + t, R m, the supports and hypots of the formula,
rand_rot's orthogonality defect of a few ulp times a size, which is what scales with `scale`), a few dozen roundings in all, and the
golden-section search of the capsule-mesh truth stops within 1e-13 x 0.24 m of the minimiser of a function of slope <= 1.
E = 1e-12 x (1 + scale) covers several hundred roundings: enough by a wide margin, and six orders below kGjkTol."""
import numpy as np
import pytest

import frames_ref as F
import gjk_cases as G
import proximity_exact_ref as X
import proximity_ref as P
from geom_ref import BOX, CYLINDER, MESH, signed_dist

K_GJK_MAX_IT = 56         # kGjkMaxIt (mopa_gjk.hpp): by the project's rule at least twice the largest count measured


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def slack(its):
    return 1e-12 * (1.0 + np.array([it.scale for it in its]))


def check_truth(its, d, band, label):
    """the one-sided contract and band membership on [M] band-limited values `d`; prints the per-family deviations; -> the families' counts"""
    true, e = np.array([it.true for it in its]), slack(its)
    rep = d != F.FAR
    dev = np.where(rep, d - true, 0.0)
    bad = rep & ~((dev >= -e) & (dev <= X.K_GJK_TOL + e))
    fam = np.array([it.family for it in its])
    inside, outside = true <= band - e, true > band + e
    assert (inside | outside).all()                     # no case sits in the slack around the band's edge
    counts = {}
    for f in G.families(its):
        m = fam == f
        dv = dev[m & rep]
        counts[f] = (int((m & inside).sum()), int((m & outside).sum()))
        print(f"{label} band {band}: d - true, {f}: reported {len(dv)} of {int(m.sum())}, min = {dv.min():+.3e}, max = {dv.max():+.3e}")
        assert dv.min() >= -e[m].max(), (f, band, dv.min())
    show = lambda idx: [(its[i].family, its[i].scale, its[i].gap, its[i].variant, its[i].form, d[i], its[i].true) for i in np.nonzero(idx)[0][:8]]
    assert not bad.any(), (label, band, int(bad.sum()), show(bad))
    # membership: inside the band -> reported; outside -> FAR (a band-limited value is never above the band)
    assert not (inside & ~rep).any(), (label, band, show(inside & ~rep))
    assert not (outside & rep & ~(d > band)).any(), (label, band, show(outside & rep & ~(d > band)))
    for f, (n_in, n_out) in counts.items():
        assert n_in >= 6 and n_out >= 3, (f, band, n_in, n_out)
    return counts


@pytest.fixture(scope="module")
def can():
    from mopa_rl_amd.scene import load_scene
    return P.can_of(load_scene("sawyer_lift_obstacle"))


@pytest.fixture(scope="module")
def solved(can):
    """the items and, per band, the exact route's (distance, support evaluations)"""
    its = G.items(can)
    cs = [it.case for it in its]
    return its, {b: X.host_sep(cs, can, b, iters=True) for b in X.BANDS}


def test_the_sweep_is_what_it_says(solved):
    its, _ = solved
    fams = G.families(its)
    assert len(fams) == 34 and len(its) > 6000, (len(fams), len(its))
    assert {it.gap for it in its} == set(G.GAPS) and {it.scale for it in its} == set(G.SCALES)
    assert {it.form for it in its} == {"built", "moved1", "moved2", "swapped"}
    for cls in ("box-box", "capsule-cylinder", "cylinder-cylinder", "cylinder-box", "box-cylinder", "cylinder-capsule", "sphere-mesh", "capsule-mesh",
                "cylinder-mesh", "box-mesh"):
        assert any(it.case.cls == cls for it in its), cls
    assert all(not P.closed(it.case) for it in its)
    # plates and needles: an aspect ratio of 100 among a box's half extents and between a cylinder's radius and half height
    for t, k in ((BOX, 3), (CYLINDER, 2)):
        for variant, n_small in (("plate", 1), ("needle", k - 1)):
            sizes = [it.case.s1[:k] for it in its if it.variant == variant and it.case.t1 == t and it.family.startswith(("box-box", "cylinders"))]
            assert len(sizes) > 100 and all(int((s <= s.max() / 99.0).sum()) == n_small for s in sizes), (t, variant)


def test_contract_one_sided_and_band_membership(solved):
    its, ex = solved
    for band in X.BANDS:
        check_truth(its, ex[band][0], band, "host")


def test_the_check_can_fail(solved, can):
    its, ex = solved
    d = ex[0.05][0]
    rep = d != F.FAR
    # 1e-11 below the truth (the polytope pairs are exact to rounding); one tolerance above it
    for delta in (-1e-11, X.K_GJK_TOL):
        with pytest.raises(AssertionError):
            check_truth(its, np.where(rep, d + delta, d), 0.05, "shifted")
    # the inflated route, conservative but short of the distance by up to millimetres, is not within the contract
    with pytest.raises(AssertionError):
        check_truth(its, P.host_sep([it.case for it in its], can, 0.05), 0.05, "inflated")
    # a pair inside the band that is not reported
    gone = d.copy()
    gone[np.nonzero(rep)[0][0]] = F.FAR
    with pytest.raises(AssertionError):
        check_truth(its, gone, 0.05, "one dropped")


def test_no_case_ends_at_the_iteration_cap(solved):
    its, ex = solved
    true = np.array([it.true for it in its])
    top = 0
    for band in X.BANDS:
        d, n = ex[band]
        assert (n >= 0).all(), (band, [(its[i].family, its[i].scale, its[i].gap, its[i].variant, its[i].form, int(n[i])) for i in np.nonzero(n < 0)[0][:8]])
        # every case inside the band went through the exact route (the culls in front of it may answer for the others)
        assert (n[true <= band] > 0).all(), band
        top = max(top, int(n.max()))
    n = np.maximum(ex[0.01][1], ex[0.05][1])
    edges = (2, 4, 8, 12, 16, 24, 32, K_GJK_MAX_IT)
    print("support evaluations per run of the exact route (the larger of the two bands): family, scale: runs, median, max, then the counts <= " + ", ".join(map(str, edges)))
    for f in G.families(its):
        for s in G.SCALES:
            v = np.array([k for it, k in zip(its, n) if it.family == f and it.scale == s and k > 0])
            hist, lo = [], 0
            for hi in edges:
                hist.append(int(((v > lo) & (v <= hi)).sum()))
                lo = hi
            print(f"  {f}, {s}: {len(v)}, {int(np.median(v))}, {v.max()}, {hist}")
    print("largest number of support evaluations:", top)
    # the project's rule (mopa_gjk.hpp): kGjkMaxIt is at least twice the largest count measured
    assert 2 * top <= K_GJK_MAX_IT, top


def test_same_bits_at_both_bands_and_in_either_order(solved, can):
    its, ex = solved
    a, b = ex[0.01][0], ex[0.05][0]
    both = (a != F.FAR) & (b != F.FAR)
    assert both.sum() > 2000 and np.array_equal(_bits(a[both]), _bits(b[both])), [(its[i].family, a[i], b[i]) for i in np.nonzero(both & (_bits(a) != _bits(b)))[0][:8]]
    pick = [i for i, it in enumerate(its) if it.case.t2 != MESH]
    rev = X.host_sep([its[i].case.swapped() for i in pick], can, 0.05)
    bad = _bits(rev) != _bits(b[pick])
    assert not bad.any(), [(its[pick[k]].family, its[pick[k]].form, rev[k], b[pick[k]]) for k in np.nonzero(bad)[0][:8]]
    assert (rev != F.FAR).sum() > 3000


def reference_sample(its):
    """about 60 items at scale 1, plain variant: every family as built at the 0.0101 gap, and the first 26 families moved at 0.03"""
    pick = [it for it in its if it.scale == 1.0 and it.variant in ("plain", "end-on") and it.form == "built" and it.gap == 0.0101]
    fams = G.families(its)[:26]
    pick += [it for it in its if it.scale == 1.0 and it.variant in ("plain", "end-on") and it.form == "moved1" and it.gap == 0.03 and it.family in fams]
    return pick


def test_the_formulas_against_the_direction_search(solved, can):
    """the reference alone: a wrong formula can neither pass as a kernel bug nor hide one.  2e-7 is geom_ref.signed_dist's stated accuracy"""
    its, _ = solved
    pick = reference_sample(its)
    assert 55 <= len(pick) <= 65 and len({it.family for it in pick}) == 34, len(pick)
    worst = {}
    for it in pick:
        c = it.case
        ref = signed_dist(c.t1, c.s1, c.p1, c.m1, c.t2, can if c.t2 == MESH else c.s2, c.p2, c.m2)
        worst[it.family] = max(worst.get(it.family, 0.0), abs(ref - it.true))
        assert abs(ref - it.true) <= 2e-7, (it.family, it.form, it.gap, ref, it.true)
    print("largest |signed_dist - formula|:", max(worst.values()), "in", max(worst, key=worst.get))
