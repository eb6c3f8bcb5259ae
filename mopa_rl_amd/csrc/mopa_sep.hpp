// mopa_sep.hpp -- band-limited separation: for a posed pair, the signed distance if it is <= band, kFar otherwise.
//
// Numerics contract: mopa_device.hpp's.  geom_sep calls geom_dist first and hands its value on untouched whenever the shapes
// overlap, so a pair in overlap carries the contact report's bits.  For separated shapes ("Proximity report"):
//   closed form    plane-X, sphere-X, capsule-capsule, capsule-box, plane-mesh: the pair function's positive value IS the
//                  separation distance; it is kept when it is <= band.
//   inflated       box-box (whose positive value is a separating-axis gap, a lower bound of the distance), PC_CONVEX and
//                  PC_CONVEX_MESH (whose pair function says nothing about disjoint shapes): MuJoCo's rule for `margin` on convex
//                  pairs -- the portal refinement on the two shapes inflated by band / 2 each, i.e. on the Minkowski difference
//                  with support support_md(dir) + band * dir, and band taken off its depth again.  The refinement is
//                  mpr_penetration itself (INFL = true); its loops keep their bounds.  The depth is never less than the true
//                  depth minus kMprTol, so the distance never exceeds the true one by more than that: a conservative clearance.
//                  The portal's depth is the one along the centre line's portal, not the least one: the distance falls short of
//                  the true one by an amount that grows with band (measured per class in DESIGN.md), so it depends on band.
//   exact          EXACT = true (opt-in): the same three classes, the same culls in front, but gjk_distance (mopa_gjk.hpp) on the shapes
//                  as they are in place of the inflated refinement: true <= d <= true + kGjkTol, the same bits at every band that
//                  reports the pair, whichever order the pair is given in.  EXACT = false compiles to the code it was before.
// The host compile of these functions (mopa_geom_sep_host) is the sequential form the kernels must match bit for bit.
#pragma once
#include "mopa_device.hpp"
#include "mopa_gjk.hpp"

namespace mopa {

// the classes whose pair function is the separation distance of disjoint shapes
MOPA_HD bool sep_closed_form(int code) { return (code >= 0 && code < PC_BOX_BOX) || code == PC_PLANE_MESH; }

// lexicographic order of two records' sizes
MOPA_HD bool size_before(const double *X, const double *Y) {
    for (int i = 0; i < 3; i++)
        if (X[GO_SIZE + i] != Y[GO_SIZE + i]) return X[GO_SIZE + i] < Y[GO_SIZE + i];
    return false;
}

// the exact route's value: the distance when it is inside the band
MOPA_HD double sep_in_band(double d, double band) { return (d <= band) ? d : kFar; }

// iters (EXACT only, optional): the exact route's number of support evaluations, negative where its cap ended it; untouched where
// the route is not taken
template <bool MESH = false, int G = 1, bool EXACT = false>
MOPA_HD double geom_sep(int code, const double *A, int ta, const double *B, int tb, double band, const double *aux = nullptr, int *iters = nullptr) {
    const double d0 = geom_dist<MESH, G>(code, A, ta, B, tb, aux);
    if (d0 <= 0.0) return d0;
    if (sep_closed_form(code)) return (d0 <= band) ? d0 : kFar;
    if (!(band > 0.0)) return kFar;
    double p = 0.0;
    if (EXACT && MESH && code == PC_CONVEX_MESH) return sep_in_band(gjk_distance<MESH, G>(A, ta, B, tb, band, aux, iters), band);
    if (MESH && code == PC_CONVEX_MESH) return mpr_penetration<MESH, G, true>(A, ta, B, tb, p, aux, band) ? dmax(band - p, 0.0) : kFar;
    // conservative culls in front of the refinement: lower bounds of the distance against band + 1e-9
    if (code == PC_BOX_BOX) {
        if (d0 > band + 1e-9) return kFar;                // the gap along a unit separating axis
    } else if (code == PC_CONVEX) {
        const double pre = (tb == G_BOX) ? d_capsule_box(A, B) : d_capsule_capsule(A, B);       // the enclosing capsules
        if (pre > band + 1e-9) return kFar;
    } else {
        return kFar;
    }
    // (the refinement is not symmetric in its two shapes: two shapes of ONE type go in by the order of their sizes -- which neither the
    //  order they are given in nor a rigid motion changes -- and as given when they are equal)
    const bool flip = ta == tb && size_before(B, A);
    if (EXACT) return sep_in_band(gjk_distance<false, 1>(flip ? B : A, ta, flip ? A : B, tb, band, nullptr, iters), band);
    return mpr_penetration<false, 1, true>(flip ? B : A, ta, flip ? A : B, tb, p, nullptr, band) ? dmax(band - p, 0.0) : kFar;
}

// a pair given in either type order; the value does not depend on the order
template <bool MESH, bool EXACT = false>
MOPA_HD double geom_sep_pair(int t1, const double *r1, int t2, const double *r2, double band, const double *aux, int *iters = nullptr) {
    int code = pair_code(t1, t2);
    if (code >= 0) return geom_sep<MESH, 1, EXACT>(code, r1, t1, r2, t2, band, aux, iters);
    code = pair_code(t2, t1);
    if (code >= 0) return geom_sep<MESH, 1, EXACT>(code, r2, t2, r1, t1, band, aux, iters);
    return kFar;
}

// the same from two bare records [15] = pos[3] mat[9] size[3]: a mesh (type 7, either side) has its size slots replaced by where
// its hull lives -- offset 0 of mesh_verts, nvert vertices
template <bool EXACT = false>
MOPA_HD double geom_sep_rec(int t1, const double *r1, int t2, const double *r2, const double *mesh_verts, int nvert, double band, int *iters = nullptr) {
    if (t1 == G_MESH) {
        const int t = t1; t1 = t2; t2 = t;
        const double *r = r1; r1 = r2; r2 = r;
    }
    if (t2 == G_MESH && nvert > 0) {
        double rm[15];
        for (int i = 0; i < 15; i++) rm[i] = r2[i];
        rm[GO_SIZE] = 0.0; rm[GO_SIZE + 1] = (double)nvert; rm[GO_SIZE + 2] = 0.0;
        return geom_sep_pair<true, EXACT>(t1, r1, t2, rm, band, mesh_verts, iters);
    }
    return geom_sep_pair<false, EXACT>(t1, r1, t2, r2, band, nullptr, iters);
}

}  // namespace mopa
