// mopa_witness.hpp -- witness points of the proximity report: for a posed pair, the two closest points and the unit direction
// between them that go with the distance geom_sep's exact route reports ("Proximity report", paragraph
// "Witness points").
//
// Numerics contract: mopa_device.hpp's (IEEE double, -ffp-contract=off, explicit fma only); one text for host and device, so the
// host compile (mopa_geom_witness_host) is the sequential form the kernels match bit for bit.
//
// geom_witness returns exactly the bits of geom_sep<MESH, G, /*EXACT=*/true> and, when that is not kFar, p1 on (or in) the first
// shape, p2 on the second and the unit vector n from the first towards the second:
//   overlap or touching (d <= 0, geom_dist's value)   geom_frame's normal; p1 = pos - (d/2) n, p2 = pos + (d/2) n: the contact
//                  frame's own definition (w2 - w1 = dist n, pos their midpoint) read the other way round.
//   separated, closed form (sep_closed_form)   the same two lines.  Separated shapes take the OUTSIDE branch of every f_* routine of
//                  mopa_frames.hpp -- the clamp residual, the segment parameters, the plane's deepest point -- and that branch
//                  forms w1 on A, w2 on B with w2 - w1 = d n at any sign of d; its distance is geom_dist's expression, so d's
//                  bits are geom_sep's.  No routine was missing.
//   separated, GJK classes (box-box, PC_CONVEX, PC_CONVEX_MESH)   gjk_witness below: gjk_distance's walk, the same operations on
//                  the same simplex in the same order -- so the same iterates and the same returned bits -- with every simplex
//                  vertex carrying the support point of A it came from (B's is A's minus the vertex).  At every exit the
//                  barycentric weights of v in the KEPT simplex (the one to three vertices that carry v; gjk_weights: the
//                  expressions gjk_seg / gjk_tri placed v by) are clamped to >= 0 and renormalised, so p1 = sum l_i a_i and
//                  p2 = sum l_i b_i are convex combinations of points of the shapes whatever the conditioning;
//                  n = (p2 - p1) / |p2 - p1|.  The exits that do not return |v| -- `return 0.0` (|v| < kMinVal, the origin
//                  enclosed) and the iteration cap -- return the kept simplex's points all the same and unit_or_x for the
//                  normal (world x when the two points coincide): a point of each shape, not a closest pair.
// Order: geom_sep's flip (two shapes of one type go into the GJK walk by the order of their sizes) and geom_witness_pair's
// type-order swap are undone on the way out -- p1 / p2 exchanged, n negated -- so p1 always belongs to the first shape as given;
// giving such a pair in the other order returns p1 and p2 exchanged and n negated, bit for bit.  (Capsule-capsule has neither:
// d_capsule_capsule evaluates the two axes in the order given, and so does its witness.)
// d == kFar: n = p1 = p2 = 0.
#pragma once
#include "mopa_device.hpp"
#include "mopa_frames.hpp"
#include "mopa_gjk.hpp"
#include "mopa_sep.hpp"

namespace mopa {

// the weights of the origin's closest point in the kept simplex p0 .. p(n-1), n in 1..3: >= 0, summing to 1
MOPA_HD void gjk_weights(int n, V3 p0, V3 p1, V3 p2, double &l0, double &l1, double &l2) {
    l0 = 1.0; l1 = 0.0; l2 = 0.0;
    if (n == 2) {
        // gjk_seg's parameter
        const V3 d = sub3(p1, p0);
        const double dd = dot3(d, d), t = -dot3(p0, d);
        if (dd > 0.0) l1 = clampd(t / dd, 0.0, 1.0);
        l0 = 1.0 - l1;
    } else if (n == 3) {
        // gjk_tri's barycentric signs: their sum is the squared normal
        const V3 nn = cross3(sub3(p1, p0), sub3(p2, p0));
        const double w0 = dmax(dot3(cross3(p1, p2), nn), 0.0), w1 = dmax(dot3(cross3(p2, p0), nn), 0.0), w2 = dmax(dot3(cross3(p0, p1), nn), 0.0);
        const double sum = (w0 + w1) + w2;
        if (sum > 0.0) {
            const double inv = 1.0 / sum;
            l0 = w0 * inv; l1 = w1 * inv; l2 = w2 * inv;
        }
    }
}
MOPA_HD void gjk_witness_out(int n, V3 p0, V3 p1, V3 p2, V3 a0, V3 a1, V3 a2, V3 &wa, V3 &wb) {
    double l0, l1, l2;
    gjk_weights(n, p0, p1, p2, l0, l1, l2);
    wa = scl3(a0, l0);
    wb = scl3(sub3(a0, p0), l0);
    if (n > 1) { wa = addscl3(wa, a1, l1); wb = addscl3(wb, sub3(a1, p1), l1); }
    if (n > 2) { wa = addscl3(wa, a2, l2); wb = addscl3(wb, sub3(a2, p2), l2); }
}

// gjk_distance (mopa_gjk.hpp) with the witness: the same walk, returning the same bits; wa on A, wb on B.  A sibling, not a
// switch inside gjk_distance: the report and planner kernels inline that one and keep their register budgets.
template <bool MESH = false, int G = 1>
MOPA_HD double gjk_witness(const double *A, int ta, const double *B, int tb, double band, const double *aux, V3 &wa, V3 &wb, int *iters = nullptr) {
    V3 v0 = sub3(ld3(A + GO_POS), ld3(B + GO_POS));
    if (vec_eq0(v0)) v0.x += kCcdEps * 10.0;
    V3 dir = normalize3(neg3(v0));
    V3 a0 = support_geom<false>(A, ta, dir), a1 = a0, a2 = a0;
    V3 p0 = sub3(a0, support_geom<MESH, G>(B, tb, neg3(dir), aux)), p1 = p0, p2 = p0;       // support_md's two halves
    int n = 1;
    V3 v = p0;
    double vv = dot3(v, v), lb = -kFar;
    wa = V3{0.0, 0.0, 0.0};
    wb = V3{0.0, 0.0, 0.0};
    // every exit but kFar's leaves the loop with the value to return and meets the others at the one reconstruction below
    double ret = -1.0;      // (the cap's mark: no exit returns a negative value)
    for (int it = 1; it < kGjkMaxIt; it++) {
        const double nv = sqrt(vv);
        if (nv < kMinVal) { if (iters) *iters = it; ret = 0.0; break; }
        const double inv = 1.0 / nv;
        dir = V3{-v.x * inv, -v.y * inv, -v.z * inv};
        V3 a3 = support_geom<false>(A, ta, dir);
        const V3 w = sub3(a3, support_geom<MESH, G>(B, tb, neg3(dir), aux));
        if (iters) *iters = it + 1;
        const double vw = dot3(v, w);
        lb = dmax(lb, vw / nv);
        if (lb > band) return kFar;
        if (nv - lb <= kGjkTol) { ret = nv; break; }
        if (gjk_same(w, p0) || (n > 1 && gjk_same(w, p1)) || (n > 2 && gjk_same(w, p2)) || !(vw < vv)) { ret = nv; break; }
        V3 c = v, p3 = w;
        double cc = kFar * kFar;
        int mask = 0;
        // (w joins the simplex behind the n kept vertices, which stay where they are until the reduction below: the two exits in
        //  between leave with the kept simplex)
        if (n == 1) {
            p1 = w; a1 = a3;
            gjk_seg(p0, 1, p1, 2, c, cc, mask);
        } else if (n == 2) {
            p2 = w; a2 = a3;
            gjk_tri(p0, 1, p1, 2, p2, 4, c, cc, mask);
        } else {
            if (gjk_tet(p0, p1, p2, p3, c, cc, mask)) { ret = 0.0; break; }
        }
        if (!(cc < vv)) { ret = nv; break; }
        v = c;
        vv = cc;
        for (int pass = 0; pass < 3; pass++) {
            bool s = !(mask & 1) && (mask & 2);
            gjk_swap_if(s, p0, p1); gjk_swap_if(s, a0, a1);
            if (s) mask ^= 3;
            s = !(mask & 2) && (mask & 4);
            gjk_swap_if(s, p1, p2); gjk_swap_if(s, a1, a2);
            if (s) mask ^= 6;
            s = !(mask & 4) && (mask & 8);
            gjk_swap_if(s, p2, p3); gjk_swap_if(s, a2, a3);
            if (s) mask ^= 12;
        }
        n = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
    }
    if (ret < 0.0) {
        if (iters) *iters = -kGjkMaxIt;
        ret = dmax(lb, 0.0);
    }
    gjk_witness_out(n, p0, p1, p2, a0, a1, a2, wa, wb);
    return ret;
}

// (A, B) in the narrow phase's order, as geom_sep takes them
template <bool MESH = false, int G = 1>
MOPA_HD double geom_witness(int code, const double *A, int ta, const double *B, int tb, double band, const double *aux, V3 &n, V3 &p1, V3 &p2,
                            int *iters = nullptr) {
    V3 pos;
    const double d0 = geom_frame<MESH>(code, A, ta, B, tb, aux, n, pos);      // geom_dist's bits, and the frame where d0 != kFar
    double d = d0;
    bool gjk = false, flip = false;
    if (d0 > 0.0) {
        // geom_sep's rules for separated shapes, in its order
        if (sep_closed_form(code)) d = (d0 <= band) ? d0 : kFar;
        else if (!(band > 0.0)) d = kFar;
        else if (MESH && code == PC_CONVEX_MESH) {
            d = sep_in_band(gjk_witness<MESH, G>(A, ta, B, tb, band, aux, p1, p2, iters), band);
            gjk = true;
        } else {
            bool cull = true;
            if (code == PC_BOX_BOX) cull = d0 > band + 1e-9;
            else if (code == PC_CONVEX) cull = ((tb == G_BOX) ? d_capsule_box(A, B) : d_capsule_capsule(A, B)) > band + 1e-9;
            if (cull) d = kFar;
            else {
                flip = ta == tb && size_before(B, A);
                if (flip) d = sep_in_band(gjk_witness<false, 1>(B, ta, A, tb, band, nullptr, p2, p1, iters), band);
                else d = sep_in_band(gjk_witness<false, 1>(A, ta, B, tb, band, nullptr, p1, p2, iters), band);
                gjk = true;
            }
        }
    }
    if (d == kFar) {
        n = V3{0.0, 0.0, 0.0};
        p1 = V3{0.0, 0.0, 0.0};
        p2 = V3{0.0, 0.0, 0.0};
    } else if (gjk) {
        // (in the order the walk took the shapes, then undone: world x for coincident points is negated with the rest)
        const V3 u = flip ? sub3(p1, p2) : sub3(p2, p1);
        n = unit_or_x(u, norm3(u));
        if (flip) n = neg3(n);
    } else {
        p1 = addscl3(pos, n, -(0.5 * d));
        p2 = addscl3(pos, n, 0.5 * d);
    }
    return d;
}

// One posed pair given by its two types in ANY order (geom_sep_pair's rule): evaluated in pair_code's canonical order, p1 / p2
// exchanged and the normal negated on the way out when that is the reverse.  out[10] = d, n[3], p1[3], p2[3]; an unsupported
// type pair reports kFar.
template <bool MESH>
MOPA_HD void geom_witness_pair(int t1, const double *r1, int t2, const double *r2, double band, const double *aux, double *out, int *iters = nullptr) {
    int code = pair_code(t1, t2);
    bool swapped = false;
    if (code < 0) { code = pair_code(t2, t1); swapped = true; }
    V3 n{0.0, 0.0, 0.0}, p1{0.0, 0.0, 0.0}, p2{0.0, 0.0, 0.0};
    double d = kFar;
    if (code >= 0) d = swapped ? geom_witness<MESH, 1>(code, r2, t2, r1, t1, band, aux, n, p2, p1, iters) : geom_witness<MESH, 1>(code, r1, t1, r2, t2, band, aux, n, p1, p2, iters);
    if (swapped && d != kFar) n = neg3(n);
    out[0] = d;
    out[1] = n.x; out[2] = n.y; out[3] = n.z;
    out[4] = p1.x; out[5] = p1.y; out[6] = p1.z;
    out[7] = p2.x; out[8] = p2.y; out[9] = p2.z;
}

// the same from two bare records [15] (geom_sep_rec's rule: a mesh, either side, reads the hull at mesh_verts)
MOPA_HD void geom_witness_rec(int t1, const double *r1, int t2, const double *r2, const double *mesh_verts, int nvert, double band, double *out, int *iters = nullptr) {
    const bool first_mesh = t1 == G_MESH;
    if (first_mesh) {
        const int t = t1; t1 = t2; t2 = t;
        const double *r = r1; r1 = r2; r2 = r;
    }
    if (t2 == G_MESH && nvert > 0) {
        double rm[15];
        for (int i = 0; i < 15; i++) rm[i] = r2[i];
        rm[GO_SIZE] = 0.0; rm[GO_SIZE + 1] = (double)nvert; rm[GO_SIZE + 2] = 0.0;
        geom_witness_pair<true>(t1, r1, t2, rm, band, mesh_verts, out, iters);
    } else {
        geom_witness_pair<false>(t1, r1, t2, r2, band, nullptr, out, iters);
    }
    if (first_mesh && out[0] != kFar)
        for (int i = 0; i < 3; i++) {
            out[1 + i] = -out[1 + i];
            const double t = out[4 + i];
            out[4 + i] = out[7 + i];
            out[7 + i] = t;
        }
}

}  // namespace mopa
