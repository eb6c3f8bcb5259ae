// mopa_gjk.hpp -- gjk_distance: the exact separation distance of two disjoint convex shapes, band-limited (DESIGN.md section 4,
// "Proximity report", paragraph "Exact route").
//
// Numerics contract: mopa_device.hpp's (FP64, -ffp-contract=off, explicit fma only); one text for host and device, so the host
// compile is the sequential form the kernels match bit for bit.
// GJK on the Minkowski difference A - B through support_md -- the shapes as they are, no inflation.  The simplex holds at most
// four points and no witness points: only the distance is wanted.  Per iteration: v = the simplex's point closest to the origin,
// w = support_md(-v / |v|), lb = (v . w) / |v| -- the origin's distance to the supporting plane of A - B with normal -v / |v|, a
// lower bound of the distance -- kept as a running maximum; |v| is the distance of a point OF A - B, an upper bound.  Exits, in
// this order:
//   lb > band                        kFar: the distance is at least lb, so membership in the band is decided exactly
//   |v| - lb <= kGjkTol              |v|
//   w adds nothing                   |v|: w is already a simplex vertex, v . w is not below v . v (the support found nothing
//                                    nearer the origin's side than v itself), or the new simplex's closest point is not nearer
//   |v| < kMinVal / origin enclosed  0.0 (|v| is tested before it divides: ahead of the support evaluation of its iteration)
//   kGjkMaxIt support evaluations    the running lb (not below 0): never above the distance; *iters = -kGjkMaxIt
// so a returned d has  true <= d <= true + kGjkTol  except at the cap.  `band` is read by the first exit only: the iterates, and
// with them the bits of a reported value, do not depend on it.
// Closest point of the simplex (gjk_seg / gjk_tri / gjk_tet): candidates by feature, the nearest one kept -- the foot of the
// origin on a triangle's plane where its barycentric signs say it lies inside, a segment's interior foot where its parameter lies
// in (0, 1), the vertices otherwise.  Every divisor is tested before it is used: a segment's squared length against 0, a
// triangle's squared normal against kGjkDegen2 x its edges' squared lengths (else it is three segments), a tetrahedron's squared
// volume against kGjkDegen2 x base x edge (else it is four triangles).  Repeated and collinear support points -- the usual case
// for boxes and hulls -- are therefore reduced, never divided by; the vertices that do not carry the closest point are dropped.
// Every loop is bounded by kGjkMaxIt.
#pragma once
#include "mopa_device.hpp"

namespace mopa {

constexpr double kGjkTol = kMprTol;
// twice the largest number of support evaluations measured ("Exact route": histogram per class), rounded up to 8
constexpr int kGjkMaxIt = 56;
// squared sine below which a triangle counts as collinear / a tetrahedron as flat (an angle of 1e-8)
constexpr double kGjkDegen2 = 1e-16;

MOPA_HD void gjk_offer(V3 c, int m, V3 &v, double &vv, int &mask) {
    const double cc = dot3(c, c);
    if (cc < vv) { v = c; vv = cc; mask = m; }
}
// the origin's closest point on segment a-b
MOPA_HD void gjk_seg(V3 a, int ma, V3 b, int mb, V3 &v, double &vv, int &mask) {
    const V3 d = sub3(b, a);
    const double dd = dot3(d, d), t = -dot3(a, d);
    if (!(dd > 0.0) || !(t > 0.0)) gjk_offer(a, ma, v, vv, mask);
    else if (t >= dd) gjk_offer(b, mb, v, vv, mask);
    else gjk_offer(addscl3(a, d, t / dd), ma | mb, v, vv, mask);
}
// ... on triangle a-b-c
MOPA_HD void gjk_tri(V3 a, int ma, V3 b, int mb, V3 c, int mc, V3 &v, double &vv, int &mask) {
    const V3 ab = sub3(b, a), ac = sub3(c, a), n = cross3(ab, ac);
    const double nn = dot3(n, n);
    if (nn > kGjkDegen2 * dot3(ab, ab) * dot3(ac, ac)) {
        // barycentric signs of the origin's foot on the plane
        if (dot3(cross3(b, c), n) >= 0.0 && dot3(cross3(c, a), n) >= 0.0 && dot3(cross3(a, b), n) >= 0.0) {
            const double s = dot3(a, n) / nn;
            gjk_offer(V3{n.x * s, n.y * s, n.z * s}, ma | mb | mc, v, vv, mask);
            return;
        }
    }
    gjk_seg(a, ma, b, mb, v, vv, mask);
    gjk_seg(a, ma, c, mc, v, vv, mask);
    gjk_seg(b, mb, c, mc, v, vv, mask);
}
// ... on tetrahedron a-b-c-d (mask bits 1, 2, 4, 8); true: the origin is enclosed
MOPA_HD bool gjk_tet(V3 a, V3 b, V3 c, V3 d, V3 &v, double &vv, int &mask) {
    const V3 ab = sub3(b, a), ac = sub3(c, a), ad = sub3(d, a);
    const V3 nabc = cross3(ab, ac), nabd = cross3(ab, ad), nacd = cross3(ac, ad), nbcd = cross3(sub3(c, b), sub3(d, b));
    const double det = dot3(nabc, ad);
    const bool flat = !(det * det > kGjkDegen2 * dot3(nabc, nabc) * dot3(ad, ad));
    const double sg = det > 0.0 ? 1.0 : -1.0;
    // a face is a candidate when the origin is not strictly on its inner side (the side of the opposite vertex)
    const bool o_abc = flat || !(-dot3(nabc, a) * sg > 0.0);
    const bool o_abd = flat || !(dot3(nabd, a) * sg > 0.0);
    const bool o_acd = flat || !(-dot3(nacd, a) * sg > 0.0);
    const bool o_bcd = flat || !(dot3(nbcd, b) * sg > 0.0);
    if (!(o_abc || o_abd || o_acd || o_bcd)) return true;
    if (o_abc) gjk_tri(a, 1, b, 2, c, 4, v, vv, mask);
    if (o_abd) gjk_tri(a, 1, b, 2, d, 8, v, vv, mask);
    if (o_acd) gjk_tri(a, 1, c, 4, d, 8, v, vv, mask);
    if (o_bcd) gjk_tri(b, 2, c, 4, d, 8, v, vv, mask);
    return false;
}
MOPA_HD bool gjk_same(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
MOPA_HD void gjk_swap_if(bool c, V3 &a, V3 &b) {
    const V3 t = a;
    if (c) { a = b; b = t; }
}

// A, B: posed records as support_md takes them (a mesh is B).  *iters (optional): the number of support evaluations, -kGjkMaxIt at the cap.
template <bool MESH = false, int G = 1>
MOPA_HD double gjk_distance(const double *A, int ta, const double *B, int tb, double band, const double *aux, int *iters = nullptr) {
    // the start direction is the centre line as mpr_penetration takes it
    V3 v0 = sub3(ld3(A + GO_POS), ld3(B + GO_POS));
    if (vec_eq0(v0)) v0.x += kCcdEps * 10.0;
    V3 p0 = support_md<MESH, G>(A, ta, B, tb, normalize3(neg3(v0)), aux), p1 = p0, p2 = p0;      // (at most three points survive an iteration)
    int n = 1;
    V3 v = p0;
    double vv = dot3(v, v), lb = -kFar;
    for (int it = 1; it < kGjkMaxIt; it++) {
        const double nv = sqrt(vv);
        if (nv < kMinVal) { if (iters) *iters = it; return 0.0; }
        const double inv = 1.0 / nv;
        const V3 w = support_md<MESH, G>(A, ta, B, tb, V3{-v.x * inv, -v.y * inv, -v.z * inv}, aux);
        if (iters) *iters = it + 1;
        const double vw = dot3(v, w);
        lb = dmax(lb, vw / nv);
        if (lb > band) return kFar;
        if (nv - lb <= kGjkTol) return nv;
        if (gjk_same(w, p0) || (n > 1 && gjk_same(w, p1)) || (n > 2 && gjk_same(w, p2)) || !(vw < vv)) return nv;
        // the closest point of the simplex with w
        V3 c = v, p3 = w;
        double cc = kFar * kFar;
        int mask = 0;
        if (n == 1) {
            p1 = w;
            gjk_seg(p0, 1, p1, 2, c, cc, mask);
        } else if (n == 2) {
            p2 = w;
            gjk_tri(p0, 1, p1, 2, p2, 4, c, cc, mask);
        } else {
            if (gjk_tet(p0, p1, p2, p3, c, cc, mask)) return 0.0;
        }
        if (!(cc < vv)) return nv;
        v = c;
        vv = cc;
        // drop the vertices that do not carry v: the kept ones move to the front, in order
        for (int pass = 0; pass < 3; pass++) {
            bool s = !(mask & 1) && (mask & 2);
            gjk_swap_if(s, p0, p1);
            if (s) mask ^= 3;
            s = !(mask & 2) && (mask & 4);
            gjk_swap_if(s, p1, p2);
            if (s) mask ^= 6;
            s = !(mask & 4) && (mask & 8);
            gjk_swap_if(s, p2, p3);
            if (s) mask ^= 12;
        }
        n = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
    }
    if (iters) *iters = -kGjkMaxIt;
    return dmax(lb, 0.0);
}

}  // namespace mopa
