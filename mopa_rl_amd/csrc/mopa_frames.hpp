// mopa_frames.hpp -- contact frames: for a posed pair, the contact normal and point that go with the distance geom_dist reports.
//
// Numerics contract: mopa_device.hpp's (IEEE double, -ffp-contract=off, explicit fma only, mopa_sincos never libm).  Every routine
// here forms its distance by the SAME expressions, in the same order, as the distance routine it sits next to, so the value it
// returns has the bits of geom_dist; the host compile of these functions (mopa_geom_frames_host) is the sequential form the
// kernels must match bit for bit.
//
// Definition ("Contact report"; PARITY UNPINNED): ONE frame per pair, that of the deepest contact.  For the
// pair (A, B) as the narrow phase orders it: `n` is a unit vector from A towards B -- translating B by -dist * n (dist < 0)
// removes the overlap along n -- and `pos` is the midpoint of two witness points w1 on A, w2 on B with w2 - w1 = dist * n.  The
// witness is the one the distance function determines implicitly: the clamp residual, the SAT axis that won (the first on
// ties), the portal's closest point to the origin (what libccd's ccdMPRPenetration returns besides the depth).
#pragma once
#include "mopa_device.hpp"

namespace mopa {

MOPA_HD V3 mid3(V3 a, V3 b) { return V3{0.5 * (a.x + b.x), 0.5 * (a.y + b.y), 0.5 * (a.z + b.z)}; }
MOPA_HD V3 scl3(V3 a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
// v / len, world x when the vector is zero
MOPA_HD V3 unit_or_x(V3 v, double len) {
    if (!(len > 0.0)) return V3{1.0, 0.0, 0.0};
    const double inv = 1.0 / len;
    return V3{v.x * inv, v.y * inv, v.z * inv};
}
// sign with a zero counting as +
MOPA_HD double sgnp(double x) { return (x < 0.0) ? -1.0 : 1.0; }
MOPA_HD double comp3(V3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
MOPA_HD V3 axis3(int i, double s) { return V3{i == 0 ? s : 0.0, i == 1 ? s : 0.0, i == 2 ? s : 0.0}; }
// w1 = w2 - dist n; pos = their midpoint
MOPA_HD V3 pos_from_w2(V3 w2, V3 n, double dist) { return mid3(addscl3(w2, n, -dist), w2); }
MOPA_HD V3 pos_from_w1(V3 w1, V3 n, double dist) { return mid3(w1, addscl3(w1, n, dist)); }

// ---------------------------------------------------------------------------
// plane - X: n = the plane's z column; w2 = the deepest point of X, w1 = w2 - dist n
// ---------------------------------------------------------------------------
MOPA_HD double f_plane_sphere(const double *P, const double *S, V3 &n, V3 &pos) {
    n = col3(P + GO_MAT, 2);
    V3 diff = sub3(ld3(S + GO_POS), ld3(P + GO_POS));
    const double dist = dot3(diff, n) - S[GO_SIZE];
    pos = pos_from_w2(addscl3(ld3(S + GO_POS), n, -S[GO_SIZE]), n, dist);
    return dist;
}
MOPA_HD double f_plane_capsule(const double *P, const double *C, V3 &n, V3 &pos) {
    n = col3(P + GO_MAT, 2);
    V3 a = col3(C + GO_MAT, 2);
    V3 cp = ld3(C + GO_POS), pp = ld3(P + GO_POS);
    V3 e1 = addscl3(cp, a, C[GO_SIZE + 1]);
    double d1 = dot3(sub3(e1, pp), n) - C[GO_SIZE];
    V3 e2 = addscl3(cp, a, -C[GO_SIZE + 1]);
    double d2 = dot3(sub3(e2, pp), n) - C[GO_SIZE];
    const bool first = d1 < d2;          // the end dmin(d1, d2) returned
    const double dist = first ? d1 : d2;
    pos = pos_from_w2(addscl3(first ? e1 : e2, n, -C[GO_SIZE]), n, dist);
    return dist;
}
MOPA_HD double f_plane_cylinder(const double *P, const double *C, V3 &n, V3 &pos) {
    n = col3(P + GO_MAT, 2);
    V3 a = col3(C + GO_MAT, 2);
    V3 diff = sub3(ld3(C + GO_POS), ld3(P + GO_POS));
    double d0 = dot3(diff, n);
    double na = dot3(n, a);
    double s2 = fma(-na, na, 1.0);
    double sr = (s2 > 0.0) ? sqrt(s2) : 0.0;
    const double dist = (d0 - C[GO_SIZE + 1] * fabs(na)) - C[GO_SIZE] * sr;
    // the deepest rim point: c - signd(n.a) h a - r (n - (n.a) a) / sr
    V3 w2 = addscl3(ld3(C + GO_POS), a, -(signd(na) * C[GO_SIZE + 1]));
    if (sr > 0.0) w2 = addscl3(w2, addscl3(n, a, -na), -(C[GO_SIZE] / sr));
    pos = pos_from_w2(w2, n, dist);
    return dist;
}
MOPA_HD double f_plane_box(const double *P, const double *B, V3 &n, V3 &pos) {
    n = col3(P + GO_MAT, 2);
    V3 diff = sub3(ld3(B + GO_POS), ld3(P + GO_POS));
    double d0 = dot3(diff, n);
    double ext = 0.0;
    V3 w2 = ld3(B + GO_POS);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const V3 u = col3(B + GO_MAT, i);
        const double nu = dot3(n, u);
        ext = fma(fabs(nu), B[GO_SIZE + i], ext);
        w2 = addscl3(w2, u, -(signd(nu) * B[GO_SIZE + i]));      // signd(0) = 0: a flat contact gives the face or edge centre
    }
    const double dist = d0 - ext;
    pos = pos_from_w2(w2, n, dist);
    return dist;
}
MOPA_HD double f_plane_mesh(const double *P, const double *M, const double *aux, V3 &n, V3 &pos) {
    n = col3(P + GO_MAT, 2);
    const V3 ln = matT_vec(M + GO_MAT, n);
    const double *V = aux + (int)M[GO_SIZE];
    const int nv = (int)M[GO_SIZE + 1];
    int best = 0;
    double bd = dot3(ln, ld3(V));
    for (int i = 1; i < nv; i++) {
        const double d = dot3(ln, ld3(V + 3 * i));
        if (d < bd) { bd = d; best = i; }
    }
    const V3 w = add3(mat_vec(M + GO_MAT, ld3(V + 3 * best)), ld3(M + GO_POS));
    const double dist = dot3(sub3(w, ld3(P + GO_POS)), n);
    pos = pos_from_w2(w, n, dist);
    return dist;
}

// ---------------------------------------------------------------------------
// round shapes: n along the closest-point difference, the points on the centres / axes offset by the radii
// ---------------------------------------------------------------------------
MOPA_HD double f_sphere_sphere(const double *A, const double *B, V3 &n, V3 &pos) {
    V3 diff = sub3(ld3(B + GO_POS), ld3(A + GO_POS));
    const double len = norm3(diff);
    n = unit_or_x(diff, len);
    pos = mid3(addscl3(ld3(A + GO_POS), n, A[GO_SIZE]), addscl3(ld3(B + GO_POS), n, -B[GO_SIZE]));
    return len - (A[GO_SIZE] + B[GO_SIZE]);
}
MOPA_HD double f_sphere_capsule(const double *S, const double *C, V3 &n, V3 &pos) {
    V3 a = col3(C + GO_MAT, 2);
    V3 sp = ld3(S + GO_POS), cp = ld3(C + GO_POS);
    V3 vec = sub3(sp, cp);
    double x = clampd(dot3(a, vec), -C[GO_SIZE + 1], C[GO_SIZE + 1]);
    V3 pt = addscl3(cp, a, x);
    const double len = norm3(sub3(sp, pt));
    n = unit_or_x(sub3(pt, sp), len);
    pos = mid3(addscl3(sp, n, S[GO_SIZE]), addscl3(pt, n, -C[GO_SIZE]));
    return len - (S[GO_SIZE] + C[GO_SIZE]);
}
// closest points of two segments c1 + s u1 (|s| <= h1), c2 + t u2 (|t| <= h2), r = c1 - c2: d_capsule_capsule's rule
MOPA_HD void seg_seg_params(V3 u1, V3 u2, V3 r, double h1, double h2, double &sp, double &tp) {
    double b = dot3(u1, u2), c = dot3(u1, r), f = dot3(u2, r);
    double denom = fma(-b, b, 1.0);
    sp = 0.0;
    if (denom > 1e-12) sp = clampd(fma(b, f, -c) / denom, -h1, h1);
    tp = fma(b, sp, f);
    if (tp < -h2) { tp = -h2; sp = clampd(fma(b, tp, -c), -h1, h1); }
    else if (tp > h2) { tp = h2; sp = clampd(fma(b, tp, -c), -h1, h1); }
}
MOPA_HD double f_capsule_capsule(const double *A, const double *B, V3 &n, V3 &pos) {
    V3 a1 = col3(A + GO_MAT, 2), a2 = col3(B + GO_MAT, 2);
    V3 r = sub3(ld3(A + GO_POS), ld3(B + GO_POS));
    double sp, tp;
    seg_seg_params(a1, a2, r, A[GO_SIZE + 1], B[GO_SIZE + 1], sp, tp);
    V3 w = addscl3(r, a1, sp);
    w = addscl3(w, a2, -tp);
    const double len = norm3(w);
    n = unit_or_x(neg3(w), len);
    const V3 p1 = addscl3(ld3(A + GO_POS), a1, sp), p2 = addscl3(ld3(B + GO_POS), a2, tp);
    pos = mid3(addscl3(p1, n, A[GO_SIZE]), addscl3(p2, n, -B[GO_SIZE]));
    return len - (A[GO_SIZE] + B[GO_SIZE]);
}

// ---------------------------------------------------------------------------
// sphere - box / cylinder: outside, the clamp residual; centre inside, the face (barrel) of least depth, the first on ties
// ---------------------------------------------------------------------------
MOPA_HD double f_sphere_box(const double *S, const double *B, V3 &n, V3 &pos) {
    V3 sp = ld3(S + GO_POS);
    V3 v = sub3(sp, ld3(B + GO_POS));
    V3 l = matT_vec(B + GO_MAT, v);
    double hx = B[GO_SIZE], hy = B[GO_SIZE + 1], hz = B[GO_SIZE + 2];
    V3 q{clampd(l.x, -hx, hx), clampd(l.y, -hy, hy), clampd(l.z, -hz, hz)};
    V3 e{l.x - q.x, l.y - q.y, l.z - q.z};
    bool inside = (e.x == 0.0) && (e.y == 0.0) && (e.z == 0.0);
    if (inside) {
        const double dx = hx - fabs(l.x), dy = hy - fabs(l.y), dz = hz - fabs(l.z);
        double m = dmin(dmin(dx, dy), dz);
        int ax = 0;
        double mm = dx;
        if (dy < mm) { ax = 1; mm = dy; }
        if (dz < mm) { ax = 2; mm = dz; }
        const double sg = sgnp(comp3(l, ax));
        const double hax = ax == 0 ? hx : (ax == 1 ? hy : hz);
        n = scl3(col3(B + GO_MAT, ax), -sg);                      // minus the face's outward normal
        if (ax == 0) q.x = sg * hax; else if (ax == 1) q.y = sg * hax; else q.z = sg * hax;
        const V3 w2 = add3(mat_vec(B + GO_MAT, q), ld3(B + GO_POS));
        pos = mid3(addscl3(sp, n, S[GO_SIZE]), w2);
        return -m - S[GO_SIZE];
    }
    const double len = norm3(e);
    n = mat_vec(B + GO_MAT, unit_or_x(neg3(e), len));
    const V3 w2 = add3(mat_vec(B + GO_MAT, q), ld3(B + GO_POS));
    pos = mid3(addscl3(sp, n, S[GO_SIZE]), w2);
    return len - S[GO_SIZE];
}
MOPA_HD double f_sphere_cylinder(const double *S, const double *C, V3 &n, V3 &pos) {
    V3 a = col3(C + GO_MAT, 2);
    V3 sp = ld3(S + GO_POS);
    V3 v = sub3(sp, ld3(C + GO_POS));
    double z = dot3(v, a);
    V3 w = addscl3(v, a, -z);
    double rho = norm3(w);
    double dr = rho - C[GO_SIZE];
    double dz = fabs(z) - C[GO_SIZE + 1];
    // outward radial direction; on the axis: the cylinder's own x axis
    const V3 rad = (rho > 0.0) ? scl3(w, 1.0 / rho) : col3(C + GO_MAT, 0);
    const V3 capn = scl3(a, sgnp(z));
    double dp;
    V3 res;                 // from the cylinder's surface point to the sphere centre (outside), or depth * outward normal (inside)
    if (dr <= 0.0 && dz <= 0.0) {
        dp = dmax(dr, dz);
        if (dr > dz) { n = neg3(rad); res = scl3(rad, dr); }      // (dmax keeps dz on a tie: the cap)
        else { n = neg3(capn); res = scl3(capn, dz); }
    } else {
        double er = dmax(dr, 0.0), ez = dmax(dz, 0.0);
        dp = sqrt(fma(ez, ez, er * er));
        res = add3(scl3(rad, er), scl3(capn, ez));
        n = unit_or_x(neg3(res), dp);
    }
    pos = mid3(addscl3(sp, n, S[GO_SIZE]), sub3(sp, res));
    return dp - S[GO_SIZE];
}

// ---------------------------------------------------------------------------
// SAT classes.  An axis "wins" when it raises `best`: the first on ties.
// ---------------------------------------------------------------------------
// Everything in the box's frame (p0, d: the axis segment; h: half extents), rotated to the world at the end.
MOPA_HD double f_capsule_box(const double *C, const double *B, V3 &n, V3 &pos) {
    V3 h = ld3(B + GO_SIZE);
    V3 a = col3(C + GO_MAT, 2);
    V3 v = sub3(ld3(C + GO_POS), ld3(B + GO_POS));
    V3 cl = matT_vec(B + GO_MAT, v);
    V3 al = matT_vec(B + GO_MAT, a);
    double hh = C[GO_SIZE + 1];
    V3 p0 = addscl3(cl, al, -hh);
    V3 d{al.x * (2.0 * hh), al.y * (2.0 * hh), al.z * (2.0 * hh)};
    V3 e;
    double tstar;
    double g0 = segbox_half_fprime(p0, d, h, 0.0, e);
    if (g0 >= 0.0) tstar = 0.0;
    else {
        double g1 = segbox_half_fprime(p0, d, h, 1.0, e);
        if (g1 <= 0.0) tstar = 1.0;
        else {
            double tL = 0.0, gL = g0, tR = 1.0, gR = g1;
            segbox_knot(p0, d, h, h.x, p0.x, d.x, tL, gL, tR, gR);
            segbox_knot(p0, d, h, h.y, p0.y, d.y, tL, gL, tR, gR);
            segbox_knot(p0, d, h, h.z, p0.z, d.z, tL, gL, tR, gR);
            tstar = fma(tR - tL, (-gL) / (gR - gL), tL);
        }
    }
    segbox_half_fprime(p0, d, h, tstar, e);
    double dseg = norm3(e);
    V3 nl, w1l, w2l;
    double dist;
    if (dseg > 0.0) {
        // the residual e at t*: from the box's closest point to the axis point
        const V3 p{fma(d.x, tstar, p0.x), fma(d.y, tstar, p0.y), fma(d.z, tstar, p0.z)};
        nl = scl3(e, -1.0 / dseg);
        w1l = addscl3(p, nl, C[GO_SIZE]);
        w2l = V3{clampd(p.x, -h.x, h.x), clampd(p.y, -h.y, h.y), clampd(p.z, -h.z, h.z)};
        dist = dseg - C[GO_SIZE];
    } else {
        V3 m = addscl3(p0, d, 0.5);
        V3 hd{0.5 * d.x, 0.5 * d.y, 0.5 * d.z};
        double best = -kFar;
        int win = 0;
        double x;
        x = fabs(m.x) - (h.x + fabs(hd.x)); if (x > best) win = 0; best = dmax(best, x);
        x = fabs(m.y) - (h.y + fabs(hd.y)); if (x > best) win = 1; best = dmax(best, x);
        x = fabs(m.z) - (h.z + fabs(hd.z)); if (x > best) win = 2; best = dmax(best, x);
        const double mm[3] = {m.x, m.y, m.z}, aa[3] = {al.x, al.y, al.z}, hb[3] = {h.x, h.y, h.z};
        double wtl = 0.0, wsq = 1.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = (i + 1) % 3, k = (i + 2) % 3;
            double l2 = fma(aa[k], aa[k], aa[j] * aa[j]);
            if (l2 < 1e-12) continue;
            double tl = fma(mm[k], aa[j], -(mm[j] * aa[k]));
            double ra = fma(hb[k], fabs(aa[j]), hb[j] * fabs(aa[k]));
            const double sq = sqrt(l2);
            x = (fabs(tl) - ra) / sq;
            if (x > best) { win = 3 + i; wtl = tl; wsq = sq; }
            best = dmax(best, x);
        }
        dist = best - C[GO_SIZE];
        // sign: n . (c_box - c_capsule) >= 0, i.e. n . m <= 0 in the box's frame, zero counting as +
        if (win < 3) {
            // a face normal of the box: the segment's deepest feature centre along n, then the radius along n
            nl = axis3(win, comp3(m, win) <= 0.0 ? 1.0 : -1.0);
            const V3 ws = addscl3(m, al, signd(dot3(nl, al)) * hh);
            w1l = addscl3(ws, nl, C[GO_SIZE]);
            w2l = addscl3(ws, nl, best);
        } else {
            // e_i x axis: the segment against the box's supporting edge along e_i, each clamped to its extent
            const int i = win - 3, j = (i + 1) % 3, k = (i + 2) % 3;
            const double s = (wtl <= 0.0 ? 1.0 : -1.0) / wsq;
            double nn[3] = {0.0, 0.0, 0.0};
            nn[j] = -aa[k] * s;
            nn[k] = aa[j] * s;
            nl = V3{nn[0], nn[1], nn[2]};
            double ec[3] = {0.0, 0.0, 0.0};
            ec[j] = -signd(nn[j]) * hb[j];
            ec[k] = -signd(nn[k]) * hb[k];
            const V3 E{ec[0], ec[1], ec[2]}, ui = axis3(i, 1.0);
            double sp, tp;
            seg_seg_params(al, ui, sub3(m, E), hh, hb[i], sp, tp);
            w1l = addscl3(addscl3(m, al, sp), nl, C[GO_SIZE]);
            w2l = addscl3(E, ui, tp);
        }
    }
    n = mat_vec(B + GO_MAT, nl);
    pos = add3(mat_vec(B + GO_MAT, mid3(w1l, w2l)), ld3(B + GO_POS));
    return dist;
}

MOPA_HD double f_box_box(const double *A, const double *B, V3 &n, V3 &pos) {
    const double *Am = A + GO_MAT, *Bm = B + GO_MAT;
    double R[3][3], AR[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            R[i][j] = fma(Am[6 + i], Bm[6 + j], fma(Am[3 + i], Bm[3 + j], Am[i] * Bm[j]));
            AR[i][j] = fabs(R[i][j]);
        }
    V3 tv = matT_vec(Am, sub3(ld3(B + GO_POS), ld3(A + GO_POS)));
    const double t[3] = {tv.x, tv.y, tv.z};
    const double ha[3] = {A[GO_SIZE], A[GO_SIZE + 1], A[GO_SIZE + 2]}, hb[3] = {B[GO_SIZE], B[GO_SIZE + 1], B[GO_SIZE + 2]};
    double best = -kFar;
    int win = 0;
    double wsign = 1.0, wsq = 1.0;      // of the winning axis: sign of t along it (zero counts as +), length of the raw edge axis
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double rb = fma(hb[2], AR[i][2], fma(hb[1], AR[i][1], hb[0] * AR[i][0]));
        const double x = fabs(t[i]) - (ha[i] + rb);
        if (x > best) { win = i; wsign = sgnp(t[i]); }
        best = dmax(best, x);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        double tb = fma(t[2], R[2][j], fma(t[1], R[1][j], t[0] * R[0][j]));
        double ra = fma(ha[2], AR[2][j], fma(ha[1], AR[1][j], ha[0] * AR[0][j]));
        const double x = fabs(tb) - (ra + hb[j]);
        if (x > best) { win = 3 + j; wsign = sgnp(tb); }
        best = dmax(best, x);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            double l2 = fma(R[i2][j], R[i2][j], R[i1][j] * R[i1][j]);
            if (l2 < 1e-12) continue;
            double tl = fma(t[i2], R[i1][j], -(t[i1] * R[i2][j]));
            double ra = fma(ha[i2], AR[i1][j], ha[i1] * AR[i2][j]);
            double rb = fma(hb[j2], AR[i][j1], hb[j1] * AR[i][j2]);
            const double sq = sqrt(l2);
            const double x = (fabs(tl) - (ra + rb)) / sq;
            if (x > best) { win = 6 + 3 * i + j; wsign = sgnp(tl); wsq = sq; }
            best = dmax(best, x);
        }
    }
    const V3 cA = ld3(A + GO_POS), cB = ld3(B + GO_POS);
    if (win < 3) {
        // face axis of A: the deepest feature centre of B along -n, w1 = w2 - dist n
        n = scl3(col3(Am, win), wsign);
        V3 w2 = cB;
#pragma unroll
        for (int j = 0; j < 3; j++) w2 = addscl3(w2, col3(Bm, j), -(signd(wsign * R[win][j]) * hb[j]));
        pos = pos_from_w2(w2, n, best);
    } else if (win < 6) {
        // face axis of B: the mirror image
        const int jw = win - 3;
        n = scl3(col3(Bm, jw), wsign);
        V3 w1 = cA;
#pragma unroll
        for (int i = 0; i < 3; i++) w1 = addscl3(w1, col3(Am, i), signd(wsign * R[i][jw]) * ha[i]);
        pos = pos_from_w1(w1, n, best);
    } else {
        // edge i of A x edge j of B: the closest points of the two supporting edges, each clamped to its edge
        const int i = (win - 6) / 3, j = (win - 6) % 3;
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        const double s = wsign / wsq;
        double na[3] = {0.0, 0.0, 0.0};                 // n in A's frame: u_i x (column j of R), signed and normalised
        na[i1] = -R[i2][j] * s;
        na[i2] = R[i1][j] * s;
        n = mat_vec(Am, V3{na[0], na[1], na[2]});
        const double nb1 = fma(R[i2][j1], na[i2], R[i1][j1] * na[i1]);      // n in B's frame, components j1 / j2
        const double nb2 = fma(R[i2][j2], na[i2], R[i1][j2] * na[i1]);
        V3 pA = addscl3(cA, col3(Am, i1), signd(na[i1]) * ha[i1]);
        pA = addscl3(pA, col3(Am, i2), signd(na[i2]) * ha[i2]);
        V3 pB = addscl3(cB, col3(Bm, j1), -(signd(nb1) * hb[j1]));
        pB = addscl3(pB, col3(Bm, j2), -(signd(nb2) * hb[j2]));
        const V3 ua = col3(Am, i), ub = col3(Bm, j);
        double sp, tp;
        seg_seg_params(ua, ub, sub3(pA, pB), ha[i], hb[j], sp, tp);
        pos = mid3(addscl3(pA, ua, sp), addscl3(pB, ub, tp));
    }
    return best;
}

// ---------------------------------------------------------------------------
// [3P] libccd ccdMPRPenetration, complete: depth, direction and position.  mpr_penetration's walk with every portal vertex
// carrying the two support points it is the difference of (v0: the two centres); the operations on the differences, and so
// the depth, are mpr_penetration's.  A second walk, not a switch inside mpr_penetration: every validity and planner kernel
// inlines that one and keeps its register budget to the last VGPR.
// ---------------------------------------------------------------------------
struct MprV { V3 v, a, b; };
template <bool MESH>
MOPA_HD MprV support_md_w(const double *g1, int t1, const double *g2, int t2, V3 dir, const double *aux) {
    MprV r;
    r.a = support_geom<false>(g1, t1, dir);
    r.b = support_geom<MESH, 1>(g2, t2, neg3(dir), aux);
    r.v = sub3(r.a, r.b);
    return r;
}
MOPA_HD void expand_portal_w(const MprV &v0, MprV &v1, MprV &v2, MprV &v3, const MprV &v4) {
    V3 v4v0 = cross3(v4.v, v0.v);
    double dot = dot3(v1.v, v4v0);
    if (dot > 0.0) {
        dot = dot3(v2.v, v4v0);
        if (dot > 0.0) v1 = v4; else v3 = v4;
    } else {
        dot = dot3(v3.v, v4v0);
        if (dot > 0.0) v2 = v4; else v1 = v4;
    }
}
// origin_seg_dist2 / origin_tri_dist2 with the witness point they already form
MOPA_HD double origin_seg_wit(V3 x0, V3 b, V3 &wit) {
    V3 d = sub3(b, x0);
    V3 a = x0;
    double t = -1.0 * dot3(a, d);
    t = t / dot3(d, d);
    if (t < 0.0 || is_zero(t)) { wit = x0; return dot3(x0, x0); }
    if (t > 1.0 || ccd_eq(t, 1.0)) { wit = b; return dot3(b, b); }
    V3 w = addscl3(a, d, t);
    wit = w;
    return dot3(w, w);
}
MOPA_HD double origin_tri_wit(V3 x0, V3 B, V3 C, V3 &wit) {
    V3 d1 = sub3(B, x0), d2 = sub3(C, x0), a = x0;
    double v = dot3(d1, d1), w = dot3(d2, d2);
    double p = dot3(a, d1), q = dot3(a, d2), r = dot3(d1, d2);
    double s = fma(q, r, -(w * p)) / fma(w, v, -(r * r));
    double t = (fma(-s, r, -q)) / w;
    if ((is_zero(s) || s > 0.0) && (ccd_eq(s, 1.0) || s < 1.0) && (is_zero(t) || t > 0.0) &&
        (ccd_eq(t, 1.0) || t < 1.0) && (ccd_eq(t + s, 1.0) || t + s < 1.0)) {
        V3 wv = addscl3(a, d1, s);
        wv = addscl3(wv, d2, t);
        wit = wv;
        return dot3(wv, wv);
    }
    V3 w2;
    double dist = origin_seg_wit(x0, B, wit);
    double dd = origin_seg_wit(x0, C, w2);
    if (dd < dist) { dist = dd; wit = w2; }
    dd = origin_seg_wit(B, C, w2);
    if (dd < dist) { dist = dd; wit = w2; }
    return dist;
}
// [3P] libccd _ccdFindPos: the origin's barycentric weights in the tetrahedron v0 v1 v2 v3 (in the portal when that
// degenerates), applied to the two bodies' points; their mean
MOPA_HD V3 mpr_find_pos(const MprV &v0, const MprV &v1, const MprV &v2, const MprV &v3, V3 pdir) {
    double b0 = dot3(cross3(v1.v, v2.v), v3.v);
    double b1 = dot3(cross3(v3.v, v2.v), v0.v);
    double b2 = dot3(cross3(v0.v, v1.v), v3.v);
    double b3 = dot3(cross3(v2.v, v1.v), v0.v);
    double sum = ((b0 + b1) + b2) + b3;
    if (is_zero(sum) || sum < 0.0) {
        b0 = 0.0;
        b1 = dot3(cross3(v2.v, v3.v), pdir);
        b2 = dot3(cross3(v3.v, v1.v), pdir);
        b3 = dot3(cross3(v1.v, v2.v), pdir);
        sum = (b1 + b2) + b3;
    }
    const double inv = 1.0 / sum;
    V3 p1 = scl3(v0.a, b0), p2 = scl3(v0.b, b0);
    p1 = addscl3(p1, v1.a, b1); p2 = addscl3(p2, v1.b, b1);
    p1 = addscl3(p1, v2.a, b2); p2 = addscl3(p2, v2.b, b2);
    p1 = addscl3(p1, v3.a, b3); p2 = addscl3(p2, v3.b, b3);
    return scl3(add3(p1, p2), 0.5 * inv);
}
template <bool MESH = false>
MOPA_HD bool mpr_frame(const double *g1, int t1, const double *g2, int t2, double &depth, V3 &n, V3 &pos, const double *aux = nullptr) {
    MprV v0;
    v0.a = ld3(g1 + GO_POS);
    v0.b = ld3(g2 + GO_POS);
    v0.v = sub3(v0.a, v0.b);
    if (vec_eq0(v0.v)) v0.v.x += kCcdEps * 10.0;
    V3 dir = normalize3(neg3(v0.v));
    MprV v1 = support_md_w<MESH>(g1, t1, g2, t2, dir, aux);
    double dot = dot3(v1.v, dir);
    if (is_zero(dot) || dot < 0.0) return false;
    dir = cross3(v0.v, v1.v);
    if (is_zero(dot3(dir, dir))) {
        // touching, or the origin on the segment v0 v1: along v1, at the mean of v1's two points
        const double len = norm3(v1.v);
        depth = vec_eq0(v1.v) ? 0.0 : len;
        n = unit_or_x(v1.v, len);
        pos = mid3(v1.a, v1.b);
        return true;
    }
    dir = normalize3(dir);
    MprV v2 = support_md_w<MESH>(g1, t1, g2, t2, dir, aux);
    dot = dot3(v2.v, dir);
    if (is_zero(dot) || dot < 0.0) return false;
    dir = normalize3(cross3(sub3(v1.v, v0.v), sub3(v2.v, v0.v)));
    dot = dot3(dir, v0.v);
    if (dot > 0.0) {
        MprV tmp = v1; v1 = v2; v2 = tmp;
        dir = neg3(dir);
    }
    MprV v3, v4;
    int it = 0;
    for (;;) {
        if (++it > kMprPortalMaxIt) return false;
        v3 = support_md_w<MESH>(g1, t1, g2, t2, dir, aux);
        dot = dot3(v3.v, dir);
        if (is_zero(dot) || dot < 0.0) return false;
        bool cont = false;
        dot = dot3(cross3(v1.v, v3.v), v0.v);
        if (dot < 0.0 && !is_zero(dot)) { v2 = v3; cont = true; }
        if (!cont) {
            dot = dot3(cross3(v3.v, v2.v), v0.v);
            if (dot < 0.0 && !is_zero(dot)) { v1 = v3; cont = true; }
        }
        if (!cont) break;
        dir = normalize3(cross3(sub3(v1.v, v0.v), sub3(v2.v, v0.v)));
    }
    it = 0;
    for (;;) {
        if (++it > kMprPortalMaxIt) return false;
        dir = portal_dir(v1.v, v2.v, v3.v);
        dot = dot3(dir, v1.v);
        if (is_zero(dot) || dot > 0.0) break;
        v4 = support_md_w<MESH>(g1, t1, g2, t2, dir, aux);
        dot = dot3(v4.v, dir);
        if (!(is_zero(dot) || dot > 0.0) || portal_reach_tol(v1.v, v2.v, v3.v, v4.v, dir)) return false;
        expand_portal_w(v0, v1, v2, v3, v4);
    }
    int iterations = 0;
    for (;;) {
        dir = portal_dir(v1.v, v2.v, v3.v);
        v4 = support_md_w<MESH>(g1, t1, g2, t2, dir, aux);
        if (portal_reach_tol(v1.v, v2.v, v3.v, v4.v, dir) || iterations > kMprMaxIt) {
            V3 wit;
            depth = sqrt(origin_tri_wit(v1.v, v2.v, v3.v, wit));
            const double len = norm3(wit);
            n = (len > 0.0) ? scl3(wit, 1.0 / len) : dir;         // the portal's closest point to the origin; zero: the portal's direction
            pos = mpr_find_pos(v0, v1, v2, v3, dir);
            return true;
        }
        expand_portal_w(v0, v1, v2, v3, v4);
        iterations++;
    }
}
template <bool MESH = false>
MOPA_HD double f_convex(const double *A, int ta, const double *B, int tb, const double *aux, V3 &n, V3 &pos) {
    double depth;
    if (mpr_frame<MESH>(A, ta, B, tb, depth, n, pos, aux)) return -depth;
    return kFar;
}

// geom_dist with the frame: returns geom_dist's distance (same bits); n, pos are zero when it reports kFar.  (A, B) in the
// narrow phase's order, as geom_dist takes them.
template <bool MESH = false>
MOPA_HD double geom_frame(int code, const double *A, int ta, const double *B, int tb, const double *aux, V3 &n, V3 &pos) {
    double d = kFar;
    n = V3{0.0, 0.0, 0.0};
    pos = V3{0.0, 0.0, 0.0};
    switch (code) {
        case PC_PLANE_SPHERE: d = f_plane_sphere(A, B, n, pos); break;
        case PC_PLANE_CAPSULE: d = f_plane_capsule(A, B, n, pos); break;
        case PC_PLANE_CYLINDER: d = f_plane_cylinder(A, B, n, pos); break;
        case PC_PLANE_BOX: d = f_plane_box(A, B, n, pos); break;
        case PC_SPHERE_SPHERE: d = f_sphere_sphere(A, B, n, pos); break;
        case PC_SPHERE_CAPSULE: d = f_sphere_capsule(A, B, n, pos); break;
        case PC_SPHERE_CYLINDER: d = f_sphere_cylinder(A, B, n, pos); break;
        case PC_SPHERE_BOX: d = f_sphere_box(A, B, n, pos); break;
        case PC_CAPSULE_CAPSULE: d = f_capsule_capsule(A, B, n, pos); break;
        case PC_CAPSULE_BOX: d = f_capsule_box(A, B, n, pos); break;
        case PC_BOX_BOX: d = f_box_box(A, B, n, pos); break;
        case PC_CONVEX: {
            const double pre = (tb == G_BOX) ? d_capsule_box(A, B) : d_capsule_capsule(A, B);     // geom_dist's pre-tests
            if (pre > 1e-9) break;
            if (convex_axes_separate(A, ta, B, tb)) break;
            d = f_convex<false>(A, ta, B, tb, nullptr, n, pos);
            break;
        }
        case PC_PLANE_MESH: if (MESH) d = f_plane_mesh(A, B, aux, n, pos); break;
        case PC_CONVEX_MESH: if (MESH) d = f_convex<MESH>(A, ta, B, tb, aux, n, pos); break;
        default: break;
    }
    if (d == kFar) {
        n = V3{0.0, 0.0, 0.0};
        pos = V3{0.0, 0.0, 0.0};
    }
    return d;
}

// One posed pair given by its two types in ANY order: evaluated in pair_code's canonical order, the normal negated on the way
// out when that is the reverse (the normal always points from the first geom given towards the second).  out[7] = dist,
// normal[3], pos[3]; an unsupported type pair reports kFar.
template <bool MESH = false>
MOPA_HD void geom_frame_pair(int t1, const double *r1, int t2, const double *r2, const double *aux, double *out) {
    int code = pair_code(t1, t2);
    bool swapped = false;
    if (code < 0) { code = pair_code(t2, t1); swapped = true; }
    V3 n{0.0, 0.0, 0.0}, pos{0.0, 0.0, 0.0};
    double d = kFar;
    if (code >= 0) d = swapped ? geom_frame<MESH>(code, r2, t2, r1, t1, aux, n, pos) : geom_frame<MESH>(code, r1, t1, r2, t2, aux, n, pos);
    if (swapped && d != kFar) n = neg3(n);
    out[0] = d;
    out[1] = n.x; out[2] = n.y; out[3] = n.z;
    out[4] = pos.x; out[5] = pos.y; out[6] = pos.z;
}

}  // namespace mopa
