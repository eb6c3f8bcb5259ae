// mopa_manifold.hpp -- contact manifolds: for a posed pair, the frame's normal and UP TO 8 contact points where the flat pair
// classes touch along a face, an edge or a line (MuJoCo emits several contacts there: box-plane 4, capsule-plane 2, box-box up to 8).
//
// Numerics contract: mopa_device.hpp's (IEEE double, -ffp-contract=off, explicit fma only).  The host compile of these functions
// (mopa_geom_manifolds_host) is the sequential form the kernels must match bit for bit.
//
// Definition ("Contact manifolds"; [3P] restated from MuJoCo's documented behaviour, PARITY UNPINNED): ONE
// normal per pair, geom_frame's bits.  Every point i has two witnesses, w1_i on geom 1 and w2_i on geom 2, with
// w2_i - w1_i = dist_i * normal; pos_i is their midpoint.  A class rule below generates candidates in a fixed order; those with
// dist_i <= point_cutoff are kept, sorted by ascending dist_i (ties keep generation order), and the first P are written.  When
// the rule yields none, the manifold is the single frame point (geom_frame's pos / dist bits) if that lies under point_cutoff.
#pragma once
#include "mopa_frames.hpp"

namespace mopa {

constexpr int kManifoldMax = 8;                  // most points a manifold has (box-box: a quadrilateral clipped by four half planes)
constexpr double kSin120 = 0.8660254037844386;   // sqrt(3) / 2
constexpr double kManifoldFaceTol = 1e-14;       // an edge x edge axis this close to a face axis counts as that face axis

struct ManifoldPts {
    int n;
    double d[kManifoldMax];
    V3 p[kManifoldMax];
};
MOPA_HD void mf_push(ManifoldPts &c, V3 pos, double dist, double cut) {
    if (dist <= cut && c.n < kManifoldMax) {
        c.d[c.n] = dist;
        c.p[c.n] = pos;
        c.n++;
    }
}

// The capsule's surface point farthest along the unit direction g within the cross-section at the end e = c + sg hh a: on the cap,
// e + r g, when the cap faces g (g . (sg a) >= 0); else on the barrel's rim, e + r u with u = unit(g - (g . a) a) -- e + r g would
// lie INSIDE the capsule there.  false: the rim is degenerate (the axis is along g and the cap faces away).
MOPA_HD bool capsule_end_point(const double *C, double sg, V3 g, V3 &e, V3 &w) {
    const V3 a = col3(C + GO_MAT, 2);
    e = addscl3(ld3(C + GO_POS), a, sg * C[GO_SIZE + 1]);
    const double ga = dot3(g, a);
    if (sg * ga >= 0.0) {
        w = addscl3(e, g, C[GO_SIZE]);
        return true;
    }
    const V3 perp = addscl3(g, a, -ga);
    const double len = norm3(perp);
    if (!(len > 0.0)) return false;
    w = addscl3(e, perp, C[GO_SIZE] / len);
    return true;
}

// plane - capsule: the two ends e+- = c +- hh a, + first; w2 = the end's lowest surface point (e - r n where the cap faces the
// plane: dist = n . (e - p) - r as d_plane_capsule forms it)
MOPA_HD void mf_plane_capsule(const double *P, const double *C, V3 n, double cut, ManifoldPts &c) {
    const V3 pp = ld3(P + GO_POS), a = col3(C + GO_MAT, 2);
    const double na = dot3(n, a);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double sg = (k == 0) ? 1.0 : -1.0;
        V3 e, w2;
        if (!capsule_end_point(C, sg, neg3(n), e, w2)) continue;
        const double dist = (sg * na <= 0.0) ? dot3(sub3(e, pp), n) - C[GO_SIZE] : dot3(sub3(w2, pp), n);
        mf_push(c, pos_from_w2(w2, n, dist), dist, cut);
    }
}
// plane - box: the 8 vertices, index bit 0 / 1 / 2 = sign of x / y / z, - first; w2 = the vertex (the caller keeps the 4 deepest)
MOPA_HD void mf_plane_box(const double *P, const double *B, V3 n, double cut, ManifoldPts &c) {
    const V3 cb = ld3(B + GO_POS), pp = ld3(P + GO_POS);
    for (int k = 0; k < 8; k++) {
        V3 v = addscl3(cb, col3(B + GO_MAT, 0), (k & 1) ? B[GO_SIZE] : -B[GO_SIZE]);
        v = addscl3(v, col3(B + GO_MAT, 1), (k & 2) ? B[GO_SIZE + 1] : -B[GO_SIZE + 1]);
        v = addscl3(v, col3(B + GO_MAT, 2), (k & 4) ? B[GO_SIZE + 2] : -B[GO_SIZE + 2]);
        const double dist = dot3(sub3(v, pp), n);
        mf_push(c, pos_from_w2(v, n, dist), dist, cut);
    }
}
// plane - cylinder: (a) the deepest rim point -- the near cap (a zero n.a counts as +) on the radial side u that points into the
// plane, the cylinder's own x axis when the axis is along the normal; (b) the other cap's rim point on the same side; (c, d) the
// near cap's rim at +-120 degrees from (a) about the axis.  w2 = the rim point.
MOPA_HD void mf_plane_cylinder(const double *P, const double *C, V3 n, double cut, ManifoldPts &c) {
    const V3 a = col3(C + GO_MAT, 2), cc = ld3(C + GO_POS), pp = ld3(P + GO_POS);
    const double na = dot3(n, a);
    const V3 perp = addscl3(n, a, -na);
    const double len = norm3(perp);
    const V3 u = (len > 0.0) ? scl3(perp, -1.0 / len) : col3(C + GO_MAT, 0);
    const V3 w = cross3(a, u);
    const double r = C[GO_SIZE], sh = sgnp(na) * C[GO_SIZE + 1];
    const V3 near = addscl3(cc, a, -sh), far = addscl3(cc, a, sh);
    V3 q[4];
    q[0] = addscl3(near, u, r);
    q[1] = addscl3(far, u, r);
    q[2] = addscl3(addscl3(near, u, -0.5 * r), w, kSin120 * r);
    q[3] = addscl3(addscl3(near, u, -0.5 * r), w, -(kSin120 * r));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double dist = dot3(sub3(q[k], pp), n);
        mf_push(c, pos_from_w2(q[k], n, dist), dist, cut);
    }
}

// One Sutherland-Hodgman pass: keep sg * x[ax] <= h.  A crossing point gets the bound itself in the clipped coordinate.
MOPA_HD int mf_clip(const double (*in)[3], int nin, double (*out)[3], int ax, double sg, double h) {
    int no = 0;
    for (int i = 0; i < nin; i++) {
        const double *cur = in[i], *prev = in[(i + nin - 1) % nin];
        const double sc = sg * cur[ax], sp = sg * prev[ax];
        const bool cin = sc <= h, pin = sp <= h;
        if (cin != pin && no < kManifoldMax) {
            const double t = (h - sp) / (sc - sp);
            out[no][0] = fma(cur[0] - prev[0], t, prev[0]);
            out[no][1] = fma(cur[1] - prev[1], t, prev[1]);
            out[no][2] = fma(cur[2] - prev[2], t, prev[2]);
            out[no][ax] = sg * h;
            no++;
        }
        if (cin && no < kManifoldMax) {
            out[no][0] = cur[0]; out[no][1] = cur[1]; out[no][2] = cur[2];
            no++;
        }
    }
    return no;
}
// box - box, a face axis won.  X: the box with the reference face (its axis w, outward normal so * e_w in X's frame); Y: the other
// box, given in X's frame -- Cm[i][j] = (axis i of X) . (axis j of Y), ty = its centre.  Incident face: the face of Y along
// j* = argmax_j |Cm[w][j]| (the first on ties) whose outward normal opposes the reference face's; its vertices in the cyclic order
// (-,-) (+,-) (+,+) (-,+) over the axes (j*+1, j*+2), clipped against the reference face's side planes +i1, -i1, +i2, -i2.  Each
// vertex that is left is the witness on Y; dist = its height over the reference face; the witness on X = its foot on that face.
// vertex_is_w2: Y is the pair's second geom (a face axis of A won), else its first (the mirror image).
MOPA_HD void mf_box_face(const double *X, const double *Y, const double Cm[3][3], const double ty[3], int w, double so, V3 n, bool vertex_is_w2,
                         double cut, ManifoldPts &c) {
    const double hx[3] = {X[GO_SIZE], X[GO_SIZE + 1], X[GO_SIZE + 2]}, hy[3] = {Y[GO_SIZE], Y[GO_SIZE + 1], Y[GO_SIZE + 2]};
    int js = 0;
    double big = fabs(Cm[w][0]);
    if (fabs(Cm[w][1]) > big) { js = 1; big = fabs(Cm[w][1]); }
    if (fabs(Cm[w][2]) > big) { js = 2; big = fabs(Cm[w][2]); }
    const int j1 = (js + 1) % 3, j2 = (js + 2) % 3;
    const double sy = (so * Cm[w][js] > 0.0) ? -1.0 : 1.0;
    double pa[kManifoldMax][3], pb[kManifoldMax][3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double s1 = (k == 1 || k == 2) ? hy[j1] : -hy[j1], s2 = (k >= 2) ? hy[j2] : -hy[j2];
#pragma unroll
        for (int i = 0; i < 3; i++) pa[k][i] = fma(Cm[i][j2], s2, fma(Cm[i][j1], s1, fma(Cm[i][js], sy * hy[js], ty[i])));
    }
    const int i1 = (w + 1) % 3, i2 = (w + 2) % 3;
    int np = mf_clip(pa, 4, pb, i1, 1.0, hx[i1]);
    np = mf_clip(pb, np, pa, i1, -1.0, hx[i1]);
    np = mf_clip(pa, np, pb, i2, 1.0, hx[i2]);
    np = mf_clip(pb, np, pa, i2, -1.0, hx[i2]);
    for (int k = 0; k < np; k++) {
        const double dist = so * pa[k][w] - hx[w];
        const V3 v = add3(mat_vec(X + GO_MAT, V3{pa[k][0], pa[k][1], pa[k][2]}), ld3(X + GO_POS));
        mf_push(c, vertex_is_w2 ? pos_from_w2(v, n, dist) : pos_from_w1(v, n, dist), dist, cut);
    }
}
// f_box_box's SAT sweep again, expression for expression, for what that routine does not hand out: the axis that won (0..2 a face
// axis of A, 3..5 of B, 6..14 edge i of A x edge j of B; the first on ties) and the sign of t along it.  (A copy, not a new out
// parameter of f_box_box: the frames kernels keep their instructions.)
MOPA_HD void box_box_winner(const double *A, const double *B, int &win, double &wsign) {
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
    win = 0;
    wsign = 1.0;
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
            const double x = (fabs(tl) - (ra + rb)) / sqrt(l2);
            if (x > best) { win = 6 + 3 * i + j; wsign = sgnp(tl); }
            best = dmax(best, x);
        }
    }
}

MOPA_HD void mf_box_box(const double *A, const double *B, V3 n, double cut, ManifoldPts &c) {
    const double *Am = A + GO_MAT, *Bm = B + GO_MAT;
    int win;
    double wsign;
    box_box_winner(A, B, win, wsign);
    if (win >= 6) {
        // An edge pair that lies in a face gives that face's axis again (two boxes flat on each other, turned about the normal:
        // u_x(A) x u_x(B) is the common z), and rounding decides which of the tied axes won.  Such an axis counts as the face axis
        // it is parallel to (1 - |n . u| <= 1e-14; A's first); every other edge x edge contact is the frame's single point.
        const V3 la = matT_vec(Am, n), lb = matT_vec(Bm, n);
        const double ca[3] = {la.x, la.y, la.z}, cb[3] = {lb.x, lb.y, lb.z};
        int found = -1;
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (found < 0 && fabs(ca[i]) >= 1.0 - kManifoldFaceTol) { found = i; wsign = sgnp(ca[i]); }
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (found < 0 && fabs(cb[j]) >= 1.0 - kManifoldFaceTol) { found = 3 + j; wsign = sgnp(cb[j]); }
        if (found < 0) return;
        win = found;
    }
    double R[3][3];                              // f_box_box's
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = fma(Am[6 + i], Bm[6 + j], fma(Am[3 + i], Bm[3 + j], Am[i] * Bm[j]));
    const V3 tv = matT_vec(Am, sub3(ld3(B + GO_POS), ld3(A + GO_POS)));
    const double t[3] = {tv.x, tv.y, tv.z};
    if (win < 3) {
        mf_box_face(A, B, R, t, win, wsign, n, true, cut, c);
    } else {
        double Rt[3][3], tb[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            tb[j] = -fma(t[2], R[2][j], fma(t[1], R[1][j], t[0] * R[0][j]));
#pragma unroll
            for (int i = 0; i < 3; i++) Rt[j][i] = R[i][j];
        }
        mf_box_face(B, A, Rt, tb, win - 3, -wsign, n, false, cut, c);
    }
}

// capsule - box: k = the box axis with the largest |n . u_k| (the first on ties), F = the box face on that axis that faces the
// capsule.  Each end e+-: w1 = the end's surface point farthest along n (capsule_end_point: e + r n where the cap faces the box),
// dist = the way from w1 to F's plane along n, w2 = w1 + dist n -- a candidate only when w2 lies inside F's rectangle, bounds
// included.
MOPA_HD void mf_capsule_box(const double *C, const double *B, V3 n, double cut, ManifoldPts &c) {
    const V3 nl = matT_vec(B + GO_MAT, n);
    const double nn[3] = {nl.x, nl.y, nl.z}, hb[3] = {B[GO_SIZE], B[GO_SIZE + 1], B[GO_SIZE + 2]};
    int k = 0;
    double big = fabs(nn[0]);
    if (fabs(nn[1]) > big) { k = 1; big = fabs(nn[1]); }
    if (fabs(nn[2]) > big) { k = 2; big = fabs(nn[2]); }
    if (!(big > 0.0)) return;
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    const double face = (nn[k] > 0.0) ? -hb[k] : hb[k];          // F's coordinate along k: its outward normal opposes n
    const V3 cb = ld3(B + GO_POS);
#pragma unroll
    for (int e = 0; e < 2; e++) {
        V3 end, w1;
        if (!capsule_end_point(C, e == 0 ? 1.0 : -1.0, n, end, w1)) continue;
        const V3 wl = matT_vec(B + GO_MAT, sub3(w1, cb));
        const double l[3] = {wl.x, wl.y, wl.z};
        const double dist = (face - l[k]) / nn[k];
        const double x1 = fma(nn[k1], dist, l[k1]), x2 = fma(nn[k2], dist, l[k2]);
        if (fabs(x1) <= hb[k1] && fabs(x2) <= hb[k2]) mf_push(c, pos_from_w1(w1, n, dist), dist, cut);
    }
}

// geom_frame with the manifold: returns geom_frame's distance and writes its normal (same bits); npoint = the number of points
// under point_cutoff before the cap P (1..8); pdist [P] / ppos [P,3] hold the first P of them, deepest first, kFar / 0.0 in the
// slots behind.  (A, B) in the narrow phase's order.  A pair that reports kFar: npoint = 0, a zero normal.
template <bool MESH = false>
MOPA_HD double geom_manifold(int code, const double *A, int ta, const double *B, int tb, const double *aux, double point_cutoff, int P, V3 &n, int &npoint,
                             double *pdist, double *ppos) {
    V3 pos;
    const double d = geom_frame<MESH>(code, A, ta, B, tb, aux, n, pos);
    ManifoldPts c;
    c.n = 0;
    int most = kManifoldMax;
    if (d != kFar) {
        switch (code) {
            case PC_PLANE_CAPSULE: mf_plane_capsule(A, B, n, point_cutoff, c); break;
            case PC_PLANE_BOX: mf_plane_box(A, B, n, point_cutoff, c); most = 4; break;
            case PC_PLANE_CYLINDER: mf_plane_cylinder(A, B, n, point_cutoff, c); break;
            case PC_CAPSULE_BOX: mf_capsule_box(A, B, n, point_cutoff, c); break;
            case PC_BOX_BOX: mf_box_box(A, B, n, point_cutoff, c); break;
            default: break;
        }
    } else {
        n = V3{0.0, 0.0, 0.0};
    }
    // ascending dist, ties in generation order: a stable insertion sort
    for (int i = 1; i < c.n; i++) {
        const double di = c.d[i];
        const V3 pi = c.p[i];
        int j = i;
        while (j > 0 && c.d[j - 1] > di) {
            c.d[j] = c.d[j - 1];
            c.p[j] = c.p[j - 1];
            j--;
        }
        c.d[j] = di;
        c.p[j] = pi;
    }
    int np = c.n < most ? c.n : most;
    if (np == 0 && d != kFar && d <= point_cutoff) {     // the fallback, and every single-point class: the frame's point
        c.d[0] = d;
        c.p[0] = pos;
        np = 1;
    }
    npoint = np;
    for (int i = 0; i < P; i++) {
        const bool used = i < np;
        pdist[i] = used ? c.d[i] : kFar;
        ppos[3 * i] = used ? c.p[i].x : 0.0;
        ppos[3 * i + 1] = used ? c.p[i].y : 0.0;
        ppos[3 * i + 2] = used ? c.p[i].z : 0.0;
    }
    return d;
}

// One posed pair given by its two types in ANY order (geom_frame_pair's rule: evaluated in canonical order, the normal negated on
// the way out when that is the reverse, the points unchanged).  nd[4] = normal[3], dist; pts[P,4] = pos[3], dist_i.
template <bool MESH = false>
MOPA_HD void geom_manifold_pair(int t1, const double *r1, int t2, const double *r2, const double *aux, double point_cutoff, int P, double *nd, int *npoint,
                                double *pts) {
    int code = pair_code(t1, t2);
    bool swapped = false;
    if (code < 0) { code = pair_code(t2, t1); swapped = true; }
    V3 n{0.0, 0.0, 0.0};
    double d = kFar;
    int np = 0;
    double pd[kManifoldMax], pp[3 * kManifoldMax];
    for (int i = 0; i < P; i++) { pd[i] = kFar; pp[3 * i] = 0.0; pp[3 * i + 1] = 0.0; pp[3 * i + 2] = 0.0; }
    if (code >= 0)
        d = swapped ? geom_manifold<MESH>(code, r2, t2, r1, t1, aux, point_cutoff, P, n, np, pd, pp)
                    : geom_manifold<MESH>(code, r1, t1, r2, t2, aux, point_cutoff, P, n, np, pd, pp);
    if (swapped && d != kFar) n = neg3(n);
    nd[0] = n.x; nd[1] = n.y; nd[2] = n.z; nd[3] = d;
    *npoint = np;
    for (int i = 0; i < P; i++) {
        pts[4 * i] = pp[3 * i]; pts[4 * i + 1] = pp[3 * i + 1]; pts[4 * i + 2] = pp[3 * i + 2];
        pts[4 * i + 3] = pd[i];
    }
}

}  // namespace mopa
