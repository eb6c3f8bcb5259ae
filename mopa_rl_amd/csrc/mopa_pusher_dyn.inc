// mopa_pusher_dyn.inc -- K8: PusherObstacle-v0 dynamics (env/pusher/pusher_obstacle.py `_step`, env/base.py `_get_control`,
// env/assets/xml/common/pusher_gripper.xml).  Included by mopa_envdyn.hip; C ABI in include/mopa_hip.h "mopa_env_*pusher*".
//
// One env.step = the env's PID loop over nsub (100) sub-steps of MuJoCo 2.0's RK4 (mj_RungeKutta: four forward passes per
// sub-step), then K4 kind 3's reward / obs / bookkeeping (env_step_lane<3>, with the carried velocities in the obs).
// Simulated dofs: joint0..3 (planar hinges about z) and box_x / box_y (slides); everything moves in one horizontal plane,
// so kinematics, mass matrix and bias forces are written in 2-D (dynamics.py:pusher_dyn_facts has the planar tree).
// A forward pass: kinematics -> M, bias -> unconstrained qacc -> contacts (restated planar pair geometry, below) and joint
// limits as soft-constraint rows (solref / solimp impedance, pyramidal cones, condim 3) -> primal Newton solve with an exact
// line search (K7's solver 1 restated for one lane) -> qacc.
//
// Mapping: one LANE per env, 64 envs per wave.  A sub-step is a serial chain (PID -> 4 x (forward pass) -> RK4 sum), the
// Newton problem has 6 unknowns, and most pairs are culled by a bounding-circle test; spreading the ~72 pairs of an env over
// lanes (K7) would put cross-lane sums into every Newton iteration of a 6 x 6 problem.  DESIGN.md section 4 K8 has the
// measurement.  The contact records live in a per-lane private array (scratch): an env has at most kPdMaxCon contacts.
//
// Numerics: no fma(); -ffp-contract=off; trig through mopa_sincos.  tests/pusher_dyn_ref.py performs the same operations in the
// same order, so qpos / qvel / i_term are compared bit for bit.

constexpr int kPdNv = 6, kPdArm = 4, kPdMaxCon = 16, kPdLsEvals = 50, kPdPairRec = 20;
constexpr double kPdMinVal = 1e-15;      // MuJoCo's mjMINVAL: floor of a row's regulariser R

struct PdHdr {
    int npair, maxcon, iterations, nsub, contacts;
    int qadr[kPdNv], limited[kPdNv];
    double lo[kPdNv], hi[kPdNv];
    double base_x, base_y;                                       // anchor of joint0 in the world
    double rel_x[kPdArm], rel_y[kPdArm];                         // anchor of arm body k in the frame of body k - 1 (k = 0: unused)
    double mass[kPdArm], com_x[kPdArm], com_y[kPdArm], izz[kPdArm];   // lumped arm bodies (fingertip welded to body3)
    double box_mass, box_org_x, box_org_y, box_ref_x, box_ref_y;
    double armature[kPdNv], damping[kPdNv];
    double gear[kPdArm], kv[kPdArm], ctrl_lo[kPdArm], ctrl_hi[kPdArm];
    double kp, kd, ki, alpha, frame_dt, h, tol, inv_scale;
    double lim_par[8];                                           // -, margin, K, B, d0, dmax, width, -
};

// pose of a body in the plane: origin and rotation (c, s)
struct PdPose { double x, y, c, s; };

__device__ __forceinline__ void pd_xform(const PdPose &p, double lx, double ly, double &wx, double &wy) {
    wx = p.x + (p.c * lx - p.s * ly);
    wy = p.y + (p.s * lx + p.c * ly);
}

// soft-constraint impedance (MuJoCo's solimp sigmoid with midpoint 0.5, power 2) -- the same curve as ct_impedance, fma-free
__device__ __forceinline__ double pd_impedance(const double *par, double dist) {
    const double x = fabs(dist - par[1]) / par[6];
    double y;
    if (x >= 1.0) y = 1.0;
    else if (x <= 0.5) y = 2.0 * (x * x);
    else y = 1.0 - 2.0 * ((1.0 - x) * (1.0 - x));
    return par[4] + y * (par[5] - par[4]);
}

// packed lower-triangular L D L^T of a 6 x 6 matrix in place (D on the diagonal), then solve for x
__device__ __forceinline__ void pd_ldl(double *A) {
#pragma unroll
    for (int i = 0; i < kPdNv; i++) {
#pragma unroll
        for (int k = 0; k <= i; k++) {
            double acc = A[i * (i + 1) / 2 + k];
#pragma unroll
            for (int j = 0; j < k; j++) acc = acc - A[i * (i + 1) / 2 + j] * (A[k * (k + 1) / 2 + j] * A[j * (j + 1) / 2 + j]);
            if (k < i) A[i * (i + 1) / 2 + k] = acc / A[k * (k + 1) / 2 + k];
            else A[i * (i + 1) / 2 + i] = acc;
        }
    }
}
__device__ __forceinline__ void pd_ldl_solve(const double *A, double *x) {
#pragma unroll
    for (int i = 0; i < kPdNv; i++) {
        double acc = x[i];
#pragma unroll
        for (int j = 0; j < i; j++) acc = acc - A[i * (i + 1) / 2 + j] * x[j];
        x[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < kPdNv; i++) x[i] = x[i] / A[i * (i + 1) / 2 + i];
#pragma unroll
    for (int i = kPdNv - 1; i >= 0; i--) {
        double acc = x[i];
#pragma unroll
        for (int j = i + 1; j < kPdNv; j++) acc = acc - A[j * (j + 1) / 2 + i] * x[j];
        x[i] = acc;
    }
}

// the contacts of one forward pass
struct PdCon {
    int n, dropped;
    double Jn[kPdMaxCon][kPdNv], Jt[kPdMaxCon][kPdNv];
    double dist[kPdMaxCon];
    int pair[kPdMaxCon];
    double mu[kPdMaxCon], D[kPdMaxCon][4], aref[kPdMaxCon][4];      // the rows' friction, weight and reference acceleration (kept for the readout)
};

// kinematics of the planar tree: poses of the arm bodies (0..3) and of the box (4)
__device__ __forceinline__ void pd_kinematics(const PdHdr &ph, const double *q, PdPose *P) {
    double px = ph.base_x, py = ph.base_y, pc = 1.0, ps = 0.0, th = 0.0;
#pragma unroll
    for (int k = 0; k < kPdArm; k++) {
        double ox = px, oy = py;
        if (k > 0) pd_xform(PdPose{px, py, pc, ps}, ph.rel_x[k], ph.rel_y[k], ox, oy);
        th = th + q[k];
        double s, c;
        mopa_sincos(th, s, c);
        P[k] = PdPose{ox, oy, c, s};
        px = ox; py = oy; pc = c; ps = s;
    }
    P[4] = PdPose{ph.box_org_x + (q[4] - ph.box_ref_x), ph.box_org_y + (q[5] - ph.box_ref_y), 1.0, 0.0};
}

// d . (velocity of world point (x, y) on body b) per unit dof velocity, accumulated into J with sign sg
__device__ __forceinline__ void pd_point_jac(const PdPose *P, int b, double x, double y, double nx, double ny, double sg, double *J) {
    if (b < 0) return;
    if (b == 4) {
        J[4] = J[4] + sg * nx;
        J[5] = J[5] + sg * ny;
        return;
    }
#pragma unroll
    for (int j = 0; j < kPdArm; j++)
        if (j <= b) {
            const double rx = x - P[j].x, ry = y - P[j].y;
            J[j] = J[j] + sg * (rx * ny - ry * nx);
        }
}

__device__ __forceinline__ void pd_emit(PdCon &C, int maxcon, const PdPose *P, int ba, int bb, int pair, double px, double py, double nx, double ny,
                                        double dist) {
    if (C.n >= maxcon) { C.dropped++; return; }
    const int c = C.n++;
    double Jn[kPdNv] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Jt[kPdNv] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double tx = -ny, ty = nx;
    pd_point_jac(P, ba, px, py, nx, ny, 1.0, Jn);
    pd_point_jac(P, bb, px, py, nx, ny, -1.0, Jn);
    pd_point_jac(P, ba, px, py, tx, ty, 1.0, Jt);
    pd_point_jac(P, bb, px, py, tx, ty, -1.0, Jt);
#pragma unroll
    for (int i = 0; i < kPdNv; i++) { C.Jn[c][i] = Jn[i]; C.Jt[c][i] = Jt[i]; }
    C.dist[c] = dist;
    C.pair[c] = pair;
}

// closest point of segment (ax, ay) -> (bx, by) to (x, y): parameter t in [0, 1]
__device__ __forceinline__ double pd_seg_t(double ax, double ay, double bx, double by, double x, double y) {
    const double dx = bx - ax, dy = by - ay;
    const double L2 = dx * dx + dy * dy;
    double t = L2 > 0.0 ? ((x - ax) * dx + (y - ay) * dy) / L2 : 0.0;
    return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
}

// collision: every pair of the compiled list (dynamics.py:pusher_dyn_facts), restated planar geometry.
//   class 0 capsule (A) - box (B): candidates = the two segment ends against the rectangle, and each rectangle corner against
//           the segment interior; the two deepest penetrating candidates are kept (two points when the capsule lies along a face)
//   class 1 capsule - capsule: closest points of the two segments (ends against the other segment): one point
//   class 2 box (A) - box (B): axis-aligned rectangles; penetration along the axis of least overlap, the four corners of
//           the overlap rectangle as points
// Normals point from B to A; dist < margin (0 in this scene) makes a contact; the point sits midway between the surfaces.
__device__ __forceinline__ void pd_collide(const PdHdr &ph, const double *__restrict__ PR, const PdPose *P, PdCon &C) {
    C.n = 0;
#pragma unroll 1
    for (int p = 0; p < ph.npair; p++) {
        const double *r = PR + (size_t)kPdPairRec * p;
        const int cls = (int)r[0], ba = (int)r[1], bb = (int)r[2];
        const double *ga = r + 3, *gb = r + 8;
        const double margin = r[14];
        const PdPose pa = ba >= 0 ? P[ba] : PdPose{0.0, 0.0, 1.0, 0.0};
        const PdPose pb = bb >= 0 ? P[bb] : PdPose{0.0, 0.0, 1.0, 0.0};
        if (cls == 2) {
            double ax, ay, bx, by;
            pd_xform(pa, ga[0], ga[1], ax, ay);
            pd_xform(pb, gb[0], gb[1], bx, by);
            const double ux = ax - bx, uy = ay - by;
            const double ox = (ga[2] + gb[2]) - fabs(ux), oy = (ga[3] + gb[3]) - fabs(uy);
            const double dist = -(ox < oy ? ox : oy);
            if (!(ox > 0.0 && oy > 0.0) || !(dist < margin)) continue;
            double nx = 0.0, ny = 0.0;
            if (ox <= oy) nx = ux >= 0.0 ? 1.0 : -1.0; else ny = uy >= 0.0 ? 1.0 : -1.0;
            const double x0 = dmax(ax - ga[2], bx - gb[2]), x1 = dmin(ax + ga[2], bx + gb[2]);
            const double y0 = dmax(ay - ga[3], by - gb[3]), y1 = dmin(ay + ga[3], by + gb[3]);
            pd_emit(C, ph.maxcon, P, ba, bb, p, x0, y0, nx, ny, dist);
            pd_emit(C, ph.maxcon, P, ba, bb, p, x1, y0, nx, ny, dist);
            pd_emit(C, ph.maxcon, P, ba, bb, p, x0, y1, nx, ny, dist);
            pd_emit(C, ph.maxcon, P, ba, bb, p, x1, y1, nx, ny, dist);
            continue;
        }
        double a0x, a0y, a1x, a1y;
        pd_xform(pa, ga[0], ga[1], a0x, a0y);
        pd_xform(pa, ga[2], ga[3], a1x, a1y);
        const double ra = ga[4];
        // bounding circles
        const double cax = 0.5 * (a0x + a1x), cay = 0.5 * (a0y + a1y);
        const double dax = a1x - a0x, day = a1y - a0y;
        const double rba = 0.5 * sqrt(dax * dax + day * day) + ra;
        if (cls == 1) {
            double b0x, b0y, b1x, b1y;
            pd_xform(pb, gb[0], gb[1], b0x, b0y);
            pd_xform(pb, gb[2], gb[3], b1x, b1y);
            const double rb = gb[4];
            const double cbx = 0.5 * (b0x + b1x), cby = 0.5 * (b0y + b1y);
            const double dbx = b1x - b0x, dby = b1y - b0y;
            const double rbb = 0.5 * sqrt(dbx * dbx + dby * dby) + rb;
            const double ccx = cax - cbx, ccy = cay - cby, rr = (rba + rbb) + margin;
            if (ccx * ccx + ccy * ccy > rr * rr) continue;
            // the four end-to-segment candidates: (X on A, Y on B)
            double best = 0.0, Xx = 0.0, Xy = 0.0, Yx = 0.0, Yy = 0.0;
            bool have = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                double xx, xy, yx, yy;
                if (k < 2) {
                    xx = k == 0 ? a0x : a1x; xy = k == 0 ? a0y : a1y;
                    const double t = pd_seg_t(b0x, b0y, b1x, b1y, xx, xy);
                    yx = b0x + t * dbx; yy = b0y + t * dby;
                } else {
                    yx = k == 2 ? b0x : b1x; yy = k == 2 ? b0y : b1y;
                    const double t = pd_seg_t(a0x, a0y, a1x, a1y, yx, yy);
                    xx = a0x + t * dax; xy = a0y + t * day;
                }
                const double wx = xx - yx, wy = xy - yy;
                const double d2 = wx * wx + wy * wy;
                if (!have || d2 < best) { have = true; best = d2; Xx = xx; Xy = xy; Yx = yx; Yy = yy; }
            }
            const double d = sqrt(best);
            const double dist = (d - ra) - rb;
            if (!(dist < margin) || !(d > 0.0)) continue;
            const double nx = (Xx - Yx) / d, ny = (Xy - Yy) / d;
            const double off = ra + 0.5 * dist;
            pd_emit(C, ph.maxcon, P, ba, bb, p, Xx - nx * off, Xy - ny * off, nx, ny, dist);
            continue;
        }
        // class 0: capsule A against box B
        double bx, by;
        pd_xform(pb, gb[0], gb[1], bx, by);
        const double hx = gb[2], hy = gb[3];
        {
            const double ccx = cax - bx, ccy = cay - by, rr = (rba + sqrt(hx * hx + hy * hy)) + margin;
            if (ccx * ccx + ccy * ccy > rr * rr) continue;
        }
        // candidates 0, 1: segment ends; 2..5: rectangle corners against the segment interior
        double cd[6], cpx[6], cpy[6], cnx[6], cny[6];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const double ex = k == 0 ? a0x : a1x, ey = k == 0 ? a0y : a1y;
            const double ux = ex - bx, uy = ey - by;
            const double qx = dmin(dmax(ux, -hx), hx), qy = dmin(dmax(uy, -hy), hy);
            const double wx = ux - qx, wy = uy - qy;
            const double d = sqrt(wx * wx + wy * wy);
            double nx, ny, dd;
            if (d > 0.0) {
                nx = wx / d; ny = wy / d; dd = d;
            } else {            // the end inside the rectangle: out through the nearest face
                const double fx = hx - fabs(ux), fy = hy - fabs(uy);
                if (fx <= fy) { nx = ux >= 0.0 ? 1.0 : -1.0; ny = 0.0; dd = -fx; }
                else { nx = 0.0; ny = uy >= 0.0 ? 1.0 : -1.0; dd = -fy; }
            }
            const double dist = dd - ra;
            const double off = ra + 0.5 * dist;
            cd[k] = dist; cpx[k] = ex - nx * off; cpy[k] = ey - ny * off; cnx[k] = nx; cny[k] = ny;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double kx = bx + ((k & 1) ? hx : -hx), ky = by + ((k & 2) ? hy : -hy);
            const double dx = a1x - a0x, dy = a1y - a0y;
            const double L2 = dx * dx + dy * dy;
            const double t = L2 > 0.0 ? ((kx - a0x) * dx + (ky - a0y) * dy) / L2 : 0.0;
            cd[2 + k] = 1.0; cpx[2 + k] = 0.0; cpy[2 + k] = 0.0; cnx[2 + k] = 0.0; cny[2 + k] = 0.0;
            if (t > 0.0 && t < 1.0) {
                const double sx = a0x + t * dx, sy = a0y + t * dy;
                const double wx = sx - kx, wy = sy - ky;
                const double d = sqrt(wx * wx + wy * wy);
                if (d > 0.0) {
                    const double nx = wx / d, ny = wy / d;
                    const double dist = d - ra;
                    const double off = ra + 0.5 * dist;
                    cd[2 + k] = dist; cpx[2 + k] = sx - nx * off; cpy[2 + k] = sy - ny * off; cnx[2 + k] = nx; cny[2 + k] = ny;
                }
            }
        }
        int i0 = -1, i1 = -1;
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (cd[k] < margin) {
                if (i0 < 0 || cd[k] < cd[i0]) { i1 = i0; i0 = k; }
                else if (i1 < 0 || cd[k] < cd[i1]) i1 = k;
            }
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (k == i0) pd_emit(C, ph.maxcon, P, ba, bb, p, cpx[k], cpy[k], cnx[k], cny[k], cd[k]);
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (k == i1) pd_emit(C, ph.maxcon, P, ba, bb, p, cpx[k], cpy[k], cnx[k], cny[k], cd[k]);
    }
}

// One forward pass at (q, v) with control ctrl: qacc.  C (contacts) is scratch; dropped contacts are counted into *drop.
__device__ __forceinline__ void pd_forward(const PdHdr &ph, const double *__restrict__ PR, const double *q, const double *v, const double *ctrl,
                                           double *qacc, PdCon &C, int &drop) {
    PdPose P[5];
    pd_kinematics(ph, q, P);
    // ---- mass matrix (packed lower triangle) and bias forces of the planar chain; the box block is diagonal
    double cx[kPdArm], cy[kPdArm];
#pragma unroll
    for (int b = 0; b < kPdArm; b++) pd_xform(P[b], ph.com_x[b], ph.com_y[b], cx[b], cy[b]);
    double M[21];
#pragma unroll
    for (int i = 0; i < 21; i++) M[i] = 0.0;
#pragma unroll
    for (int j = 0; j < kPdArm; j++)
#pragma unroll
        for (int k = 0; k <= j; k++) {
            double acc = 0.0;
#pragma unroll
            for (int b = 0; b < kPdArm; b++)
                if (b >= j) {
                    const double rjx = cx[b] - P[j].x, rjy = cy[b] - P[j].y, rkx = cx[b] - P[k].x, rky = cy[b] - P[k].y;
                    acc = acc + (ph.mass[b] * (rjx * rkx + rjy * rky) + ph.izz[b]);
                }
            M[j * (j + 1) / 2 + k] = j == k ? acc + ph.armature[j] : acc;
        }
    M[14] = ph.box_mass + ph.armature[4];
    M[20] = ph.box_mass + ph.armature[5];
    // accelerations at qacc = 0: anchors, then centres of mass (every link turns at its absolute rate W)
    double W[kPdArm], aax[kPdArm], aay[kPdArm];
    double w = 0.0, ax_ = 0.0, ay_ = 0.0;
#pragma unroll
    for (int k = 0; k < kPdArm; k++) {
        if (k > 0) {
            const double w2 = W[k - 1] * W[k - 1];
            ax_ = ax_ - w2 * (P[k].x - P[k - 1].x);
            ay_ = ay_ - w2 * (P[k].y - P[k - 1].y);
        }
        w = w + v[k];
        W[k] = w; aax[k] = ax_; aay[k] = ay_;
    }
    double f[kPdNv];
#pragma unroll
    for (int j = 0; j < kPdArm; j++) {
        double bias = 0.0;
#pragma unroll
        for (int b = 0; b < kPdArm; b++)
            if (b >= j) {
                const double w2 = W[b] * W[b];
                const double acx = aax[b] - w2 * (cx[b] - P[b].x), acy = aay[b] - w2 * (cy[b] - P[b].y);
                const double rx = cx[b] - P[j].x, ry = cy[b] - P[j].y;
                bias = bias + ph.mass[b] * (rx * acy - ry * acx);
            }
        // velocity actuator (ctrllimited): gear * (kv ctrl - kv gear qdot); passive: -damping qdot
        const double cc = clampd(ctrl[j], ph.ctrl_lo[j], ph.ctrl_hi[j]);
        const double act = ph.gear[j] * (ph.kv[j] * cc - ph.kv[j] * ph.gear[j] * v[j]);
        f[j] = (-(ph.damping[j] * v[j]) - bias) + act;
    }
    f[4] = -(ph.damping[4] * v[4]);
    f[5] = -(ph.damping[5] * v[5]);
    double L[21];
#pragma unroll
    for (int i = 0; i < 21; i++) L[i] = M[i];
    pd_ldl(L);
    double a0[kPdNv];
#pragma unroll
    for (int i = 0; i < kPdNv; i++) a0[i] = f[i];
    pd_ldl_solve(L, a0);
    // ---- constraints: contacts (4 pyramid edges each) and joint limits
    C.n = 0;
    C.dropped = 0;
    if (ph.contacts) pd_collide(ph, PR, P, C);
    drop += C.dropped;
    double lside[kPdNv], laref[kPdNv], lD[kPdNv];
    bool any = C.n > 0;
#pragma unroll
    for (int l = 0; l < kPdNv; l++) {
        lside[l] = 0.0; laref[l] = 0.0; lD[l] = 0.0;
        if (!ph.limited[l]) continue;
        const double dlo = q[l] - ph.lo[l], dhi = ph.hi[l] - q[l];
        double dist = 0.0;
        if (dlo < 0.0) { lside[l] = 1.0; dist = dlo; } else if (dhi < 0.0) { lside[l] = -1.0; dist = dhi; }
        if (lside[l] != 0.0) {
            any = true;
            double e[kPdNv] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            e[l] = 1.0;
            pd_ldl_solve(L, e);
            const double imp = pd_impedance(ph.lim_par, dist);
            double Ri = ((1.0 - imp) / imp) * e[l];
            if (Ri < kPdMinVal) Ri = kPdMinVal;
            laref[l] = -(ph.lim_par[3] * (lside[l] * v[l])) - (ph.lim_par[2] * imp) * (dist - ph.lim_par[1]);
            lD[l] = 1.0 / Ri;
        }
    }
#pragma unroll
    for (int i = 0; i < kPdNv; i++) qacc[i] = a0[i];
    if (!any) return;
    // rows of the contacts: edge i = Jn + s mu Jt (i = 0, 1: s = +1, -1 along the in-plane tangent), Jn (i = 2, 3: the tangent
    // along z moves no dof); weight D = 1 / R, R = (1 - imp) / imp * A_ii with A_ii = J_i M^-1 J_i^T; reference acceleration
    // aref = -B J_i v - K imp (dist - margin)
#pragma unroll 1
    for (int c = 0; c < C.n; c++) {
        const double *par = PR + (size_t)kPdPairRec * C.pair[c] + 13;
        double bn[kPdNv], bt[kPdNv];
#pragma unroll
        for (int i = 0; i < kPdNv; i++) { bn[i] = C.Jn[c][i]; bt[i] = C.Jt[c][i]; }
        pd_ldl_solve(L, bn);
        pd_ldl_solve(L, bt);
        double G0 = 0.0, G1 = 0.0, G3 = 0.0, jvn = 0.0, jvt = 0.0;
#pragma unroll
        for (int i = 0; i < kPdNv; i++) {
            G0 = G0 + C.Jn[c][i] * bn[i];
            G1 = G1 + C.Jn[c][i] * bt[i];
            G3 = G3 + C.Jt[c][i] * bt[i];
            jvn = jvn + C.Jn[c][i] * v[i];
            jvt = jvt + C.Jt[c][i] * v[i];
        }
        const double mu = par[0];
        const double imp = pd_impedance(par, C.dist[c]);
        const double kpos = (par[2] * imp) * (C.dist[c] - par[1]);
        C.mu[c] = mu;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double sm = i == 0 ? mu : (i == 1 ? -mu : 0.0);
            const double Aii = (G0 + (2.0 * sm) * G1) + (sm * sm) * G3;
            double Ri = ((1.0 - imp) / imp) * Aii;
            if (Ri < kPdMinVal) Ri = kPdMinVal;
            const double jv = jvn + sm * jvt;
            C.D[c][i] = 1.0 / Ri;
            C.aref[c][i] = -(par[3] * jv) - kpos;
        }
    }
    // ---- primal Newton: minimise 1/2 (a - a0)' M (a - a0) + sum_rows 1/2 D min(0, J a - aref)^2
#pragma unroll 1
    for (int it = 0; it < ph.iterations; it++) {
        double dq[kPdNv], Mg[kPdNv], g[kPdNv], H[21];
#pragma unroll
        for (int i = 0; i < kPdNv; i++) dq[i] = qacc[i] - a0[i];
#pragma unroll
        for (int i = 0; i < kPdNv; i++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < kPdNv; k++) acc = acc + M[i >= k ? i * (i + 1) / 2 + k : k * (k + 1) / 2 + i] * dq[k];
            Mg[i] = acc;
        }
        double gauss = 0.0;
#pragma unroll
        for (int i = 0; i < kPdNv; i++) gauss = gauss + dq[i] * Mg[i];
        gauss = 0.5 * gauss;
        double p0 = gauss;
#pragma unroll
        for (int i = 0; i < kPdNv; i++) g[i] = Mg[i];
#pragma unroll
        for (int i = 0; i < 21; i++) H[i] = M[i];
#pragma unroll 1
        for (int c = 0; c < C.n; c++) {
            double un = 0.0, ut = 0.0;
#pragma unroll
            for (int i = 0; i < kPdNv; i++) { un = un + C.Jn[c][i] * qacc[i]; ut = ut + C.Jt[c][i] * qacc[i]; }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double sm = r == 0 ? C.mu[c] : (r == 1 ? -C.mu[c] : 0.0);
                const double x = (un + sm * ut) - C.aref[c][r];
                if (!(x < 0.0)) continue;
                const double D = C.D[c][r];
                p0 = p0 + (0.5 * D * x) * x;
                double J[kPdNv];
#pragma unroll
                for (int i = 0; i < kPdNv; i++) J[i] = C.Jn[c][i] + sm * C.Jt[c][i];
#pragma unroll
                for (int i = 0; i < kPdNv; i++) {
                    g[i] = g[i] + (D * x) * J[i];
#pragma unroll
                    for (int k = 0; k <= i; k++) H[i * (i + 1) / 2 + k] = H[i * (i + 1) / 2 + k] + (D * J[i]) * J[k];
                }
            }
        }
#pragma unroll
        for (int l = 0; l < kPdNv; l++)
            if (lD[l] > 0.0) {
                const double x = lside[l] * qacc[l] - laref[l];
                if (x < 0.0) {
                    p0 = p0 + (0.5 * lD[l] * x) * x;
                    g[l] = g[l] + (lD[l] * x) * lside[l];
                    H[l * (l + 1) / 2 + l] = H[l * (l + 1) / 2 + l] + lD[l];
                }
            }
        pd_ldl(H);
        double dir[kPdNv];
#pragma unroll
        for (int i = 0; i < kPdNv; i++) dir[i] = -g[i];
        pd_ldl_solve(H, dir);
        // exact line search on the piecewise-quadratic cost along dir: safeguarded Newton on p'(alpha), first trial the full step
        double Md[kPdNv];
#pragma unroll
        for (int i = 0; i < kPdNv; i++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < kPdNv; k++) acc = acc + M[i >= k ? i * (i + 1) / 2 + k : k * (k + 1) / 2 + i] * dir[k];
            Md[i] = acc;
        }
        double qa = 0.0, qb = 0.0, slope0 = 0.0;
#pragma unroll
        for (int i = 0; i < kPdNv; i++) { qa = qa + dir[i] * Md[i]; qb = qb + dir[i] * Mg[i]; slope0 = slope0 + dir[i] * g[i]; }
        double alpha = 1.0, lo = 0.0, hi = -1.0, pa = p0;
        bool exact = false;
#pragma unroll 1
        for (int e = 0; e < kPdLsEvals; e++) {
            double d1 = alpha * qa + qb, d2 = qa;
            pa = gauss + alpha * (qb + (0.5 * alpha) * qa);
            bool chg = false;
#pragma unroll 1
            for (int c = 0; c < C.n; c++) {
                double un = 0.0, ut = 0.0, dn = 0.0, dt = 0.0;
#pragma unroll
                for (int i = 0; i < kPdNv; i++) {
                    un = un + C.Jn[c][i] * qacc[i]; ut = ut + C.Jt[c][i] * qacc[i];
                    dn = dn + C.Jn[c][i] * dir[i]; dt = dt + C.Jt[c][i] * dir[i];
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double sm = r == 0 ? C.mu[c] : (r == 1 ? -C.mu[c] : 0.0);
                    const double x = (un + sm * ut) - C.aref[c][r], jd = dn + sm * dt;
                    const double xr = x + alpha * jd;
                    if ((x < 0.0) != (xr < 0.0)) chg = true;
                    if (xr < 0.0) {
                        const double D = C.D[c][r];
                        d1 = d1 + (D * xr) * jd;
                        d2 = d2 + (D * jd) * jd;
                        pa = pa + (0.5 * D * xr) * xr;
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < kPdNv; l++)
                if (lD[l] > 0.0) {
                    const double x = lside[l] * qacc[l] - laref[l], jd = lside[l] * dir[l];
                    const double xr = x + alpha * jd;
                    if ((x < 0.0) != (xr < 0.0)) chg = true;
                    if (xr < 0.0) {
                        d1 = d1 + (lD[l] * xr) * jd;
                        d2 = d2 + (lD[l] * jd) * jd;
                        pa = pa + (0.5 * lD[l] * xr) * xr;
                    }
                }
            if (fabs(d1) <= 1e-9 * fabs(slope0) || e == kPdLsEvals - 1) {
                exact = e == 0 && !chg && fabs(d1) <= 1e-9 * fabs(slope0);
                break;
            }
            if (d1 < 0.0) lo = alpha; else hi = alpha;
            double an = alpha - d1 / d2;
            if (an <= lo || (hi >= 0.0 && an >= hi)) an = (hi >= 0.0) ? 0.5 * (lo + hi) : 2.0 * alpha;
            alpha = an;
        }
#pragma unroll
        for (int i = 0; i < kPdNv; i++) qacc[i] = qacc[i] + alpha * dir[i];
        if ((p0 - pa) * ph.inv_scale < ph.tol || exact) break;
    }
}

// One sub-step: the env's PID (`_get_control`) at the state it starts from, then mj_step with the RK4 integrator
// (MuJoCo 2.0 mj_RungeKutta, restated): F0 = (v, qacc(X0)); for i = 1..3: dX = sum_j A[i-1][j] F[j] (mju_scl, then mju_addToScl
// in j order), X_i = (q0 + h dX_v, v0 + h dX_a), F_i = (v_i, qacc(X_i)); finally dX = sum_j B[j] F[j], q = q0 + h dX_v,
// v = v0 + h dX_a.  A = {1/2; 0 1/2; 0 0 1}, B = {1/6, 1/3, 1/3, 1/6}.
__device__ __forceinline__ void pd_substep(const PdHdr &ph, const double *__restrict__ PR, double *q, double *v, double *iterm,
                                           const double *desired, const double *prev, const double *tv0, PdCon &C, int &drop, double *qacc4) {
    double ctrl[kPdArm];
#pragma unroll
    for (int j = 0; j < kPdArm; j++) {
        const double pt = ph.kp * (desired[j] - q[j]);
        const double dt = ph.kd * (tv0[j] - v[j]);
        iterm[j] = ph.alpha * iterm[j] + ph.ki * (prev[j] - q[j]);
        ctrl[j] = (pt + dt) + iterm[j];
    }
    const double Acoef[3][3] = {{0.5, 0.0, 0.0}, {0.0, 0.5, 0.0}, {0.0, 0.0, 1.0}};
    const double Bcoef[4] = {1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0};
    double Fv[4][kPdNv], Fa[4][kPdNv], qi[kPdNv], vi[kPdNv];
#pragma unroll
    for (int i = 0; i < kPdNv; i++) Fv[0][i] = v[i];
    pd_forward(ph, PR, q, v, ctrl, Fa[0], C, drop);
#pragma unroll 1
    for (int s = 1; s < 4; s++) {
#pragma unroll
        for (int i = 0; i < kPdNv; i++) {
            double dv = Fv[0][i] * Acoef[s - 1][0], da = Fa[0][i] * Acoef[s - 1][0];
#pragma unroll
            for (int j = 1; j < 4; j++)
                if (j < s) { dv = dv + Fv[j][i] * Acoef[s - 1][j]; da = da + Fa[j][i] * Acoef[s - 1][j]; }
            qi[i] = q[i] + ph.h * dv;
            vi[i] = v[i] + ph.h * da;
        }
#pragma unroll
        for (int i = 0; i < kPdNv; i++) Fv[s][i] = vi[i];
        pd_forward(ph, PR, qi, vi, ctrl, Fa[s], C, drop);
    }
#pragma unroll
    for (int i = 0; i < kPdNv; i++) {
        double dv = Fv[0][i] * Bcoef[0], da = Fa[0][i] * Bcoef[0];
#pragma unroll
        for (int j = 1; j < 4; j++) { dv = dv + Fv[j][i] * Bcoef[j]; da = da + Fa[j][i] * Bcoef[j]; }
        q[i] = q[i] + ph.h * dv;
        v[i] = v[i] + ph.h * da;
        qacc4[i] = Fa[3][i];
    }
}

// Contact-force readout (mopa_env_set_contact_force), after the sub-step loop: the contacts of the 4th RK4 stage of the last sub-step -- what the
// constraint forces hold when the reference's `_do_simulation` returns -- with the edge forces recomputed from that stage's qacc
// (p_r = -D_r x_r where x_r = J_r qacc - aref_r < 0, as tests/pusher_dyn_ref.py's forward(want=True)), decoded as mj_contactForce decodes
// a pyramid: f0 = (p0 + p1) + (p2 + p3), f1 = mu (p0 - p1), f2 = mu (p2 - p3).  Row: (pair, dist, f0, f1, f2, 0, 0, 0); force = the sum
// of |f0| + |f1| + |f2| over the contacts in contact order, plain adds.  PARITY UNPINNED like the solve it reads.
__device__ __forceinline__ void pd_force_readout(const PdCon &C, const double *qacc, long long e, const CfOut &cf) {
    double force = 0.0;
#pragma unroll 1
    for (int c = 0; c < C.n; c++) {
        double un = 0.0, ut = 0.0;
#pragma unroll
        for (int i = 0; i < kPdNv; i++) { un = un + C.Jn[c][i] * qacc[i]; ut = ut + C.Jt[c][i] * qacc[i]; }
        double p[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double sm = r == 0 ? C.mu[c] : (r == 1 ? -C.mu[c] : 0.0);
            const double x = (un + sm * ut) - C.aref[c][r];
            p[r] = x < 0.0 ? -(C.D[c][r] * x) : 0.0;
        }
        const double f0 = (p[0] + p[1]) + (p[2] + p[3]);
        const double f1 = C.mu[c] * (p[0] - p[1]), f2 = C.mu[c] * (p[2] - p[3]);
        force = force + ((fabs(f0) + fabs(f1)) + fabs(f2));       // (f3 .. f5 = 0: adding them changes no bit)
        if (cf.rows) {
            double *row = cf.rows + ((size_t)e * (size_t)cf.K + (size_t)c) * 8;
            row[0] = (double)C.pair[c]; row[1] = C.dist[c]; row[2] = f0; row[3] = f1; row[4] = f2; row[5] = 0.0; row[6] = 0.0; row[7] = 0.0;
        }
    }
    cf.force[e] = force;
    if (cf.total) cf.total[e] = cf.total[e] + force;
    if (cf.count) cf.count[e] = C.n;
}

// mode 0: env.step physics (desired state by K4's rule, nsub sub-steps, prev_state <- desired); the reward / obs half follows in
//         k_env_step<3> (env_step_launch with qvel).  move_mask bit 0 clear: the command is recorded, no sub-step runs; bit 1: the
//         env sits the launch out.
// mode 1: n raw sub-steps towards desired_in [E,4] with prev_state [E,4] as the PID's prev (tests).
// stats (optional, [E] int32): contacts dropped by the cap over the launch.
// cf (optional, cf.force != nullptr): the contact-force readout of the last sub-step, for the envs that ran one.
__global__ __launch_bounds__(64) void k_pusher_dyn(EnvHdr h, const PdHdr *__restrict__ php, const double *__restrict__ GD,
                                                   const int32_t *__restrict__ GI, const double *__restrict__ PR, long long E, int mode, int n_steps,
                                                   double *__restrict__ qpos, double *__restrict__ qvel, double *__restrict__ i_term,
                                                   double *__restrict__ prev_state, unsigned char *__restrict__ has_prev,
                                                   const double *__restrict__ action, int is_planner, const unsigned char *__restrict__ move_mask,
                                                   const double *__restrict__ desired_in, int32_t *__restrict__ stats, CfOut cf) {
    const PdHdr &ph = *php;
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const unsigned flags = move_mask ? move_mask[e] : 1u;
    if (flags & 2u) return;
    double *row = qpos + e * h.nq;
    double *prev = prev_state + e * kPdArm;
    double des[kPdArm], pv[kPdArm], tv0[kPdArm];
    if (mode == 0) {
        const bool use_prev = is_planner && has_prev[e];
#pragma unroll
        for (int j = 0; j < kPdArm; j++) {
            pv[j] = use_prev ? prev[j] : row[ph.qadr[j]];     // `if not is_planner or self._prev_state is None: prev = joint positions`
            des[j] = pv[j];
        }
        // K4 kind 3's desired-state rule (move = false: it leaves the row alone and writes desired_state into des)
        env_advance<3>(h, GD, GI, row, des, use_prev, false, action + e * h.adim, nullptr, 0.0, is_planner);
        has_prev[e] = 1;
#pragma unroll
        for (int j = 0; j < kPdArm; j++) prev[j] = des[j];    // `self._prev_state = np.copy(desired_state)`
        if (!(flags & 1u)) return;
        n_steps = ph.nsub;
    } else {
#pragma unroll
        for (int j = 0; j < kPdArm; j++) { des[j] = desired_in[e * kPdArm + j]; pv[j] = prev[j]; }
    }
    // target_vel = (desired - prev) / frame_dt enters the D term multiplied by 0 (env/base.py:202)
#pragma unroll
    for (int j = 0; j < kPdArm; j++) tv0[j] = ((des[j] - pv[j]) / ph.frame_dt) * 0.0;
    double q[kPdNv], v[kPdNv], it[kPdArm];
#pragma unroll
    for (int i = 0; i < kPdNv; i++) { q[i] = row[ph.qadr[i]]; v[i] = qvel[e * kPdNv + i]; }
#pragma unroll
    for (int j = 0; j < kPdArm; j++) it[j] = i_term[e * kPdArm + j];
    PdCon C;
    C.n = 0;
    int drop = 0;
    double qacc4[kPdNv] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // qacc of the last sub-step's 4th stage (the readout's)
#pragma unroll 1
    for (int s = 0; s < n_steps; s++) pd_substep(ph, PR, q, v, it, des, pv, tv0, C, drop, qacc4);
    if (cf.force && n_steps > 0) pd_force_readout(C, qacc4, e, cf);
#pragma unroll
    for (int i = 0; i < kPdNv; i++) { row[ph.qadr[i]] = q[i]; qvel[e * kPdNv + i] = v[i]; }
#pragma unroll
    for (int j = 0; j < kPdArm; j++) i_term[e * kPdArm + j] = it[j];
    if (stats) stats[e] = drop;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct MopaPusherDyn {
    PdHdr *d_hdr = nullptr;
    double *d_pairs = nullptr;
    int32_t *stats = nullptr;
    ~MopaPusherDyn() {
        if (d_hdr) (void)hipFree(d_hdr);
        if (d_pairs) (void)hipFree(d_pairs);
    }
};
static void pd_free(void *p) { delete static_cast<MopaPusherDyn *>(p); }
static MopaPusherDyn *pd_of(const MopaEnv *env) { return env ? static_cast<MopaPusherDyn *>(env->pusher) : nullptr; }

extern "C" int mopa_pusher_dyn_desc_size(void) { return (int)sizeof(MopaPusherDynDesc); }

extern "C" int mopa_env_attach_pusher_dynamics(MopaEnv *env, const MopaPusherDynDesc *d) {
    if (!env || !d) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (env->hdr.kind != MOPA_ENV_PUSHER) return fail(MOPA_ERR_INVALID_ARG, "the Pusher dynamics attach to a PusherObstacle env only");
    if (env->hdr.n_arm != kPdArm || env->hdr.adim != kPdArm) return fail(MOPA_ERR_INVALID_ARG, "the Pusher dynamics take four arm joints");
    if (d->nsub < 1 || d->maxcon < 0 || d->maxcon > kPdMaxCon || MOPA_PUSHER_MAXCON != kPdMaxCon || d->iterations < 1 || d->npair < 0 || (d->npair > 0 && !d->pairs))
        return fail(MOPA_ERR_INVALID_ARG, "bad sub-step count, contact cap (<= 16), iteration count or pair table");
    if (!(d->timestep > 0.0) || !(d->frame_dt > 0.0)) return fail(MOPA_ERR_INVALID_ARG, "timestep and frame_dt must be > 0");
    for (int i = 0; i < kPdNv; i++)
        if (d->qadr[i] < 0 || d->qadr[i] >= env->hdr.nq) return fail(MOPA_ERR_INVALID_ARG, "dof qpos address out of range");
    for (int p = 0; p < d->npair; p++) {
        const double *r = d->pairs + (size_t)kPdPairRec * p;
        const int cls = (int)r[0], ba = (int)r[1], bb = (int)r[2];
        if (cls < 0 || cls > 2 || ba < -1 || ba > 4 || bb < -1 || bb > 4) return fail(MOPA_ERR_INVALID_ARG, "bad pair record");
    }
    PdHdr ph{};
    ph.npair = d->npair; ph.maxcon = d->maxcon; ph.iterations = d->iterations; ph.nsub = d->nsub; ph.contacts = d->npair > 0;
    for (int i = 0; i < kPdNv; i++) {
        ph.qadr[i] = d->qadr[i]; ph.limited[i] = d->limited[i]; ph.lo[i] = d->lo[i]; ph.hi[i] = d->hi[i];
        ph.armature[i] = d->armature[i]; ph.damping[i] = d->damping[i];
    }
    ph.base_x = d->base[0]; ph.base_y = d->base[1];
    for (int k = 0; k < kPdArm; k++) {
        ph.rel_x[k] = d->rel[2 * k]; ph.rel_y[k] = d->rel[2 * k + 1];
        ph.mass[k] = d->mass[k]; ph.com_x[k] = d->com[2 * k]; ph.com_y[k] = d->com[2 * k + 1]; ph.izz[k] = d->izz[k];
        ph.gear[k] = d->gear[k]; ph.kv[k] = d->kv[k]; ph.ctrl_lo[k] = d->ctrl_lo[k]; ph.ctrl_hi[k] = d->ctrl_hi[k];
    }
    ph.box_mass = d->box_mass; ph.box_org_x = d->box_org[0]; ph.box_org_y = d->box_org[1];
    ph.box_ref_x = d->box_ref[0]; ph.box_ref_y = d->box_ref[1];
    ph.kp = d->kp; ph.kd = d->kd; ph.ki = d->ki; ph.alpha = d->alpha; ph.frame_dt = d->frame_dt; ph.h = d->timestep;
    ph.tol = d->tolerance; ph.inv_scale = d->inv_scale;
    for (int k = 0; k < 8; k++) ph.lim_par[k] = d->lim_par[k];
    ON_DEVICE(env->device);
    auto *pd = new MopaPusherDyn();
    if (hipMalloc(&pd->d_hdr, sizeof(PdHdr)) != hipSuccess ||
        hipMalloc(&pd->d_pairs, sizeof(double) * (size_t)kPdPairRec * (size_t)std::max(d->npair, 1)) != hipSuccess) {
        delete pd;
        return fail(MOPA_ERR_HIP, "hipMalloc failed");
    }
    if (hipMemcpy(pd->d_hdr, &ph, sizeof(PdHdr), hipMemcpyHostToDevice) != hipSuccess ||
        (d->npair > 0 && hipMemcpy(pd->d_pairs, d->pairs, sizeof(double) * (size_t)kPdPairRec * d->npair, hipMemcpyHostToDevice) != hipSuccess)) {
        delete pd;
        return fail(MOPA_ERR_HIP, "hipMemcpy failed");
    }
    // the obs half (k_env_step<3>) reads qvel rows of 6: joint0..3, box_x, box_y
    env->dyn.nd = kPdNv;
    env->dyn.nv = kPdNv;
    if (env->pusher_free) env->pusher_free(env->pusher);
    env->pusher = pd;
    env->pusher_free = pd_free;
    env->pusher_maxcon = d->maxcon;
    env->cf = CfOut{nullptr, nullptr, nullptr, nullptr, 0};
    return MOPA_OK;
}

extern "C" int mopa_env_set_pusher_stats(MopaEnv *env, int32_t *stats_dev) {
    MopaPusherDyn *pd = pd_of(env);
    if (!pd) return fail(MOPA_ERR_INVALID_ARG, "env without Pusher dynamics (mopa_env_attach_pusher_dynamics)");
    pd->stats = stats_dev;
    return MOPA_OK;
}

static int pd_launch(MopaEnv *env, MopaPusherDyn *pd, int64_t E, int mode, int n, double *qpos, double *qvel, double *i_term, double *prev_state,
                     uint8_t *has_prev, const double *action, int is_planner, const uint8_t *move_mask, const double *desired, hipStream_t st) {
    const unsigned blocks = (unsigned)((E + 63) / 64);
    hipLaunchKernelGGL(k_pusher_dyn, dim3(blocks), dim3(64), 0, st, env->hdr, pd->d_hdr, env->d_dbl, env->d_int, pd->d_pairs, (long long)E, mode, n,
                       qpos, qvel, i_term, prev_state, has_prev, action, is_planner, move_mask, desired, pd->stats, env->cf);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_env_pusher_substeps_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *i_term_dev,
                                              const double *desired_dev, const double *prev_state_dev, int32_t n, void *stream) {
    MopaPusherDyn *pd = pd_of(env);
    if (!pd) return fail(MOPA_ERR_INVALID_ARG, "env without Pusher dynamics (mopa_env_attach_pusher_dynamics)");
    if (E < 0 || n < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E / n");
    if (E == 0 || n == 0) return MOPA_OK;
    if (!qpos_dev || !qvel_dev || !i_term_dev || !desired_dev || !prev_state_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(env->device);
    return pd_launch(env, pd, E, 1, n, qpos_dev, qvel_dev, i_term_dev, const_cast<double *>(prev_state_dev), nullptr, nullptr, 0, nullptr,
                     desired_dev, (hipStream_t)stream);
}

extern "C" int mopa_env_step_pusher_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *i_term_dev, double *prev_state_dev,
                                          uint8_t *has_prev_dev, int32_t *ep_len_dev, const double *action_dev, int32_t is_planner,
                                          const uint8_t *move_mask_dev, double *obs_dev, double *reward_dev, uint8_t *done_dev,
                                          uint8_t *success_dev, void *stream) {
    MopaPusherDyn *pd = pd_of(env);
    if (!pd) return fail(MOPA_ERR_INVALID_ARG, "env without Pusher dynamics (mopa_env_attach_pusher_dynamics)");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !qvel_dev || !obs_dev) return fail(MOPA_ERR_INVALID_ARG, "null qpos / qvel / obs buffer");
    if (action_dev && (!i_term_dev || !prev_state_dev || !has_prev_dev || !ep_len_dev || !reward_dev || !done_dev || !success_dev))
        return fail(MOPA_ERR_INVALID_ARG, "a stepping call needs i_term, prev_state, has_prev, ep_len, reward, done and success buffers");
    ON_DEVICE(env->device);
    hipStream_t st = (hipStream_t)stream;
    if (action_dev) {
        const int rc = pd_launch(env, pd, E, 0, 0, qpos_dev, qvel_dev, i_term_dev, prev_state_dev, has_prev_dev, action_dev, (int)is_planner,
                                 move_mask_dev, nullptr, st);
        if (rc != MOPA_OK) return rc;
    }
    return env_step_launch(env, E, qpos_dev, prev_state_dev, has_prev_dev, ep_len_dev, action_dev, (int)is_planner, move_mask_dev, obs_dev,
                           reward_dev, done_dev, success_dev, qvel_dev, st);
}

// One entry for both solver-backed contact stages (K7: mopa_env_attach_contacts, K8: mopa_env_attach_pusher_dynamics); the kernels read the
// pointers at every launch that follows (K7 from its header in device memory, K8 as a kernel argument).  All pointers null: off.  Call it
// between launches: a launch in flight on another stream may see either setting.
extern "C" int mopa_env_set_contact_force(MopaEnv *env, double *force_dev, double *total_dev, double *rows_dev, int32_t *count_dev, int32_t K) {
    if (!env) return fail(MOPA_ERR_INVALID_ARG, "null env");
    const bool k8 = pd_of(env) != nullptr;
    if (!k8 && !env->ct_on)
        return fail(MOPA_ERR_INVALID_ARG, "contact forces need a contact stage behind a constraint solver (K7 contacts or the Pusher dynamics)");
    if (!force_dev && (total_dev || rows_dev || count_dev)) return fail(MOPA_ERR_INVALID_ARG, "force_dev is null but another output is set");
    const int maxcon = k8 ? env->pusher_maxcon : env->ct_maxcon;
    if (rows_dev && K < maxcon) return fail(MOPA_ERR_INVALID_ARG, "rows_dev needs K >= the stage's maxcon rows per env");
    const CfOut cf{force_dev, total_dev, rows_dev, count_dev, rows_dev ? (int)K : 0};
    if (!k8) {       // K7 reads it from its device-side header (a blocking copy: ordered behind the launches already on the default stream)
        ON_DEVICE(env->device);
        HIP_TRY(hipMemcpy(reinterpret_cast<char *>(env->d_cthdr) + offsetof(CtHdr, cf), &cf, sizeof(CfOut), hipMemcpyHostToDevice));
    }
    env->cf = cf;
    return MOPA_OK;
}
