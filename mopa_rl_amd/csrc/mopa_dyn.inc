// mopa_dyn.inc -- K6: contact-free SERVO DYNAMICS of the actuated kinematic tree inside env.step (SURVEY.md 8 f4b, stage A).
// (included by mopa_hip.hip after mopa_env.inc; C ABI in include/mopa_hip.h "mopa_env_*dyn*")
//
// What it restates: the reference's `_do_simulation` loop -- 75 x { qfrc_applied[arm] = qfrc_bias[arm]; ctrl = desired_state;
// sim.step() } (env/sawyer/sawyer_push_obstacle.py:186-203, env/base.py:388-392) -- for a robot that touches nothing:
// per sub-step the [3P] mj_step pipeline on the arm's own tree (7 hinges + 2 gripper slides): kinematics, composite-rigid-body
// inertia + armature, RNE bias force incl. gravity, passive damping, force-limited position servos (sawyer_joint_pos_act.xml),
// semi-implicit Euler at 2 ms with joint damping integrated implicitly (sawyer_dependencies.xml:11).  The arithmetic, in
// this order, is the specification the CPU checker under tests restates (spatial vectors in world axes about the
// world origin); tests compare every sub-step bit for bit.  Stage-A limits (no contacts, inelastic joint stops, welded
// bodies lumped) are listed there and in DESIGN.md.
//
// Mapping: one LANE per env, one wave per workgroup.  The per-body quantities of a sub-step (joint subspace S 6, inertia
// about the origin 10, force 6 doubles per body) are indexed by body at run time, so they live in LDS as [slot][64]
// columns (conflict-free ds_read/write_b64), as do the env's joint state and the one DFS save slot of the tree's branch
// point (the hand: both fingers hang off it).  253 doubles per lane = 127 KiB per wave: one wave per CU, which at the
// bench's 4096 envs (64 waves) is not what limits the launch -- the 75 x ~5 k dependent FP64 operations of a lane are.
// The 9 x 9 solve runs in registers (fully unrolled L D L^T, static indices).  Per-dof model constants are wave-uniform
// and come through scalar loads.
// HBM per env-step: the qpos row's 9 entries + qvel + lagged bias in and out (9 x 8 B x 6) + action / prev_state: ~0.6 KB.

// (kDynMax, DynHdr: mopa_env.inc, next to the env handle that carries them)
constexpr int kDynRec = 32;          // doubles per dof record
// record layout
constexpr int DR_RPOS = 0, DR_RQUAT = 3, DR_AXIS = 7, DR_JPOS = 10, DR_QREF = 13, DR_MASS = 14, DR_IPOS = 15, DR_INERTIA = 18,
              DR_DAMP = 24, DR_ARM = 25, DR_LO = 26, DR_HI = 27, DR_KP = 28, DR_FLO = 29, DR_FHI = 30;
// LDS slots ([slot][64] doubles)
constexpr int DL_Q = 0, DL_V = kDynMax, DL_LAG = 2 * kDynMax, DL_CTRL = 3 * kDynMax, DL_S = 4 * kDynMax, DL_IC = DL_S + 6 * kDynMax,
              DL_F = DL_IC + 10 * kDynMax, DL_OBJ = DL_F + 6 * kDynMax, DL_OBJF = DL_OBJ + 13, DL_SAVE = DL_OBJF + 6, kDynSaveStride = 19;
// (DL_OBJ: the manipulated object's state, stage B: position 3, quaternion 4, linear / angular velocity 3 + 3;
//  DL_OBJF: the force / torque accumulated on it in the current sub-step -- parked in LDS so that the arm's forward pass
//  does not carry the object's 60 registers: they are loaded only for a body that has a collider near)
constexpr int kObjRec = 18;          // doubles per collider record: type, size 3, pos 3, mat 9, mu, rbound


struct SpV { V3 w, v; };

__device__ __forceinline__ double spdot(const SpV &a, const SpV &b) { return dot3(a.w, b.w) + dot3(a.v, b.v); }
// I (w; v) = (J w + h x v;  m v - h x w),  J: xx yy zz xy xz yz
__device__ __forceinline__ SpV sp_inertia_mul(double m, V3 hh, const double *J, const SpV &x) {
    const V3 r0{J[0], J[3], J[4]}, r1{J[3], J[1], J[5]}, r2{J[4], J[5], J[2]};
    const V3 jw{dot3(r0, x.w), dot3(r1, x.w), dot3(r2, x.w)};
    const V3 hv = cross3(hh, x.v), hw = cross3(hh, x.w);
    SpV r;
    r.w = add3(jw, hv);
    r.v = V3{fma(m, x.v.x, -hw.x), fma(m, x.v.y, -hw.y), fma(m, x.v.z, -hw.z)};
    return r;
}

#define DLW(slot) W[(size_t)(slot) * ST]      // ST: element stride of a slot (64: one column per lane; 4: the contact kernel, 4 envs per wave)

template <int ST = 64>
__device__ __forceinline__ SpV dl_ld6(const double *W, int slot) {
    return SpV{V3{DLW(slot), DLW(slot + 1), DLW(slot + 2)}, V3{DLW(slot + 3), DLW(slot + 4), DLW(slot + 5)}};
}
template <int ST = 64>
__device__ __forceinline__ void dl_st6(double *W, int slot, const SpV &x) {
    DLW(slot) = x.w.x; DLW(slot + 1) = x.w.y; DLW(slot + 2) = x.w.z;
    DLW(slot + 3) = x.v.x; DLW(slot + 4) = x.v.y; DLW(slot + 5) = x.v.z;
}


// ---- stage B (Push): the manipulated object as a free body with PENALTY contacts --------------------------------------
// NOT MuJoCo's constraint solver: spring-damper normal force + capped regularised Coulomb friction at the object's feature
// points found inside a collider (and a moving box's vertices found inside the object); one-way coupling (the robot moves
// the object, the reaction on the arm is neglected).  Same arithmetic, in the same order, as the CPU checker's obj_substep.
// mine: this lane's collider mask (bit c: collider c passed the lane's last full scan); any: the wave's union of them
struct ObjCtx { V3 p; double R[9]; V3 v, w, F, T; unsigned long long mine, any; bool precull; };

// point y in a collider's frame: inside -> penetration depth and outward unit normal (collider frame)
__device__ __forceinline__ bool obj_point_in_shape(int type, double s0, double s1, double s2, V3 y, double &depth, V3 &nl) {
    if (type == G_PLANE) {
        if (!(y.z < 0.0)) return false;
        depth = -y.z; nl = V3{0.0, 0.0, 1.0};
        return true;
    }
    if (type == G_SPHERE || type == G_CAPSULE) {
        V3 c{0.0, 0.0, 0.0};
        if (type == G_CAPSULE) c.z = clampd(y.z, -s1, s1);
        const V3 dv = sub3(y, c);
        const double dd = dot3(dv, dv);
        if (!(dd < s0 * s0)) return false;
        const double dist = sqrt(dd);
        depth = s0 - dist;
        if (dist > 0.0) nl = V3{dv.x / dist, dv.y / dist, dv.z / dist};
        else nl = V3{0.0, 0.0, 1.0};
        return true;
    }
    if (type == G_CYLINDER) {
        const double az = fabs(y.z), rr = fma(y.y, y.y, y.x * y.x);
        if (!(az < s1) || !(rr < s0 * s0)) return false;
        const double rho = sqrt(rr), ds = s0 - rho, dc = s1 - az;
        if (ds < dc && rho > 0.0) { depth = ds; nl = V3{y.x / rho, y.y / rho, 0.0}; }
        else { depth = dc; nl = V3{0.0, 0.0, (y.z < 0.0) ? -1.0 : 1.0}; }
        return true;
    }
    if (type == G_BOX) {
        const double d0 = s0 - fabs(y.x), d1 = s1 - fabs(y.y), d2 = s2 - fabs(y.z);
        if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) return false;
        int a = 0;
        double dm = d0;
        if (d1 < dm) { dm = d1; a = 1; }
        if (d2 < dm) { dm = d2; a = 2; }
        depth = dm;
        nl = V3{0.0, 0.0, 0.0};
        if (a == 0) nl.x = (y.x < 0.0) ? -1.0 : 1.0;
        else if (a == 1) nl.y = (y.y < 0.0) ? -1.0 : 1.0;
        else nl.z = (y.z < 0.0) ? -1.0 : 1.0;
        return true;
    }
    return false;
}

// Feature point k of a box (centre c, scaled axes aX = hx R[:,0], aY, aZ): c + sx aX + sy aY + sz aZ, signs in {-1, 0, +1}, zero
// terms skipped, added in x, y, z order.  k = 0..7 the vertices (bit 0 / 1 / 2: +x / +y / +z), 8..19 edge midpoints, 20..25
// face centres.  The loops over k are unrolled, so the signs are compile-time constants: no table loads, no multiplies.
constexpr int kObjFeat = 26;
// sign + 1 of feature k along x / y / z, two bits per feature (the loops over k stay rolled: unrolled 26-fold with the contact
// path inlined, the kernel ran out of registers)
constexpr unsigned long long obj_pack(int axis) {
    const signed char sg[kObjFeat][3] = {
        {-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {-1, 1, 1}, {1, 1, 1},
        {-1, -1, 0}, {-1, 1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {1, 0, -1}, {1, 0, 1},
        {0, -1, -1}, {0, -1, 1}, {0, 1, -1}, {0, 1, 1},
        {-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
    unsigned long long w = 0;
    for (int k = 0; k < kObjFeat; k++) w |= (unsigned long long)(sg[k][axis] + 1) << (2 * k);
    return w;
}
constexpr unsigned long long kObjSx = obj_pack(0), kObjSy = obj_pack(1), kObjSz = obj_pack(2);
__device__ __forceinline__ V3 obj_feature(V3 c, V3 aX, V3 aY, V3 aZ, int k) {
    const int sx = (int)((kObjSx >> (2 * k)) & 3ull) - 1, sy = (int)((kObjSy >> (2 * k)) & 3ull) - 1, sz = (int)((kObjSz >> (2 * k)) & 3ull) - 1;
    V3 x = c;
    if (sx > 0) x = add3(x, aX); else if (sx < 0) x = sub3(x, aX);
    if (sy > 0) x = add3(x, aY); else if (sy < 0) x = sub3(x, aY);
    if (sz > 0) x = add3(x, aZ); else if (sz < 0) x = sub3(x, aZ);
    return x;
}

__device__ __forceinline__ void obj_apply(const DynHdr &dh, ObjCtx &o, V3 x, V3 n, double depth, V3 u, double mu) {
    const double un = dot3(u, n);
    const double fn = fma(-dh.o_dn, un, dh.o_kn * depth);
    if (!(fn > 0.0)) return;
    const V3 ut = addscl3(u, n, -un);
    const double sc = dmin((mu * fn) / sqrt(dot3(ut, ut) + dh.o_eps2), dh.o_ctmax);
    const V3 f{fma(fn, n.x, -(sc * ut.x)), fma(fn, n.y, -(sc * ut.y)), fma(fn, n.z, -(sc * ut.z))};
    o.F = add3(o.F, f);
    o.T = add3(o.T, cross3(sub3(x, o.p), f));
}

// the colliders riding on dynamic body b (b = -1: the static ones; bpos / bmat / V unused then)
__device__ __forceinline__ void obj_colliders(const DynHdr &dh, const double *__restrict__ OD, ObjCtx &o, int b, V3 bpos, const double *bmat,
                                              const SpV &V) {
    const double *recs = OD + 3 * dh.obj_nfeat;
    for (int c = dh.co_first[b + 1]; c < dh.co_first[b + 2]; c++) {
        if (!o.precull && !((o.any >> c) & 1ull)) continue;        // (wave-uniform) no lane has this collider near
        const bool listed = (o.mine >> c) & 1ull;
        if (!o.precull && !listed) continue;
        const double *rec = recs + kObjRec * c;
        const int type = (int)rec[0];
        const double s0 = rec[1], s1 = rec[2], s2 = rec[3], mu = rec[16];
        V3 pg, vo{0.0, 0.0, 0.0}, wo{0.0, 0.0, 0.0};
        double Rg[9];
        // broad phase 1: bounding spheres about the collider's centre (a plane has none), before a moving collider's
        // rotation is composed
        if (b < 0) pg = ld3(rec + 4);
        else pg = add3(bpos, mat_vec(bmat, ld3(rec + 4)));
        const V3 dc = sub3(o.p, pg);
        if (o.precull) {
            // the full scan of every o_every-th sub-step: bounding spheres inflated by the margin decide which colliders the
            // following sub-steps visit at all
            const double rm = (dh.o_rbound + rec[17]) + dh.o_margin;
            const bool near = type == G_PLANE || !(dot3(dc, dc) > rm * rm);
            if (near) o.mine |= 1ull << c;
            if (__any(near)) o.any |= 1ull << c;
            if (!near) continue;
        }
        if (type != G_PLANE) {
            const double rs = dh.o_rbound + rec[17];
            if (dot3(dc, dc) > rs * rs) continue;
        }
        if (b < 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) Rg[k] = rec[7 + k];
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int cc = 0; cc < 3; cc++)
                    Rg[3 * r + cc] = dot3(ld3(bmat + 3 * r), V3{rec[7 + cc], rec[7 + 3 + cc], rec[7 + 6 + cc]});
            wo = V.w; vo = V.v;
        }
        // broad phase 2: the object's bounding sphere against the shape itself, in the collider's frame
        {
            const V3 yc = matT_vec(Rg, dc);
            const double rb = dh.o_rbound;
            if (type == G_PLANE) { if (yc.z > rb) continue; }
            else if (type == G_BOX) { if (fabs(yc.x) >= s0 + rb || fabs(yc.y) >= s1 + rb || fabs(yc.z) >= s2 + rb) continue; }
            else if (type == G_CYLINDER) {
                const double rr = s0 + rb;
                if (fabs(yc.z) >= s1 + rb || fma(yc.y, yc.y, yc.x * yc.x) >= rr * rr) continue;
            }
        }
        const int nf = (b < 0) ? 8 : kObjFeat;
        const V3 cX{o.R[0] * dh.o_h0, o.R[3] * dh.o_h0, o.R[6] * dh.o_h0}, cY{o.R[1] * dh.o_h1, o.R[4] * dh.o_h1, o.R[7] * dh.o_h1},
                 cZ{o.R[2] * dh.o_h2, o.R[5] * dh.o_h2, o.R[8] * dh.o_h2};
#pragma unroll 1
        for (int k = 0; k < nf; k++) {      // the object's feature points inside the collider
            const V3 x = obj_feature(o.p, cX, cY, cZ, k);
            const V3 y = matT_vec(Rg, sub3(x, pg));
            double depth;
            V3 nl;
            if (!obj_point_in_shape(type, s0, s1, s2, y, depth, nl)) continue;
            const V3 n = mat_vec(Rg, nl);
            V3 u = add3(o.v, cross3(o.w, sub3(x, o.p)));
            const V3 cx = cross3(wo, x);
            u = V3{u.x - (vo.x + cx.x), u.y - (vo.y + cx.y), u.z - (vo.z + cx.z)};
            obj_apply(dh, o, x, n, depth, u, mu);
        }
        if (b >= 0 && type == G_BOX) {             // a moving box's vertices inside the object
            const V3 gX{Rg[0] * s0, Rg[3] * s0, Rg[6] * s0}, gY{Rg[1] * s1, Rg[4] * s1, Rg[7] * s1}, gZ{Rg[2] * s2, Rg[5] * s2, Rg[8] * s2};
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const V3 x = obj_feature(pg, gX, gY, gZ, k);
                const V3 t = sub3(x, o.p);
                const V3 y = matT_vec(o.R, t);
                double depth;
                V3 nl;
                if (!obj_point_in_shape(G_BOX, dh.o_h0, dh.o_h1, dh.o_h2, y, depth, nl)) continue;
                V3 n = mat_vec(o.R, nl);
                n = V3{-n.x, -n.y, -n.z};           // the vertex pushes the object inwards
                V3 u = add3(o.v, cross3(o.w, t));
                const V3 cx = cross3(wo, x);
                u = V3{u.x - (vo.x + cx.x), u.y - (vo.y + cx.y), u.z - (vo.z + cx.z)};
                obj_apply(dh, o, x, n, depth, u, mu);
            }
        }
    }
}

__device__ __forceinline__ void obj_load(const double *W, ObjCtx &o) {
    o.p = V3{W[(size_t)(DL_OBJ) * 64], W[(size_t)(DL_OBJ + 1) * 64], W[(size_t)(DL_OBJ + 2) * 64]};
    const Q4 q{W[(size_t)(DL_OBJ + 3) * 64], W[(size_t)(DL_OBJ + 4) * 64], W[(size_t)(DL_OBJ + 5) * 64], W[(size_t)(DL_OBJ + 6) * 64]};
    quat2mat(o.R, q);
    o.v = V3{W[(size_t)(DL_OBJ + 7) * 64], W[(size_t)(DL_OBJ + 8) * 64], W[(size_t)(DL_OBJ + 9) * 64]};
    o.w = V3{W[(size_t)(DL_OBJ + 10) * 64], W[(size_t)(DL_OBJ + 11) * 64], W[(size_t)(DL_OBJ + 12) * 64]};
}
__device__ __forceinline__ void obj_ldF(const double *W, ObjCtx &o) {
    o.F = V3{W[(size_t)(DL_OBJF) * 64], W[(size_t)(DL_OBJF + 1) * 64], W[(size_t)(DL_OBJF + 2) * 64]};
    o.T = V3{W[(size_t)(DL_OBJF + 3) * 64], W[(size_t)(DL_OBJF + 4) * 64], W[(size_t)(DL_OBJF + 5) * 64]};
}
__device__ __forceinline__ void obj_stF(double *W, const ObjCtx &o) {
    W[(size_t)(DL_OBJF) * 64] = o.F.x; W[(size_t)(DL_OBJF + 1) * 64] = o.F.y; W[(size_t)(DL_OBJF + 2) * 64] = o.F.z;
    W[(size_t)(DL_OBJF + 3) * 64] = o.T.x; W[(size_t)(DL_OBJF + 4) * 64] = o.T.y; W[(size_t)(DL_OBJF + 5) * 64] = o.T.z;
}
// gravity + damping, then the static colliders; the accumulators go to LDS
__device__ __forceinline__ void obj_begin(const DynHdr &dh, const double *__restrict__ OD, double *W, bool precull, unsigned long long &mine,
                                          unsigned long long &any) {
    ObjCtx o;
    o.precull = precull;
    o.mine = precull ? 0ull : mine; o.any = precull ? 0ull : any;
    obj_load(W, o);
    o.F = V3{fma(dh.o_mass, dh.gx, -(dh.o_damp * o.v.x)), fma(dh.o_mass, dh.gy, -(dh.o_damp * o.v.y)), fma(dh.o_mass, dh.gz, -(dh.o_damp * o.v.z))};
    o.T = V3{-(dh.o_damp * o.w.x), -(dh.o_damp * o.w.y), -(dh.o_damp * o.w.z)};
    const SpV none{V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 0.0}};
    obj_colliders(dh, OD, o, -1, V3{0.0, 0.0, 0.0}, o.R, none);
    obj_stF(W, o);
    mine = o.mine; any = o.any;
}
// the colliders riding on dynamic body b: the object's state is fetched only if the body has one to look at
__device__ __forceinline__ void obj_body(const DynHdr &dh, const double *__restrict__ OD, double *W, bool precull, unsigned long long &mine,
                                         unsigned long long &any, int b, V3 bpos, const double *bmat, const SpV &V) {
    const int c0 = dh.co_first[b + 1], c1 = dh.co_first[b + 2];
    if (c1 <= c0) return;
    if (!precull) {
        const unsigned long long span = ((c1 - c0 >= 64) ? ~0ull : ((1ull << (c1 - c0)) - 1ull)) << c0;
        if (!(any & span)) return;         // (wave-uniform) none of this body's colliders passed anyone's last full scan
    }
    ObjCtx o;
    o.precull = precull; o.mine = mine; o.any = any;
    obj_load(W, o);
    obj_ldF(W, o);
    obj_colliders(dh, OD, o, b, bpos, bmat, V);
    obj_stF(W, o);
    mine = o.mine; any = o.any;
}

// semi-implicit Euler: linear in the world, angular in the body frame (principal inertia)
__device__ __forceinline__ void obj_integrate(const DynHdr &dh, double *W) {
    ObjCtx o;
    obj_load(W, o);
    obj_ldF(W, o);
    const double h = dh.h;
    V3 v{fma(h, o.F.x * dh.o_imass, o.v.x), fma(h, o.F.y * dh.o_imass, o.v.y), fma(h, o.F.z * dh.o_imass, o.v.z)};
    const V3 wb = matT_vec(o.R, o.w), Tb = matT_vec(o.R, o.T);
    const V3 Iw{dh.o_in0 * wb.x, dh.o_in1 * wb.y, dh.o_in2 * wb.z};
    const V3 g = cross3(wb, Iw);
    const V3 ab{(Tb.x - g.x) * dh.o_iin0, (Tb.y - g.y) * dh.o_iin1, (Tb.z - g.z) * dh.o_iin2};
    const V3 aw = mat_vec(o.R, ab);
    const V3 w{fma(h, aw.x, o.w.x), fma(h, aw.y, o.w.y), fma(h, aw.z, o.w.z)};
    const V3 p{fma(h, v.x, o.p.x), fma(h, v.y, o.p.y), fma(h, v.z, o.p.z)};
    double q0 = W[(size_t)(DL_OBJ + 3) * 64], q1 = W[(size_t)(DL_OBJ + 4) * 64], q2 = W[(size_t)(DL_OBJ + 5) * 64], q3 = W[(size_t)(DL_OBJ + 6) * 64];
    const double hh = 0.5 * h;
    const double dq0 = -(fma(w.z, q3, fma(w.y, q2, w.x * q1)));
    const double dq1 = fma(w.y, q3, fma(-w.z, q2, w.x * q0));
    const double dq2 = fma(w.z, q1, fma(-w.x, q3, w.y * q0));
    const double dq3 = fma(w.x, q2, fma(-w.y, q1, w.z * q0));
    q0 = fma(hh, dq0, q0); q1 = fma(hh, dq1, q1); q2 = fma(hh, dq2, q2); q3 = fma(hh, dq3, q3);
    const double qi = 1.0 / sqrt(fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0))));
    W[(size_t)(DL_OBJ) * 64] = p.x; W[(size_t)(DL_OBJ + 1) * 64] = p.y; W[(size_t)(DL_OBJ + 2) * 64] = p.z;
    W[(size_t)(DL_OBJ + 3) * 64] = q0 * qi; W[(size_t)(DL_OBJ + 4) * 64] = q1 * qi; W[(size_t)(DL_OBJ + 5) * 64] = q2 * qi; W[(size_t)(DL_OBJ + 6) * 64] = q3 * qi;
    W[(size_t)(DL_OBJ + 7) * 64] = v.x; W[(size_t)(DL_OBJ + 8) * 64] = v.y; W[(size_t)(DL_OBJ + 9) * 64] = v.z;
    W[(size_t)(DL_OBJ + 10) * 64] = w.x; W[(size_t)(DL_OBJ + 11) * 64] = w.y; W[(size_t)(DL_OBJ + 12) * 64] = w.z;
}

// kinematics + joint subspaces + inertias about the origin + RNE forward pass (qacc = 0): fills S, IC, F columns
// (oc != nullptr: the contacts of the colliders riding on each body go into the object's force accumulators)
struct ObjPass { bool on, precull; unsigned long long mine, any; };
// own: bit i = this wave computes body i's joint-subspace / inertia / force columns (the single-wave kernel: all bits; in the
// workgroup form every wave walks the whole chain -- pose, S, V, A are cheap and serial -- but only the owner does the rest)
// xp_slot >= 0 (the contact kernel): every body's world pose (pos 3, quat 4) is kept at slot xp_slot + 7 i.
// WALK_ONLY (the contact kernel, 16 lanes per env): only the serial part runs here -- pose, joint subspace (stored for EVERY
// body), velocity and bias acceleration -- with V staged at DL_F + 6 i and A at DL_IC + 6 i; the inertia about the origin and the
// force of each body follow lane-parallel, one body per lane (dyn_forward_owner_load / _store below): same expressions, so
// the same bits as the owner blocks inside the walk.
template <int ST = 64, bool OBJB = true, bool WALK_ONLY = false>
__device__ __forceinline__ void dyn_forward_pass(const DynHdr &dh, const double *__restrict__ DD, double *W,
                                                 const double *__restrict__ OD, ObjPass &op, unsigned own = ~0u, int xp_slot = -1) {
    V3 pos{0.0, 0.0, 0.0};
    Q4 quat{1.0, 0.0, 0.0, 0.0};
    double mat[9];
    SpV Vc{V3{0, 0, 0}, V3{0, 0, 0}}, Ac = Vc;
    for (int i = 0; i < dh.nd; i++) {
        const double *rec = DD + kDynRec * i;
        SpV Vp, Ap;
        const int ld = dh.load[i];
        if (ld == -2) {
            pos = ld3(rec + DR_RPOS);
            quat = Q4{rec[DR_RQUAT], rec[DR_RQUAT + 1], rec[DR_RQUAT + 2], rec[DR_RQUAT + 3]};
            Vp = SpV{V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 0.0}};
            Ap = SpV{V3{0.0, 0.0, 0.0}, V3{-dh.gx, -dh.gy, -dh.gz}};
        } else {
            V3 ppos;
            Q4 pquat;
            if (ld >= 0) {
                const int s = DL_SAVE + kDynSaveStride * ld;
                ppos = V3{DLW(s), DLW(s + 1), DLW(s + 2)};
                pquat = Q4{DLW(s + 3), DLW(s + 4), DLW(s + 5), DLW(s + 6)};
                Vp = dl_ld6<ST>(W, s + 7);
                Ap = dl_ld6<ST>(W, s + 13);
                quat2mat(mat, pquat);
            } else {
                ppos = pos; pquat = quat; Vp = Vc; Ap = Ac;
            }
            pos = add3(ppos, mat_vec(mat, ld3(rec + DR_RPOS)));
            quat = quat_mul(pquat, Q4{rec[DR_RQUAT], rec[DR_RQUAT + 1], rec[DR_RQUAT + 2], rec[DR_RQUAT + 3]});
        }
        const V3 ax = ld3(rec + DR_AXIS), jp = ld3(rec + DR_JPOS);
        const int jt = dh.jtype[i];
        const double dq = DLW(DL_Q + i) - rec[DR_QREF];
        apply_joint(jt, ax, jp, is_zero3(jp), dq, pos, quat);
        quat = quat_normalize(quat);
        quat2mat(mat, quat);
        // joint subspace
        const V3 a = mat_vec(mat, ax);
        SpV S;
        if (jt == J_SLIDE) { S.w = V3{0.0, 0.0, 0.0}; S.v = a; }
        else { const V3 r = add3(pos, mat_vec(mat, jp)); S.w = a; S.v = cross3(r, a); }
        const bool owned = !WALK_ONLY && ((own >> i) & 1u);
        if (owned || WALK_ONLY) dl_st6<ST>(W, DL_S + 6 * i, S);
        // velocities, bias accelerations
        const double qd = DLW(DL_V + i);
        const SpV vj{V3{S.w.x * qd, S.w.y * qd, S.w.z * qd}, V3{S.v.x * qd, S.v.y * qd, S.v.z * qd}};
        SpV V, A;
        V.w = add3(Vp.w, vj.w); V.v = add3(Vp.v, vj.v);
        {
            const V3 c0 = cross3(Vp.w, vj.w), c1 = cross3(Vp.w, vj.v), c2 = cross3(Vp.v, vj.w);
            A.w = add3(Ap.w, c0);
            A.v = add3(Ap.v, add3(c1, c2));
        }
        if (owned) {
        // inertia about the world origin: J = R Ic R^T + m (c.c 1 - c c^T)
        const double m = rec[DR_MASS], *ic = rec + DR_INERTIA;
        const V3 c = add3(pos, mat_vec(mat, ld3(rec + DR_IPOS)));
        const V3 i0{ic[0], ic[3], ic[4]}, i1{ic[3], ic[1], ic[5]}, i2{ic[4], ic[5], ic[2]};
        const V3 R0 = ld3(mat), R1 = ld3(mat + 3), R2 = ld3(mat + 6);
        const V3 T0{dot3(R0, i0), dot3(R0, i1), dot3(R0, i2)}, T1{dot3(R1, i0), dot3(R1, i1), dot3(R1, i2)},
                 T2{dot3(R2, i0), dot3(R2, i1), dot3(R2, i2)};
        const double cc = dot3(c, c);
        double J[6];
        J[0] = fma(m, cc - c.x * c.x, dot3(T0, R0));
        J[1] = fma(m, cc - c.y * c.y, dot3(T1, R1));
        J[2] = fma(m, cc - c.z * c.z, dot3(T2, R2));
        J[3] = fma(-m, c.x * c.y, dot3(T0, R1));
        J[4] = fma(-m, c.x * c.z, dot3(T0, R2));
        J[5] = fma(-m, c.y * c.z, dot3(T1, R2));
        const V3 hh{m * c.x, m * c.y, m * c.z};
        const int oi = DL_IC + 10 * i;
        DLW(oi) = m; DLW(oi + 1) = hh.x; DLW(oi + 2) = hh.y; DLW(oi + 3) = hh.z;
#pragma unroll
        for (int k = 0; k < 6; k++) DLW(oi + 4 + k) = J[k];
        // force
        SpV F;
        {
            const SpV IA = sp_inertia_mul(m, hh, J, A), IV = sp_inertia_mul(m, hh, J, V);
            const V3 c0 = cross3(V.w, IV.w), c1 = cross3(V.v, IV.v), c2 = cross3(V.w, IV.v);
            F.w = add3(IA.w, add3(c0, c1));
            F.v = add3(IA.v, c2);
        }
        dl_st6<ST>(W, DL_F + 6 * i, F);
        }
        if (WALK_ONLY) {
            dl_st6<ST>(W, DL_F + 6 * i, V);
            dl_st6<ST>(W, DL_IC + 6 * i, A);
        }
        if (OBJB && op.on) obj_body(dh, OD, W, op.precull, op.mine, op.any, i, pos, mat, V);
        if (xp_slot >= 0) {
            const int s = xp_slot + 7 * i;
            DLW(s) = pos.x; DLW(s + 1) = pos.y; DLW(s + 2) = pos.z;
            DLW(s + 3) = quat.w; DLW(s + 4) = quat.x; DLW(s + 5) = quat.y; DLW(s + 6) = quat.z;
        }
        Vc = V; Ac = A;
        if (dh.save[i] >= 0) {
            const int s = DL_SAVE + kDynSaveStride * dh.save[i];
            DLW(s) = pos.x; DLW(s + 1) = pos.y; DLW(s + 2) = pos.z;
            DLW(s + 3) = quat.w; DLW(s + 4) = quat.x; DLW(s + 5) = quat.y; DLW(s + 6) = quat.z;
            dl_st6<ST>(W, s + 7, V);
            dl_st6<ST>(W, s + 13, A);
        }
    }
}

// The owner block of body i after a WALK_ONLY pass, in two halves so that every lane has read its staged inputs before any lane
// overwrites the columns they were staged in: _load fetches pose / V / A of body i, _store derives the inertia about the
// origin and the force (the expressions of the owner block above) and writes the IC and F columns of body i.
struct DynOwnerIn { V3 pos; Q4 quat; SpV V, A; };
template <int ST = 64>
__device__ __forceinline__ DynOwnerIn dyn_forward_owner_load(const double *W, int xp_slot, int i) {
    DynOwnerIn in;
    const int s = xp_slot + 7 * i;
    in.pos = V3{DLW(s), DLW(s + 1), DLW(s + 2)};
    in.quat = Q4{DLW(s + 3), DLW(s + 4), DLW(s + 5), DLW(s + 6)};
    in.V = dl_ld6<ST>(W, DL_F + 6 * i);
    in.A = dl_ld6<ST>(W, DL_IC + 6 * i);
    return in;
}
// (mass, ipos, ic: the body's lumped inertial -- the contact kernel hands the wave's LDS copy: with a lane-varying body index the
// dof records would be vector loads from global memory)
template <int ST = 64>
__device__ __forceinline__ void dyn_forward_owner_store(double m, V3 ipos, const double *ic, double *W, int i, const DynOwnerIn &in) {
    double mat[9];
    quat2mat(mat, in.quat);
    const V3 pos = in.pos;
    const SpV &V = in.V, &A = in.A;
    const V3 c = add3(pos, mat_vec(mat, ipos));
    const V3 i0{ic[0], ic[3], ic[4]}, i1{ic[3], ic[1], ic[5]}, i2{ic[4], ic[5], ic[2]};
    const V3 R0 = ld3(mat), R1 = ld3(mat + 3), R2 = ld3(mat + 6);
    const V3 T0{dot3(R0, i0), dot3(R0, i1), dot3(R0, i2)}, T1{dot3(R1, i0), dot3(R1, i1), dot3(R1, i2)},
             T2{dot3(R2, i0), dot3(R2, i1), dot3(R2, i2)};
    const double cc = dot3(c, c);
    double J[6];
    J[0] = fma(m, cc - c.x * c.x, dot3(T0, R0));
    J[1] = fma(m, cc - c.y * c.y, dot3(T1, R1));
    J[2] = fma(m, cc - c.z * c.z, dot3(T2, R2));
    J[3] = fma(-m, c.x * c.y, dot3(T0, R1));
    J[4] = fma(-m, c.x * c.z, dot3(T0, R2));
    J[5] = fma(-m, c.y * c.z, dot3(T1, R2));
    const V3 hh{m * c.x, m * c.y, m * c.z};
    const int oi = DL_IC + 10 * i;
    DLW(oi) = m; DLW(oi + 1) = hh.x; DLW(oi + 2) = hh.y; DLW(oi + 3) = hh.z;
#pragma unroll
    for (int k = 0; k < 6; k++) DLW(oi + 4 + k) = J[k];
    SpV F;
    {
        const SpV IA = sp_inertia_mul(m, hh, J, A), IV = sp_inertia_mul(m, hh, J, V);
        const V3 c0 = cross3(V.w, IV.w), c1 = cross3(V.v, IV.v), c2 = cross3(V.w, IV.v);
        F.w = add3(IA.w, add3(c0, c1));
        F.v = add3(IA.v, c2);
    }
    dl_st6<ST>(W, DL_F + 6 * i, F);
}

// RNE backward pass: bias[i] = S_i . F_i, F_parent += F_i (descending i)
template <int ST = 64>
__device__ __forceinline__ void dyn_backward_bias(const DynHdr &dh, double *W, double *bias) {
#pragma unroll
    for (int i = kDynMax - 1; i >= 0; i--) {
        if (i < dh.nd) {
            const SpV S = dl_ld6<ST>(W, DL_S + 6 * i), F = dl_ld6<ST>(W, DL_F + 6 * i);
            bias[i] = spdot(S, F);
            const int pi = dh.parent[i];
            if (pi >= 0) {
                SpV Fp = dl_ld6<ST>(W, DL_F + 6 * pi);
                Fp.w = add3(Fp.w, F.w); Fp.v = add3(Fp.v, F.v);
                dl_st6<ST>(W, DL_F + 6 * pi, Fp);
            }
        } else bias[i] = 0.0;
    }
}

// composite inertias (descending: parent += child)
template <int ST = 64>
__device__ __forceinline__ void dyn_crb_accumulate(const DynHdr &dh, double *W) {
    for (int i = dh.nd - 1; i >= 1; i--) {
        const int pi = dh.parent[i];
        if (pi >= 0) {
#pragma unroll
            for (int k = 0; k < 10; k++) DLW(DL_IC + 10 * pi + k) = DLW(DL_IC + 10 * pi + k) + DLW(DL_IC + 10 * i + k);
        }
    }
}
// rows (bit mask) of the packed lower triangle of M, written over the F columns (dead after the bias pass):
// M[i][i] = S_i . (Ic_i S_i) + armature, M[i][k] = S_k . (Ic_i S_i) for the ancestors k of i, 0 elsewhere
template <int ST = 64>
__device__ __forceinline__ void dyn_crb_rows(const DynHdr &dh, const double *__restrict__ DD, double *W, unsigned rows) {
    for (int i = 0; i < dh.nd; i++) {
        if (!((rows >> i) & 1u)) continue;
        const int row = i * (i + 1) / 2;
        for (int k = 0; k < i; k++) DLW(DL_F + row + k) = 0.0;
        const int oi = DL_IC + 10 * i;
        double J[6];
#pragma unroll
        for (int k = 0; k < 6; k++) J[k] = DLW(oi + 4 + k);
        const SpV S = dl_ld6<ST>(W, DL_S + 6 * i);
        const SpV G = sp_inertia_mul(DLW(oi), V3{DLW(oi + 1), DLW(oi + 2), DLW(oi + 3)}, J, S);
        DLW(DL_F + row + i) = spdot(S, G) + DD[kDynRec * i + DR_ARM];
        for (int k = dh.parent[i]; k >= 0; k = dh.parent[k]) DLW(DL_F + row + k) = spdot(dl_ld6<ST>(W, DL_S + 6 * k), G);
    }
}
// The two backward sweeps with one COMPONENT per lane (the contact kernel): parent += child down the tree is a chain of dependent
// LDS read-modify-writes -- 6 (force) resp. 10 (inertia) of them side by side instead of one after the other; then bias_i =
// S_i . F_i with one body per lane.  Same additions in the same order per component, same dot products: same bits.
template <int ST = 64>
__device__ __forceinline__ void dyn_backward_lanes(const DynHdr &dh, double *W, int l) {
    if (l < 10) {
        for (int i = dh.nd - 1; i >= 1; i--) {
            const int pi = dh.parent[i];
            if (pi >= 0) {
                DLW(DL_IC + 10 * pi + l) = DLW(DL_IC + 10 * pi + l) + DLW(DL_IC + 10 * i + l);
                if (l < 6) DLW(DL_F + 6 * pi + l) = DLW(DL_F + 6 * pi + l) + DLW(DL_F + 6 * i + l);
            }
        }
    }
}
template <int ST = 64>
__device__ __forceinline__ double dyn_bias_of(const double *W, int i) { return spdot(dl_ld6<ST>(W, DL_S + 6 * i), dl_ld6<ST>(W, DL_F + 6 * i)); }

// row i alone (the contact kernel: one row per lane); arm: the dof's armature; par: parent of dof k at par[stride k], as a double
template <int ST = 64>
__device__ __forceinline__ void dyn_crb_row(const double *par, int stride, double arm, double *W, int i) {
    const int row = i * (i + 1) / 2;
    for (int k = 0; k < i; k++) DLW(DL_F + row + k) = 0.0;
    const int oi = DL_IC + 10 * i;
    double J[6];
#pragma unroll
    for (int k = 0; k < 6; k++) J[k] = DLW(oi + 4 + k);
    const SpV S = dl_ld6<ST>(W, DL_S + 6 * i);
    const SpV G = sp_inertia_mul(DLW(oi), V3{DLW(oi + 1), DLW(oi + 2), DLW(oi + 3)}, J, S);
    DLW(DL_F + row + i) = spdot(S, G) + arm;
    for (int k = (int)par[stride * i]; k >= 0; k = (int)par[stride * k]) DLW(DL_F + row + k) = spdot(dl_ld6<ST>(W, DL_S + 6 * k), G);
}
// ... gathered into registers with static indices: A[i (i + 1) / 2 + k]
template <int ST = 64>
__device__ __forceinline__ void dyn_m_gather(const DynHdr &dh, const double *W, double *A) {
    const int nm = dh.nd * (dh.nd + 1) / 2;
#pragma unroll
    for (int k = 0; k < kDynMax * (kDynMax + 1) / 2; k++) A[k] = (k < nm) ? DLW(DL_F + k) : 0.0;
}
template <int ST = 64>
__device__ __forceinline__ void dyn_crb(const DynHdr &dh, const double *__restrict__ DD, double *W, double *A) {
    dyn_crb_accumulate<ST>(dh, W);
    dyn_crb_rows<ST>(dh, DD, W, ~0u);
    dyn_m_gather<ST>(dh, W, A);
}

// in-place L D L^T of the packed lower triangle + solve (registers, fully unrolled; rows beyond n are skipped)
__device__ __forceinline__ void dyn_ldl_solve(int n, double *A, double *x) {
    double dinv[kDynMax];
#pragma unroll
    for (int i = 0; i < kDynMax; i++) {
        if (i < n) {
#pragma unroll
            for (int k = 0; k <= i; k++) {
                double acc = A[i * (i + 1) / 2 + k];
#pragma unroll
                for (int j = 0; j < k; j++) acc = fma(-A[i * (i + 1) / 2 + j], A[k * (k + 1) / 2 + j] * A[j * (j + 1) / 2 + j], acc);
                if (k < i) A[i * (i + 1) / 2 + k] = acc * dinv[k];
                else { A[i * (i + 1) / 2 + i] = acc; dinv[i] = 1.0 / acc; }
            }
        } else dinv[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < kDynMax; i++)
        if (i < n) {
            double acc = x[i];
#pragma unroll
            for (int j = 0; j < i; j++) acc = fma(-A[i * (i + 1) / 2 + j], x[j], acc);
            x[i] = acc;
        }
#pragma unroll
    for (int i = 0; i < kDynMax; i++)
        if (i < n) x[i] = x[i] * dinv[i];
#pragma unroll
    for (int i = kDynMax - 1; i >= 0; i--)
        if (i < n) {
            double acc = x[i];
#pragma unroll
            for (int j = i + 1; j < kDynMax; j++)
                if (j < n) acc = fma(-A[j * (j + 1) / 2 + i], x[j], acc);
            x[i] = acc;
        }
}

// generalised forces, (M + h D) qacc = tau, semi-implicit Euler step, joint stops; the sub-step's bias becomes the lagged one
template <int ST = 64>
// tc_slot >= 0 (the contact kernel): the generalised contact forces J^T f of the dofs at slots tc_slot + i are added to tau
// stops: the joint range as an inelastic stop (false: the limits are rows of the contact kernel's solver)
__device__ __forceinline__ void dyn_solve_integrate(const DynHdr &dh, const double *__restrict__ DD, double *W, const double *bias, double *A,
                                                    int tc_slot = -1, bool stops = true) {
    double tau[kDynMax];
#pragma unroll
    for (int i = 0; i < kDynMax; i++) {
        if (i < dh.nd) {
            const double *rec = DD + kDynRec * i;
            const double q = DLW(DL_Q + i), v = DLW(DL_V + i);
            const double passive = -rec[DR_DAMP] * v;
            const double applied = dh.gravcomp[i] ? DLW(DL_LAG + i) : 0.0;
            double act = 0.0;
            if (dh.actuated[i]) act = clampd(fma(-rec[DR_KP], q, rec[DR_KP] * DLW(DL_CTRL + i)), rec[DR_FLO], rec[DR_FHI]);
            tau[i] = ((passive - bias[i]) + applied) + act;
            if (tc_slot >= 0) tau[i] = tau[i] + DLW(tc_slot + i);
            A[i * (i + 1) / 2 + i] = fma(dh.h, rec[DR_DAMP], A[i * (i + 1) / 2 + i]);
        } else tau[i] = 0.0;
    }
    dyn_ldl_solve(dh.nd, A, tau);
#pragma unroll
    for (int i = 0; i < kDynMax; i++)
        if (i < dh.nd) {
            const double *rec = DD + kDynRec * i;
            double v = fma(dh.h, tau[i], DLW(DL_V + i));
            double q = fma(dh.h, v, DLW(DL_Q + i));
            if (dh.limited[i] && stops) {      // inelastic stop at the joint range
                if (q < rec[DR_LO]) { q = rec[DR_LO]; if (v < 0.0) v = 0.0; }
                else if (q > rec[DR_HI]) { q = rec[DR_HI]; if (v > 0.0) v = 0.0; }
            }
            DLW(DL_V + i) = v;
            DLW(DL_Q + i) = q;
            DLW(DL_LAG + i) = bias[i];
        }
}

// one mj_step of the lane's env (state in the Q / V / LAG / CTRL columns), single-wave form
template <int ST = 64>
__device__ __forceinline__ void dyn_substep(const DynHdr &dh, const double *__restrict__ DD, double *W, const double *__restrict__ OD,
                                            int it, unsigned long long &mine, unsigned long long &any) {
    double bias[kDynMax], A[kDynMax * (kDynMax + 1) / 2];
    ObjPass op{dh.obj_on != 0, false, mine, any};
    if (op.on) {
        op.precull = it % dh.o_every == 0;
        obj_begin(dh, OD, W, op.precull, op.mine, op.any);
    }
    dyn_forward_pass<ST>(dh, DD, W, OD, op);
    if (op.on) {
        obj_integrate(dh, W);
        mine = op.mine; any = op.any;
    }
    dyn_backward_bias<ST>(dh, W, bias);
    dyn_crb<ST>(dh, DD, W, A);
    dyn_solve_integrate<ST>(dh, DD, W, bias, A);
}

// ---- what the dynamics kernels share around the sub-steps: the column load / store (k_env_dyn, k_env_dyn4's wave 0, the contact kernel
// k_env_dyn_ct) and mode 0's command (k_env_dyn, k_env_dyn4; k_env_dyn_ct keeps its own fenced loop around the same env_desired) ----
// env e's Q / V / LAG columns from its qpos row and its rows of qvel / bias_lag (CTRL cleared), and back
template <int ST = 64>
__device__ __forceinline__ void dyn_cols_load(const DynHdr &dh, double *W, long long e, const double *row, const double *qvel, const double *bias_lag) {
    for (int i = 0; i < dh.nd; i++) {
        DLW(DL_Q + i) = row[dh.qadr[i]];
        DLW(DL_V + i) = qvel[e * dh.nv + i];
        DLW(DL_LAG + i) = bias_lag[e * dh.nd + i];
        DLW(DL_CTRL + i) = 0.0;
    }
}
template <int ST = 64>
__device__ __forceinline__ void dyn_cols_store(const DynHdr &dh, const double *W, long long e, double *row, double *qvel, double *bias_lag) {
    for (int i = 0; i < dh.nd; i++) {
        row[dh.qadr[i]] = DLW(DL_Q + i);
        qvel[e * dh.nv + i] = DLW(DL_V + i);
        bias_lag[e * dh.nd + i] = DLW(DL_LAG + i);
    }
}
// mode 0's command -- `_step`: desired_state = prev_state + clip(action [* ac_scale]) (env_desired; the Pusher has its own kernel, K8);
// ctrl = [desired_state, gripper targets], ctrlrange-clamped, into the CTRL column.  prev / has: the env's prev_state row and
// has_prev entry, written where `write` holds (the lanes that stand for the env and may record the command).
template <int ST = 64>
__device__ __forceinline__ void dyn_command(const EnvHdr &h, const DynHdr &dh, const double *__restrict__ GD, double *W, const double *act,
                                            int is_planner, double *prev, unsigned char *has, bool write) {
    const bool use_prev = is_planner && *has;
#pragma unroll 1      // (runs once per env.step; rolled, the sub-step loops behind it compile to the instruction sequence they had)
    for (int i = 0; i < dh.nd; i++) {
        const int k = dh.act_of[i];
        if (k < 0) continue;
        double target;
        if (k < h.n_arm) {
            target = env_desired(h, use_prev ? prev[k] : DLW(DL_Q + i), act[k], is_planner, false);
            if (write) prev[k] = target;      // `self._prev_state = np.copy(desired_state)`
        } else target = DLW(DL_Q + i) + act[h.n_arm];      // Lift: gripper qpos + action[-1]
        DLW(DL_CTRL + i) = clampd(target, GD[h.o_act_lo + k], GD[h.o_act_hi + k]);
    }
    if (write) *has = 1;
}

// mode 0: env.step's physics -- ctrl from the action (the `_step` arithmetic of k_env_step, nothing moved kinematically),
//         prev_state / has_prev updated, dh.nsub sub-steps when the env's move flag is set;
// mode 1: n_steps sub-steps towards the given ctrl rows [E, nd] (tests, parity per sub-step);
// mode 2: mj_forward only: bias_lag <- qfrc_bias(qpos, qvel); M_out (optional) <- packed lower triangle of M [E, nd (nd + 1) / 2].
// (the dynamics header comes through a pointer: by value its ~100 ints sat in SGPRs and 219 of them spilled;
// amdgpu_waves_per_eu(1, 1): LDS allows one wave per CU anyway, so the whole register file is this wave's)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_env_dyn(EnvHdr h, const DynHdr *__restrict__ dhp, const double *__restrict__ GD, const int32_t *__restrict__ GI,
                                                const double *__restrict__ DD, const double *__restrict__ OD, long long E, int mode, int n_steps,
                                                double *__restrict__ qpos, double *__restrict__ qvel, double *__restrict__ bias_lag,
                                                double *__restrict__ prev_state, unsigned char *__restrict__ has_prev,
                                                const double *__restrict__ action, int is_planner,
                                                const unsigned char *__restrict__ move_mask, const double *__restrict__ ctrl_in,
                                                double *__restrict__ M_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ST = 64;
    double *W = reinterpret_cast<double *>(smem) + threadIdx.x;
    const DynHdr &dh = *dhp;
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;      // no barriers below: lanes are independent
    const unsigned flags = move_mask ? move_mask[e] : 1u;
    if (flags & 2u) return;
    double *row = qpos + e * h.nq;
    dyn_cols_load(dh, W, e, row, qvel, bias_lag);
    if (dh.obj_on) {
#pragma unroll
        for (int k = 0; k < 7; k++) DLW(DL_OBJ + k) = row[dh.obj_qadr + k];
#pragma unroll
        for (int k = 0; k < 6; k++) DLW(DL_OBJ + 7 + k) = qvel[e * dh.nv + dh.nd + k];
    }
    if (mode == 0) {
        dyn_command(h, dh, GD, W, action + e * h.adim, is_planner, prev_state + e * h.n_arm, has_prev + e, true);
        if (!(flags & 1u)) return;
        n_steps = dh.nsub;
    } else if (mode == 1) {
        for (int i = 0; i < dh.nd; i++) DLW(DL_CTRL + i) = ctrl_in[e * dh.nd + i];
    } else {
        double bias[kDynMax], A[kDynMax * (kDynMax + 1) / 2];
        ObjPass none{false, false, 0ull, 0ull};
        dyn_forward_pass(dh, DD, W, OD, none);
        dyn_backward_bias(dh, W, bias);
#pragma unroll
        for (int i = 0; i < kDynMax; i++)
            if (i < dh.nd) bias_lag[e * dh.nd + i] = bias[i];
        if (M_out) {
            dyn_crb(dh, DD, W, A);
            const int nm = dh.nd * (dh.nd + 1) / 2;
#pragma unroll
            for (int k = 0; k < kDynMax * (kDynMax + 1) / 2; k++)
                if (k < nm) M_out[e * nm + k] = A[k];
        }
        return;
    }
    unsigned long long mine = 0ull, any = 0ull;      // stage B: collider masks of the last full scan
#pragma unroll 1
    for (int it = 0; it < n_steps; it++) dyn_substep(dh, DD, W, OD, it, mine, any);
    dyn_cols_store(dh, W, e, row, qvel, bias_lag);
    if (dh.obj_on) {
#pragma unroll
        for (int k = 0; k < 7; k++) row[dh.obj_qadr + k] = DLW(DL_OBJ + k);
#pragma unroll
        for (int k = 0; k < 6; k++) qvel[e * dh.nv + dh.nd + k] = DLW(DL_OBJ + 7 + k);
    }
}

// ---- workgroup form: FOUR waves share the 64 envs of a workgroup --------------------------------------------------------
// A lone wave per CU (the LDS columns allow no more) spends a sub-step as ~5.7 k dependent-ish FP64 instructions on ONE
// SIMD while three SIMDs idle.  Here the four SIMDs of the CU work on the same 64 envs: lane l of every wave is env l,
// the LDS columns are shared.  Per sub-step
//   P1  every wave walks the whole chain (pose, S, V, A: serial and cheap), but only the OWNER of a body (own4) derives its
//       inertia about the origin and its force and stores the S / IC / F columns; with stage-B contacts the fourth wave owns
//       no body and evaluates the object's contacts instead (it has every body's pose and velocity at hand)
//   P2  wave 0: RNE backward pass (bias, in its registers);  wave 1: composite inertias;  wave 3: the object's integration
//   P3  every wave: its rows of M (rows4)
//   P4  wave 0: gather M, forces, L D L^T solve, integration, joint stops
// with workgroup barriers between the phases.  Every quantity is produced by the same instruction sequence as in the
// single-wave kernel (and the CPU checker), so results are bit-identical; what changes is who computes it and when.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_env_dyn4(EnvHdr h, const DynHdr *__restrict__ dhp, const double *__restrict__ GD, const int32_t *__restrict__ GI,
                                                const double *__restrict__ DD, const double *__restrict__ OD, long long E, int mode, int n_steps,
                                                double *__restrict__ qpos, double *__restrict__ qvel, double *__restrict__ bias_lag,
                                                double *__restrict__ prev_state, unsigned char *__restrict__ has_prev,
                                                const double *__restrict__ action, int is_planner,
                                                const unsigned char *__restrict__ move_mask, const double *__restrict__ ctrl_in,
                                                double *__restrict__ M_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ST = 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *W = reinterpret_cast<double *>(smem) + lane;
    const DynHdr &dh = *dhp;
    long long e = (long long)blockIdx.x * 64 + lane;
    bool live = e < E;              // lanes past the batch and envs that sit the call out still walk along (barriers), on the
    if (!live) e = E - 1;           // state of a real env, and write nothing back
    const unsigned flags = move_mask ? move_mask[e] : 1u;
    if (flags & 2u) live = false;
    double *row = qpos + e * h.nq;
    const bool obj = dh.obj_on != 0;
    const int w_obj = 3;
    if (wv == 0) {
        dyn_cols_load(dh, W, e, row, qvel, bias_lag);
        if (mode == 0) {
            dyn_command(h, dh, GD, W, action + e * h.adim, is_planner, prev_state + e * h.n_arm, has_prev + e, live);
        } else if (mode == 1) {
            for (int i = 0; i < dh.nd; i++) DLW(DL_CTRL + i) = ctrl_in[e * dh.nd + i];
        }
    }
    if (wv == w_obj && obj) {
#pragma unroll
        for (int k = 0; k < 7; k++) DLW(DL_OBJ + k) = row[dh.obj_qadr + k];
#pragma unroll
        for (int k = 0; k < 6; k++) DLW(DL_OBJ + 7 + k) = qvel[e * dh.nv + dh.nd + k];
    }
    if (mode == 0) {
        if (!(flags & 1u)) live = false;       // the command is recorded, nothing moves
        n_steps = dh.nsub;
    }
    __syncthreads();
    // with the object on, its wave owns no body: the other three share them
    const unsigned own = obj ? (wv == w_obj ? 0u : dh.own4[wv] ) : dh.own4[wv];
    const unsigned rows = dh.rows4[wv];
    double bias[kDynMax], A[kDynMax * (kDynMax + 1) / 2];
    if (mode == 2) {
        ObjPass none{false, false, 0ull, 0ull};
        dyn_forward_pass(dh, DD, W, OD, none, own);
        __syncthreads();
        if (wv == 0) {
            dyn_backward_bias(dh, W, bias);
#pragma unroll
            for (int i = 0; i < kDynMax; i++)
                if (i < dh.nd && live) bias_lag[e * dh.nd + i] = bias[i];
        }
        if (M_out) {            // (kernel argument: uniform over the workgroup)
            if (wv == 1) dyn_crb_accumulate(dh, W);
            __syncthreads();
            dyn_crb_rows(dh, DD, W, rows);
            __syncthreads();
            if (wv == 0) {
                dyn_m_gather(dh, W, A);
                const int nm = dh.nd * (dh.nd + 1) / 2;
#pragma unroll
                for (int k = 0; k < kDynMax * (kDynMax + 1) / 2; k++)
                    if (k < nm && live) M_out[e * nm + k] = A[k];
            }
        }
        return;
    }
    unsigned long long mine = 0ull, any = 0ull;      // stage B: collider masks of the last full scan (the object's wave)
#pragma unroll 1
    for (int it = 0; it < n_steps; it++) {
        ObjPass op{obj && wv == w_obj, false, mine, any};
        if (op.on) {
            op.precull = it % dh.o_every == 0;
            obj_begin(dh, OD, W, op.precull, op.mine, op.any);
        }
        dyn_forward_pass(dh, DD, W, OD, op, own);
        if (op.on) { mine = op.mine; any = op.any; }
        __syncthreads();
        if (wv == 0) dyn_backward_bias(dh, W, bias);
        else if (wv == 1) dyn_crb_accumulate(dh, W);
        else if (op.on) obj_integrate(dh, W);
        __syncthreads();
        dyn_crb_rows(dh, DD, W, rows);
        __syncthreads();
        if (wv == 0) {
            dyn_m_gather(dh, W, A);
            dyn_solve_integrate(dh, DD, W, bias, A);
        }
        __syncthreads();
    }
    if (wv == 0 && live) dyn_cols_store(dh, W, e, row, qvel, bias_lag);
    if (wv == w_obj && obj && live) {
#pragma unroll
        for (int k = 0; k < 7; k++) row[dh.obj_qadr + k] = DLW(DL_OBJ + k);
#pragma unroll
        for (int k = 0; k < 6; k++) qvel[e * dh.nv + dh.nd + k] = DLW(DL_OBJ + 7 + k);
    }
}
#undef DLW

// What attach_dynamics compiles: the header, the per-dof records, the penalty object's [feature points | collider records] (empty:
// no object), the LDS bytes of a launch.
struct DynTables {
    DynHdr hdr{};
    std::vector<double> rec, orec;
    size_t lds = 0;
    bool slot_shared = false;      // a save slot has more than one writer (slots are numbered by saved-ancestor depth)
};
// Host half of attach_dynamics, over the env's header and the host copy of its int table (actuator / joint addresses).  No device.
static int dyn_build_host(const EnvHdr &h, const std::vector<int32_t> &hi, const MopaDynDesc *d, DynTables &T) {
    if (!d) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (d->nd <= 0 || d->nd > kDynMax) return fail(MOPA_ERR_LIMIT, "the dynamics kernel keeps 1 .. 9 dofs per env");
    if (!(d->timestep > 0.0) || d->nsub <= 0) return fail(MOPA_ERR_INVALID_ARG, "timestep / nsub must be positive");
    DynHdr &dh = T.hdr;
    dh = DynHdr{};
    dh.nd = d->nd; dh.nsub = d->nsub; dh.nv = d->nd;
    dh.gx = d->gravity[0]; dh.gy = d->gravity[1]; dh.gz = d->gravity[2]; dh.h = d->timestep;
    std::vector<double> &rec = T.rec, &orec = T.orec;
    rec.assign((size_t)kDynRec * d->nd, 0.0);
    for (int i = 0; i < d->nd; i++) {
        if (d->parent[i] >= i || d->parent[i] < -1) return fail(MOPA_ERR_INVALID_ARG, "dynamic bodies must list parents before children");
        if (d->jtype[i] != J_SLIDE && d->jtype[i] != J_HINGE) return fail(MOPA_ERR_UNSUPPORTED, "hinge / slide dofs only");
        if (d->qadr[i] < 0 || d->qadr[i] >= h.nq) return fail(MOPA_ERR_INVALID_ARG, "qadr out of range");
        if (!(d->mass[i] > 0.0)) return fail(MOPA_ERR_INVALID_ARG, "every dynamic body needs mass");
        dh.parent[i] = d->parent[i]; dh.jtype[i] = d->jtype[i]; dh.qadr[i] = d->qadr[i];
        dh.limited[i] = d->limited[i]; dh.actuated[i] = d->actuated[i]; dh.gravcomp[i] = d->gravcomp[i];
        double *r = &rec[(size_t)kDynRec * i];
        std::memcpy(r + DR_RPOS, d->rel_pos + 3 * i, 24);
        std::memcpy(r + DR_RQUAT, d->rel_quat + 4 * i, 32);
        std::memcpy(r + DR_AXIS, d->axis + 3 * i, 24);
        std::memcpy(r + DR_JPOS, d->jpos + 3 * i, 24);
        r[DR_QREF] = d->qref[i]; r[DR_MASS] = d->mass[i];
        std::memcpy(r + DR_IPOS, d->ipos + 3 * i, 24);
        std::memcpy(r + DR_INERTIA, d->inertia + 6 * i, 48);
        r[DR_DAMP] = d->damping[i]; r[DR_ARM] = d->armature[i]; r[DR_LO] = d->lo[i]; r[DR_HI] = d->hi[i];
        r[DR_KP] = d->kp[i]; r[DR_FLO] = d->force_lo[i]; r[DR_FHI] = d->force_hi[i];
        // the env actuator (ctrl entry) that drives this dof
        dh.act_of[i] = -1;
        for (int k = 0; k < h.n_act; k++)
            if (hi[h.o_act + k] == d->qadr[i]) dh.act_of[i] = k;
        if ((dh.act_of[i] >= 0) != (d->actuated[i] != 0)) return fail(MOPA_ERR_INVALID_ARG, "actuated[] does not match the env's actuator list");
    }
    for (int j = 0; j < 8; j++) dh.arm_dof[j] = -1;
    for (int j = 0; j < 4; j++) dh.grip_dof[j] = -1;
    if (h.n_arm > 8 || h.n_grip > 4) return fail(MOPA_ERR_LIMIT, "too many arm / gripper joints");
    for (int i = 0; i < d->nd; i++) {
        for (int j = 0; j < h.n_arm; j++) if (hi[h.o_arm + j] == d->qadr[i]) dh.arm_dof[j] = i;
        for (int j = 0; j < h.n_grip; j++) if (hi[h.o_grip + j] == d->qadr[i]) dh.grip_dof[j] = i;
    }
    for (int j = 0; j < h.n_arm; j++) if (dh.arm_dof[j] < 0) return fail(MOPA_ERR_INVALID_ARG, "an arm joint is not among the dynamic dofs");
    for (int j = 0; j < h.n_grip; j++) if (dh.grip_dof[j] < 0) return fail(MOPA_ERR_INVALID_ARG, "a gripper joint is not among the dynamic dofs");
    if (const int k = parents_depth_first(d->parent, d->nd); k >= 0)
        return fail(MOPA_ERR_UNSUPPORTED, "bodies are not in depth-first order (body " + std::to_string(k) + ")");
    dh.n_save = save_slot_program(d->parent, d->nd, dh.load, dh.save);
    // A slot with two writers (parent = -1 0 1 1 0 4 4: bodies 1 and 4 both park in slot 1) is safe in a walk that one wave makes.  The
    // workgroup form's four waves each make the whole walk on the SAME columns with no barrier inside it: a wave that is two bodies
    // ahead would overwrite the slot before a slower one has reloaded it.  Such a tree is launched in the single-wave form.
    {
        unsigned written = 0u;
        for (int i = 0; i < d->nd; i++)
            if (dh.save[i] >= 0) {
                if (written & (1u << dh.save[i])) T.slot_shared = true;
                written |= 1u << dh.save[i];
            }
    }
    // workgroup form: bodies round-robin over the waves that own bodies (three with the object on, four without);
    // rows of M by descending length to the least loaded wave (row i has depth(i) + 1 entries)
    {
        const int n_own = d->obj ? 3 : 4;
        for (int w = 0; w < 4; w++) { dh.own4[w] = 0u; dh.rows4[w] = 0u; }
        for (int i = 0; i < d->nd; i++) dh.own4[i % n_own] |= 1u << i;
        std::vector<int> len(d->nd, 1), order(d->nd), load(4, 0);
        for (int i = 0; i < d->nd; i++) {
            for (int k = d->parent[i]; k >= 0; k = d->parent[k]) len[i]++;
            order[i] = i;
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
        for (int i : order) {
            int w = 0;
            for (int c = 1; c < 4; c++) if (load[c] < load[w]) w = c;
            dh.rows4[w] |= 1u << i;
            load[w] += len[i];
        }
    }
    T.lds = (size_t)(DL_SAVE + kDynSaveStride * dh.n_save) * 64 * sizeof(double);
    if (T.lds > (size_t)kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "dynamic tree too branchy for the LDS layout");
    if (d->obj) {
        const MopaObjDesc &o = *d->obj;
        if (o.nfeat != kObjFeat || o.ncol < 0) return fail(MOPA_ERR_INVALID_ARG, "a box object comes with its 26 feature points (8 vertices, 12 edge midpoints, 6 face centres)");
        if (o.qadr < 0 || o.qadr + 7 > h.nq) return fail(MOPA_ERR_INVALID_ARG, "object qadr out of range");
        if (!(o.mass > 0.0) || !(o.inertia[0] > 0.0) || !(o.inertia[1] > 0.0) || !(o.inertia[2] > 0.0)) return fail(MOPA_ERR_INVALID_ARG, "object inertial must be positive");
        dh.obj_on = 1; dh.obj_qadr = o.qadr; dh.obj_nfeat = o.nfeat; dh.obj_ncol = o.ncol; dh.nv = d->nd + 6;
        dh.o_mass = o.mass; dh.o_in0 = o.inertia[0]; dh.o_in1 = o.inertia[1]; dh.o_in2 = o.inertia[2]; dh.o_damp = o.damping;
        dh.o_h0 = o.half[0]; dh.o_h1 = o.half[1]; dh.o_h2 = o.half[2]; dh.o_rbound = o.rbound;
        dh.o_kn = o.kn; dh.o_dn = o.dn; dh.o_eps2 = o.eps_v * o.eps_v; dh.o_ctmax = o.ct_max;
        dh.o_imass = o.inv_mass; dh.o_iin0 = o.inv_inertia[0]; dh.o_iin1 = o.inv_inertia[1]; dh.o_iin2 = o.inv_inertia[2];
        dh.o_margin = o.precull_margin; dh.o_every = o.precull_every;
        if (o.precull_every < 1 || !(o.precull_margin >= 0.0) || o.ncol > 64) return fail(MOPA_ERR_INVALID_ARG, "bad precull parameters (or more than 64 colliders)");
        int prev = -1, at = 0;
        for (int b = -1; b <= d->nd; b++) dh.co_first[b + 1] = 0;
        for (int c = 0; c < o.ncol; c++) {
            const int b = o.co_body[c];
            if (b < prev || b >= d->nd) return fail(MOPA_ERR_INVALID_ARG, "colliders must be sorted: static ones (-1), then by dynamic body");
            prev = b;
        }
        for (int b = -1; b < d->nd; b++) {
            dh.co_first[b + 1] = at;
            while (at < o.ncol && o.co_body[at] == b) at++;
        }
        dh.co_first[d->nd + 1] = at;
        orec.assign(o.feat, o.feat + 3 * (size_t)o.nfeat);
        for (int c = 0; c < o.ncol; c++) {
            double r[kObjRec];
            r[0] = (double)o.co_type[c];
            std::memcpy(r + 1, o.co_size + 3 * c, 24);
            std::memcpy(r + 4, o.co_pos + 3 * c, 24);
            std::memcpy(r + 7, o.co_mat + 9 * c, 72);
            r[16] = o.co_mu[c]; r[17] = o.co_rbound[c];
            orec.insert(orec.end(), r, r + kObjRec);
        }
    }
    return MOPA_OK;
}

extern "C" int mopa_env_attach_dynamics(MopaEnv *env, const MopaDynDesc *d) {
    if (!env || !d) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    DynTables T;
    if (const int rc = dyn_build_host(env->hdr, env->h_int, d, T)) return rc;
    DeviceGuard guard(env->device);
    if (!guard.ok()) return fail(MOPA_ERR_HIP, "hipSetDevice failed");
    // everything is allocated and uploaded into locals; env changes only once nothing can fail any more
    double *od = nullptr, *dd = nullptr;
    DynHdr *nh = nullptr;
    auto drop = [&](const char *what) {
        for (void *q : {(void *)od, (void *)dd, (void *)nh})
            if (q) (void)hipFree(q);
        return fail(MOPA_ERR_HIP, what);
    };
    if (!T.orec.empty() && upload_array(T.orec.data(), T.orec.size(), &od) != hipSuccess) return drop("upload of the object table failed");
    if (upload_array(T.rec.data(), T.rec.size(), &dd) != hipSuccess) return drop("upload of the dynamics table failed");
    if (!env->d_dynhdr && hipMalloc((void **)&nh, sizeof(DynHdr)) != hipSuccess) return drop("allocation of the dynamics header failed");
    if (hipMemcpy(nh ? nh : env->d_dynhdr, &T.hdr, sizeof(DynHdr), hipMemcpyHostToDevice) != hipSuccess) return drop("upload of the dynamics header failed");
    {
        std::lock_guard<std::mutex> lock(env->mu);
        if (od && env->d_obj) env->retired.push_back(env->d_obj);
        if (env->d_dyn) env->retired.push_back(env->d_dyn);
    }
    if (od) env->d_obj = od;
    env->d_dyn = dd;
    if (nh) env->d_dynhdr = nh;
    env->dyn = T.hdr;
    env->dyn_lds = T.lds;
    env->dyn_slot_shared = T.slot_shared;
    for (const void *k : {(const void *)k_env_dyn, (const void *)k_env_dyn4})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    return MOPA_OK;
}

// The host halves of mopa_env_create + mopa_env_attach_dynamics alone: status, and for accepted descriptions the fingerprint of what
// attach_dynamics would upload (header, dof records, object table) with the dynamic tree's save-slot count.  DynHdr ends in padding:
// its fields are contiguous up to rows4 (asserted), and the hash stops there.
static_assert(offsetof(DynHdr, gx) == offsetof(DynHdr, grip_dof) + 4 * sizeof(int) && offsetof(DynHdr, obj_on) == offsetof(DynHdr, h) + sizeof(double) &&
                  offsetof(DynHdr, o_mass) == offsetof(DynHdr, co_first) + (kDynMax + 2) * sizeof(int) &&
                  offsetof(DynHdr, o_every) == offsetof(DynHdr, o_margin) + sizeof(double) && offsetof(DynHdr, own4) == offsetof(DynHdr, o_every) + sizeof(int) &&
                  offsetof(DynHdr, rows4) == offsetof(DynHdr, own4) + 4 * sizeof(unsigned),
              "DynHdr has padding between its fields: mopa_dyn_tables_host would hash indeterminate bytes");
extern "C" int mopa_dyn_tables_host(const MopaEnvDesc *env_desc, const MopaDynDesc *d, uint64_t *fingerprint, int32_t *n_save) {
    MopaEnv S;
    BlobPacker B;
    if (const int rc = env_build_host(env_desc, S, B)) return rc;
    DynTables T;
    if (const int rc = dyn_build_host(S.hdr, S.h_int, d, T)) return rc;
    Fnv f;
    f.add(&T.hdr, offsetof(DynHdr, rows4) + sizeof(T.hdr.rows4));
    f.add(T.rec);
    f.add(T.orec);
    if (fingerprint) *fingerprint = f.f;
    if (n_save) *n_save = T.hdr.n_save;
    return MOPA_OK;
}

extern "C" int mopa_env_dyn_dofs(const MopaEnv *env) { return (env && env->d_dyn) ? env->dyn.nd : -1; }
extern "C" int mopa_env_dyn_qvel_width(const MopaEnv *env) { return (env && env->d_dyn) ? env->dyn.nv : -1; }
// The form a servo-dynamics launch of this env takes: the workgroup form (four waves share 64 envs) unless the tree has a save slot with
// two writers or MOPA_DYN_KERNEL=wave pins the single-wave form (A/B runs, tests).
static bool dyn_workgroup_form(const MopaEnv *env) {
    const char *force = getenv("MOPA_DYN_KERNEL");
    return !env->dyn_slot_shared && !(force && std::strcmp(force, "wave") == 0);
}
extern "C" int mopa_env_dyn_waves(const MopaEnv *env) { return (env && env->d_dyn) ? (dyn_workgroup_form(env) ? 4 : 1) : -1; }

static int env_ct_launch(MopaEnv *env, int64_t E, int mode, int n_steps, double *qpos, double *qvel, double *bias_lag, double *prev_state,
                         uint8_t *has_prev, const double *action, int is_planner, const uint8_t *move_mask, const double *ctrl, hipStream_t st);
static int env_dyn_launch(MopaEnv *env, int64_t E, int mode, int n_steps, double *qpos, double *qvel, double *bias_lag, double *prev_state,
                          uint8_t *has_prev, const double *action, int is_planner, const uint8_t *move_mask, const double *ctrl,
                          double *M_out, hipStream_t st) {
    if (env->ct_on && mode != 2)      // stage C: the sub-steps run in the contact kernel (mopa_contact.inc); mj_forward stays here
        return env_ct_launch(env, E, mode, n_steps, qpos, qvel, bias_lag, prev_state, has_prev, action, is_planner, move_mask, ctrl, st);
    const unsigned blocks = (unsigned)((E + 63) / 64);
    // default: the workgroup form; the single-wave form (one wave per 64 envs) for a tree with a shared save slot, or pinned
    const bool wg = dyn_workgroup_form(env);
    auto kern = wg ? k_env_dyn4 : k_env_dyn;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(wg ? 256 : 64), env->dyn_lds, st, env->hdr, env->d_dynhdr, env->d_dbl, env->d_int, env->d_dyn, env->d_obj,
                       (long long)E, mode, n_steps, qpos, qvel, bias_lag, prev_state, has_prev, action, is_planner, move_mask, ctrl, M_out);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_env_dyn_forward_batch(MopaEnv *env, int64_t E, const double *qpos_dev, const double *qvel_dev, double *bias_dev,
                                          double *M_dev, const uint8_t *mask_dev, void *stream) {
    if (!env || !env->d_dyn) return fail(MOPA_ERR_INVALID_ARG, "env without dynamics (mopa_env_attach_dynamics)");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !qvel_dev || !bias_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(env->device);
    return env_dyn_launch(env, E, 2, 0, const_cast<double *>(qpos_dev), const_cast<double *>(qvel_dev), bias_dev, nullptr, nullptr, nullptr, 0,
                          mask_dev, nullptr, M_dev, (hipStream_t)stream);
}

extern "C" int mopa_env_dyn_substeps_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *bias_lag_dev,
                                           const double *ctrl_dev, int32_t n, void *stream) {
    if (!env || !env->d_dyn) return fail(MOPA_ERR_INVALID_ARG, "env without dynamics (mopa_env_attach_dynamics)");
    if (E < 0 || n < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E / n");
    if (E == 0 || n == 0) return MOPA_OK;
    if (!qpos_dev || !qvel_dev || !bias_lag_dev || !ctrl_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(env->device);
    return env_dyn_launch(env, E, 1, n, qpos_dev, qvel_dev, bias_lag_dev, nullptr, nullptr, nullptr, 0, nullptr, ctrl_dev, nullptr,
                          (hipStream_t)stream);
}

extern "C" int mopa_env_step_dyn_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *qvel_dev, double *bias_lag_dev,
                                       double *prev_state_dev, uint8_t *has_prev_dev, int32_t *ep_len_dev, const double *action_dev,
                                       int32_t is_planner, const uint8_t *move_mask_dev, double *obs_dev, double *reward_dev,
                                       uint8_t *done_dev, uint8_t *success_dev, void *stream) {
    if (!env || !env->d_dyn) return fail(MOPA_ERR_INVALID_ARG, "env without dynamics (mopa_env_attach_dynamics)");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !qvel_dev || !bias_lag_dev || !obs_dev) return fail(MOPA_ERR_INVALID_ARG, "null qpos / qvel / bias_lag / obs buffer");
    if (action_dev && (!prev_state_dev || !has_prev_dev || !ep_len_dev || !reward_dev || !done_dev || !success_dev))
        return fail(MOPA_ERR_INVALID_ARG, "a stepping call needs prev_state, has_prev, ep_len, reward, done and success buffers");
    ON_DEVICE(env->device);
    hipStream_t st = (hipStream_t)stream;
    if (action_dev) {
        const int rc = env_dyn_launch(env, E, 0, 0, qpos_dev, qvel_dev, bias_lag_dev, prev_state_dev, has_prev_dev, action_dev, (int)is_planner,
                                      move_mask_dev, nullptr, nullptr, st);
        if (rc != MOPA_OK) return rc;
    }
    return env_step_launch(env, E, qpos_dev, prev_state_dev, has_prev_dev, ep_len_dev, action_dev, (int)is_planner, move_mask_dev, obs_dev,
                           reward_dev, done_dev, success_dev, qvel_dev, st);
}
