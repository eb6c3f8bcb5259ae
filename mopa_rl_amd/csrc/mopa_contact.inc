// mopa_contact.inc -- K7: `mj_step` WITH CONTACTS inside env.step (SURVEY.md 8 f4b, stage C).
// (included by mopa_envdyn.hip after mopa_dyn.inc; C ABI in include/mopa_hip.h "mopa_env_attach_contacts")
//
// What it restates: per sub-step of the reference's `_do_simulation` loop (env/sawyer/sawyer_push_obstacle.py:186-203,
// sawyer_lift_obstacle.py:218-236, sawyer_assembly_obstacle.py:121-139; options sawyer_dependencies.xml:11) the [3P] MuJoCo
// pipeline with contacts: smooth dynamics of the arm (K6's routines, unchanged), the manipulated object as a free rigid
// body, contact generation between arm / object / scene, MuJoCo's soft-constraint model (solref / solimp impedance,
// reference acceleration, regulariser), the XML's ELLIPTIC friction cones in the Newton solver (SOLVER 2, the default: MuJoCo's
// primal elliptic-cone cost; pyramidal cones with Newton -- SOLVER 1 -- or projected Gauss-Seidel -- SOLVER 0 -- stay selectable)
// with the XML's iteration cap and tolerance, the noslip pass, joint limits as solver rows, two-way coupling, Euler integration
// with implicit joint damping.  RESTATED FROM THE PUBLISHED SOLVER, PARITY UNPINNED (no MuJoCo here); not restated: torsional /
// rolling friction (condim 4 / 6 pairs are solved as condim 3).
// The arithmetic, in this order, is the specification the CPU checker under tests restates; tests compare every sub-step
// bit for bit.
//
// Mapping: SIXTEEN LANES per env, four envs per wave, one wave per workgroup (4096 envs = 1024 workgroups: every SIMD of
// the chip holds one wave; K6's lane-per-env form fills 64 of 256 CUs at that batch).
//   * smooth dynamics: the 16 lanes of an env run K6's routines redundantly (same values in every lane, the per-body
//     columns in LDS at stride 4 = one column per env of the wave) -- the chain walk is serial whichever way it is mapped;
//   * contact detection: one FEATURE POINT per lane (16 per trip) against the signed-distance function of the pair's other
//     shape, hits compacted in feature order by a ballot over the group (same order as the sequential checker);
//   * constraint rows: one DOF per lane (9 arm dofs + 6 of the object): Jacobian entries are lane-local; dot products over
//     the dofs are a fixed 4-step butterfly over the group (the checker sums the same tree); M^-1 J^T: one right-hand side
//     per lane against the L D L^T factor every lane holds in registers;
//   * projected Gauss-Seidel: per contact three dot products (J_n, J_t1, J_t2 with the running qacc), the four pyramid rows
//     updated through the contact's local 3x3 Gram matrix on every lane alike, qacc updated dof-per-lane.
// LDS per env: K6's columns (272 doubles) + body poses (63) + pair mask + maxcon x 108 doubles of contact rows: 9.7 KB at
// maxcon = 8, so four waves (16 envs) share a CU.

constexpr int kCtRec = 108;          // LDS slots (doubles) per contact
constexpr int kCtDc = 12;            // the wave's LDS copy of what the lane-parallel phases read per dof: mass, ipos 3, inertia 6, armature, parent
// slots of a contact record
constexpr int CT_J = 0;              // [3][16] Jacobian rows n, t1, t2 over the dofs
constexpr int CT_B = 48;             // [3][9]  M^-1 J^T, arm dofs (the object's are J / M, formed on the fly)
constexpr int CT_G = 76, CT_MU = 82, CT_R = 83, CT_INVD = 87, CT_AREF = 91, CT_F = 95, CT_D = 99, CT_KEY = 103;
constexpr int CT_FS = 104;           // [4] the pyramid forces after the noslip pass (what acts; CT_F warm-starts the next solve)
// detection scratch (overlays the J rows until they are formed)
constexpr int CT_DIST = 0, CT_POS = 1, CT_NRM = 4, CT_IDS = 7;
constexpr int kCtFtRec = 4, kCtPrRec = 54, kCtPar = 12;
constexpr double kCtMinMu = 1e-5;    // [3P] mjMINMU
// pair record (self-contained: one level of dependent loads per pair): sf, ss, par 12 (mu, margin, K, B, d0, dmax, width, -, condim, torsional
// friction, rolling friction, -),
// body of F, body of S, type of S, bounding radius of F, centre of F 3 and of S 3 (body frames), mat of S 9, size of S 3,
// first feature of F, feature count of F; for the reverse bound: type of F, size of F 3, mat of F 9, bounding radius of S
constexpr int PR_PAR = 2, PR_BF = 14, PR_BS = 15, PR_TYPE = 16, PR_RBF = 17, PR_PF = 18, PR_PS = 21, PR_MS = 24, PR_SZ = 33, PR_F0 = 36, PR_NF = 37,
              PR_TYPEF = 38, PR_SZF = 39, PR_MF = 42, PR_RBS = 51;

struct CtHdr {
    int ns, nf, np, maxcon, maxpair, iterations, every, warmstart, obj_qadr, nwords, noslip_iters, limit_rows, near_every, near_slot;
    int xp_slot, mask_slot, hot_slot, con_slot, qv_slot;      // LDS slot offsets (doubles, per env)
    int tab_slot, arena;                            // solver 2: the contact table (16 words) and the slots the variable-size records share
    int env_slots;                                  // slots of one env: the wave's copy of the dof records lies behind 4 of them
    unsigned anc[kDynMax];                          // bit k: dof k is body b itself or one of its ancestors
    double o_mass, o_in0, o_in1, o_in2, o_ipx, o_ipy, o_ipz, o_iqw, o_iqx, o_iqy, o_iqz, o_damp;
    double o_imass, o_iin0, o_iin1, o_iin2, o_imass_d, o_iin0_d, o_iin1_d, o_iin2_d;
    double tol, inv_scale, margin_pre, noslip_tol, lim_par[8], margin_near;
    CfOut cf;                                       // contact-force readout (mopa_env_set_contact_force rewrites it in place); cf.force == nullptr: off
};

#define DLW(slot) W[(size_t)(slot) * ST]

__device__ __forceinline__ void ct_fence() {
    // one wave per workgroup: LDS operations of a wave complete in program order; this only stops the compiler moving them
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// sum over the 16 lanes of a group, as the fixed tree ((p0+p8)+(p4+p12)) + ... of the checker's dot16 (every lane gets it).
// A group is a DPP row: four rotations within the row (v_mov_b32_dpp row_ror on both halves) instead of LDS-crossbar shuffles.
template <int N>
__device__ __forceinline__ double ct_ror(double x) {
    // (every lane of a row has a source lane under a rotation: no `old` value to preserve, bound_ctrl spares its initialisation)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), 0x120 + N, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), 0x120 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ct_sum16(double p) {
    p = p + ct_ror<8>(p);
    p = p + ct_ror<4>(p);
    p = p + ct_ror<2>(p);
    p = p + ct_ror<1>(p);
    return p;
}
// position of the n-th (0-based) set bit of x; n < popcount(x)
__device__ __forceinline__ int ct_nth_bit(unsigned long long x, int n) {
    int pos = 0;
    unsigned lo = (unsigned)x;
    int c = __popc(lo);
    if (n >= c) { n -= c; pos = 32; lo = (unsigned)(x >> 32); }
    c = __popc(lo & 0xffffu); if (n >= c) { n -= c; pos += 16; lo >>= 16; }
    lo &= 0xffffu;
    c = __popc(lo & 0xffu); if (n >= c) { n -= c; pos += 8; lo >>= 8; }
    lo &= 0xffu;
    c = __popc(lo & 0xfu); if (n >= c) { n -= c; pos += 4; lo >>= 4; }
    lo &= 0xfu;
    c = __popc(lo & 0x3u); if (n >= c) { n -= c; pos += 2; lo >>= 2; }
    if (n >= (int)(lo & 1u)) pos += 1;
    return pos;
}

// signed distance of point y (shape frame) to the shape's surface; WANT_N: and the outward unit normal there (the normal's
// divisions are only paid for features that turn out to be contacts: ct_sdf<false> first, ct_sdf<true> for the hits --
// the same expressions either way)
template <bool WANT_N>
__device__ __forceinline__ void ct_sdf(int type, double s0, double s1, double s2, V3 y, double &dist, V3 &nl) {
    if (type == G_PLANE) {
        dist = y.z;
        if (WANT_N) nl = V3{0.0, 0.0, 1.0};
        return;
    }
    if (type == G_SPHERE || type == G_CAPSULE) {
        V3 c{0.0, 0.0, 0.0};
        if (type == G_CAPSULE) c.z = clampd(y.z, -s1, s1);
        const V3 dv = sub3(y, c);
        const double d = sqrt(dot3(dv, dv));
        dist = d - s0;
        if (WANT_N) {
            if (d > 0.0) nl = V3{dv.x / d, dv.y / d, dv.z / d};
            else nl = V3{0.0, 0.0, 1.0};
        }
        return;
    }
    if (type == G_CYLINDER) {
        const double rho = sqrt(fma(y.y, y.y, y.x * y.x));
        const double dr = rho - s0, dz = fabs(y.z) - s1;
        if (dr > 0.0 && dz > 0.0) {
            const double d = sqrt(fma(dz, dz, dr * dr));
            dist = d;
            if (WANT_N) {
                const double sz = (y.z < 0.0) ? -1.0 : 1.0;
                double rx = 0.0, ry = 0.0;
                if (rho > 0.0) { rx = y.x / rho; ry = y.y / rho; }
                nl = V3{(dr * rx) / d, (dr * ry) / d, (dz * sz) / d};
            }
        } else if (dr > dz && rho > 0.0) {
            dist = dr;
            if (WANT_N) nl = V3{y.x / rho, y.y / rho, 0.0};
        } else {
            dist = dz;
            if (WANT_N) nl = V3{0.0, 0.0, (y.z < 0.0) ? -1.0 : 1.0};
        }
        return;
    }
    {
        const V3 q{clampd(y.x, -s0, s0), clampd(y.y, -s1, s1), clampd(y.z, -s2, s2)};
        const V3 dv = sub3(y, q);
        const double dd = dot3(dv, dv);
        if (dd > 0.0) {
            const double d = sqrt(dd);
            dist = d;
            if (WANT_N) nl = V3{dv.x / d, dv.y / d, dv.z / d};
            return;
        }
        const double d0 = s0 - fabs(y.x), d1 = s1 - fabs(y.y), d2 = s2 - fabs(y.z);
        int a = 0;
        double dm = d0;
        if (d1 < dm) { dm = d1; a = 1; }
        if (d2 < dm) { dm = d2; a = 2; }
        dist = -dm;
        if (WANT_N) {
            nl = V3{0.0, 0.0, 0.0};
            if (a == 0) nl.x = (y.x < 0.0) ? -1.0 : 1.0;
            else if (a == 1) nl.y = (y.y < 0.0) ? -1.0 : 1.0;
            else nl.z = (y.z < 0.0) ? -1.0 : 1.0;
        }
    }
}

// the manipulated object's state and frames (the same values on every lane of the env's group)
struct CtObj {
    V3 p; Q4 q; V3 v, w;          // body frame pose (qpos), velocity of the COM and angular velocity in the world (qvel)
    double omat[9]; V3 c; double RD[9];
};
__device__ __forceinline__ void ct_obj_frames(const CtHdr &ch, CtObj &o) {
    quat2mat(o.omat, o.q);
    o.c = add3(o.p, mat_vec(o.omat, V3{ch.o_ipx, ch.o_ipy, ch.o_ipz}));
    const Q4 qD = quat_mul(o.q, Q4{ch.o_iqw, ch.o_iqx, ch.o_iqy, ch.o_iqz});
    quat2mat(o.RD, qD);
}

// world pose of body b (0 .. nd-1: arm, from the pose slots; nd: the object)
template <int ST>
__device__ __forceinline__ void ct_body_pose(const double *W, int xp_slot, int nd, const CtObj &o, int b, V3 &bp, double *bR) {
    if (b == nd) {
        bp = o.p;
#pragma unroll
        for (int k = 0; k < 9; k++) bR[k] = o.omat[k];
    } else {
        const int s = xp_slot + 7 * b;
        bp = V3{DLW(s), DLW(s + 1), DLW(s + 2)};
        quat2mat(bR, Q4{DLW(s + 3), DLW(s + 4), DLW(s + 5), DLW(s + 6)});
    }
}
// world pose of the pair's shape S (position, rotation) from its record
template <int ST>
__device__ __forceinline__ void ct_pose_s(const double *W, int xp_slot, int nd, const CtObj &o, const double *__restrict__ pr, V3 &pg, double *Rg) {
    const int bs = (int)pr[PR_BS];
    if (bs < 0) {
        pg = ld3(pr + PR_PS);
#pragma unroll
        for (int k = 0; k < 9; k++) Rg[k] = pr[PR_MS + k];
    } else {
        V3 bp;
        double bR[9];
        ct_body_pose<ST>(W, xp_slot, nd, o, bs, bp, bR);
        pg = add3(bp, mat_vec(bR, ld3(pr + PR_PS)));
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++)
                Rg[3 * r + cc] = dot3(ld3(bR + 3 * r), V3{pr[PR_MS + cc], pr[PR_MS + 3 + cc], pr[PR_MS + 6 + cc]});
    }
}
// Lower bound of (signed distance - radius) over every feature of the pair's shape F against its shape S: the distance
// function of S is 1-Lipschitz and every feature (with its radius) lies within F's bounding radius of F's centre.
template <int ST>
__device__ __forceinline__ double ct_pair_bound(const double *W, int xp_slot, int nd, const CtObj &o, const double *__restrict__ pr) {
    const int bf = (int)pr[PR_BF];
    V3 cf = ld3(pr + PR_PF);
    if (bf >= 0) {
        V3 bp;
        double bR[9];
        ct_body_pose<ST>(W, xp_slot, nd, o, bf, bp, bR);
        cf = add3(bp, mat_vec(bR, cf));
    }
    V3 pg;
    double Rg[9];
    ct_pose_s<ST>(W, xp_slot, nd, o, pr, pg, Rg);
    double dist;
    V3 nl;
    ct_sdf<false>((int)pr[PR_TYPE], pr[PR_SZ], pr[PR_SZ + 1], pr[PR_SZ + 2], matT_vec(Rg, sub3(cf, pg)), dist, nl);
    return dist - pr[PR_RBF];
}
// The reverse bound: a contact of the pair also puts the CENTRE OF S within (margin + S's bounding radius) of F's surface
// (the feature's sphere lies in F, the point of S nearest the feature is within margin + radius of it and within S's bounding
// radius of S's centre; F's distance function is 1-Lipschitz).  Kernel-side only, per sub-step: it keeps pairs like
// (vertices of the 0.4 m roof plate, a finger) out of the narrow phase unless the finger really is at the plate.
template <int ST>
__device__ __forceinline__ double ct_pair_bound_rev(const double *W, int xp_slot, int nd, const CtObj &o, const double *__restrict__ pr) {
    const int bs = (int)pr[PR_BS], bf = (int)pr[PR_BF];
    V3 cs = ld3(pr + PR_PS);
    if (bs >= 0) {
        V3 bp;
        double bR[9];
        ct_body_pose<ST>(W, xp_slot, nd, o, bs, bp, bR);
        cs = add3(bp, mat_vec(bR, cs));
    }
    V3 pf = ld3(pr + PR_PF);
    double Rf[9];
    if (bf < 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) Rf[k] = pr[PR_MF + k];
    } else {
        V3 bp;
        double bR[9];
        ct_body_pose<ST>(W, xp_slot, nd, o, bf, bp, bR);
        pf = add3(bp, mat_vec(bR, pf));
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++)
                Rf[3 * r + cc] = dot3(ld3(bR + 3 * r), V3{pr[PR_MF + cc], pr[PR_MF + 3 + cc], pr[PR_MF + 6 + cc]});
    }
    double dist;
    V3 nl;
    ct_sdf<false>((int)pr[PR_TYPEF], pr[PR_SZF], pr[PR_SZF + 1], pr[PR_SZF + 2], matT_vec(Rf, sub3(cs, pf)), dist, nl);
    return dist - pr[PR_RBS];
}

// A pair record into registers in ONE batch of loads: the records live in global memory (L2: ~300 clocks a read, tools/ubench/lone_wave.hip),
// and read field by field -- behind the branches of the bound / pose routines -- a lone wave paid that latency a dozen times per pair.
template <int K0, int K1>
__device__ __forceinline__ void ct_pair_load(const double *__restrict__ pr, double (&t)[kCtPrRec]) {
    const double *p = static_cast<const double *>(__builtin_assume_aligned(pr, 16));
#pragma unroll
    for (int k = K0; k < K1; k++) t[k] = p[k];
#pragma unroll
    for (int k = K0; k < K1; k++) asm volatile("" : "+v"(t[k]));       // (all of them issued before the first is used)
}
constexpr int kCtPrHead = 38;       // the slots the forward bound, the narrow phase's poses and the feature range read (the rest: the reverse bound)

// in-place L D L^T of the packed lower triangle in registers (same arithmetic as dyn_ldl_solve), dinv = 1 / D
__device__ __forceinline__ void ct_ldl_factor(int n, double *A, double *dinv) {
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
}
__device__ __forceinline__ void ct_ldl_apply(int n, const double *A, const double *dinv, double *x) {
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

__device__ __forceinline__ double ct_impedance(const double *__restrict__ par, double dist) {
    const double x = fabs(dist - par[1]) / par[6];
    double y;
    if (x >= 1.0) y = 1.0;
    else if (x <= 0.5) y = 2.0 * (x * x);
    else y = 1.0 - 2.0 * ((1.0 - x) * (1.0 - x));
    return fma(y, par[5] - par[4], par[4]);
}

// value k of a register array selected by a lane-varying index (static indices only: no scratch)
__device__ __forceinline__ double ct_pick9(const double *x, int k) {
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < kDynMax; i++) r = (k == i) ? x[i] : r;
    return r;
}

struct CtCounters { int contacts, sweeps, dropped, maxc; };

// what one Gauss-Seidel visit of a contact reads: this lane's entries of the three Jacobian rows and of M^-1 J^T, the local
// Gram matrix, friction, and per pyramid row force / regulariser / 1 / (A + R) / (A + R) / reference acceleration
struct CtVisit { double Jn, J1, J2, Bn, B1, B2, G[6], mu, f[4], R[4], iD[4], D[4], ar[4]; };
template <int ST>
__device__ __forceinline__ void ct_visit_load(const double *W, int con_slot, int c, int l, int nd, double invM_l, CtVisit &v) {
    const int s = con_slot + kCtRec * c;
    v.Jn = DLW(s + CT_J + l); v.J1 = DLW(s + CT_J + 16 + l); v.J2 = DLW(s + CT_J + 32 + l);
    if (l < nd) { v.Bn = DLW(s + CT_B + l); v.B1 = DLW(s + CT_B + 9 + l); v.B2 = DLW(s + CT_B + 18 + l); }
    else { v.Bn = v.Jn * invM_l; v.B1 = v.J1 * invM_l; v.B2 = v.J2 * invM_l; }
#pragma unroll
    for (int k = 0; k < 6; k++) v.G[k] = DLW(s + CT_G + k);
    v.mu = DLW(s + CT_MU);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        v.f[i] = DLW(s + CT_F + i); v.R[i] = DLW(s + CT_R + i); v.iD[i] = DLW(s + CT_INVD + i); v.D[i] = DLW(s + CT_D + i); v.ar[i] = DLW(s + CT_AREF + i);
    }
}
// one Gauss-Seidel visit of the contact at record slot s: the four pyramid rows in turn (branch-free: a row whose force does
// not move adds exact zeros), the forces back to the record, this lane's dof of qacc; returns the cost improvement (>= 0)
template <int ST>
__device__ __forceinline__ double ct_visit(double *W, int s, CtVisit &v, double &qacc_l) {
    double un = ct_sum16(v.Jn * qacc_l), u1 = ct_sum16(v.J1 * qacc_l), u2 = ct_sum16(v.J2 * qacc_l);
    double Dn = 0.0, D1 = 0.0, D2 = 0.0, ic = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double sm = (i & 1) ? -v.mu : v.mu;
        const double ut = (i < 2) ? u1 : u2;
        const double ci = fma(v.R[i], v.f[i], -v.ar[i]);
        const double res = fma(sm, ut, un) + ci;
        double fn = fma(-res, v.iD[i], v.f[i]);
        if (fn < 0.0) fn = 0.0;
        const double df = fn - v.f[i];
        v.f[i] = fn;
        const double Gnt = (i < 2) ? v.G[1] : v.G[2], G1t = (i < 2) ? v.G[3] : v.G[4], G2t = (i < 2) ? v.G[4] : v.G[5];
        un = fma(fma(sm, Gnt, v.G[0]), df, un);
        u1 = fma(fma(sm, G1t, v.G[1]), df, u1);
        u2 = fma(fma(sm, G2t, v.G[2]), df, u2);
        Dn = Dn + df;
        if (i < 2) D1 = fma(sm, df, D1); else D2 = fma(sm, df, D2);
        ic = ic - df * fma(0.5 * df, v.D[i], res);
    }
    DLW(s + CT_F) = v.f[0]; DLW(s + CT_F + 1) = v.f[1]; DLW(s + CT_F + 2) = v.f[2]; DLW(s + CT_F + 3) = v.f[3];
    qacc_l = fma(v.B2, D2, fma(v.B1, D1, fma(v.Bn, Dn, qacc_l)));
    return ic;
}
#ifdef MOPA_CT_PROF
// -DMOPA_CT_PROF: s_memtime ticks (100 MHz) per phase of group 0 of every wave, summed into g_ct_prof[0..7] (tools/ct_bench.py prints them)
__device__ unsigned long long g_ct_prof[32];
#define CT_TICK(k) do { const unsigned long long _t = __builtin_readcyclecounter(); if (threadIdx.x == 0) atomicAdd(&g_ct_prof[k], _t - _t0); _t0 = __builtin_readcyclecounter(); } while (0)
#define CT_TICK0() unsigned long long _t0 = __builtin_readcyclecounter()
extern "C" int mopa_debug_ct_prof(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ct_prof), 256) != hipSuccess) return -1;
    if (reset) { unsigned long long z[32] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_ct_prof), z, 256); }
    return 0;
}
#else
#define CT_TICK(k)
#define CT_TICK0()
#endif

// ---- the Newton solver (MuJoCo's default; oracle ct_newton, same arithmetic) ------------------------------------------------------
// dof l on lane l of the env's 16; constraint row r (contact r / 4, pyramid edge r % 4) on lane r % 16 -- at most 32 rows (maxcon 8).
// M v of the env's joint-space inertia (packed rows at DL_F) and the object's diagonal: v passes through the LDS scratch `vs`
template <int ST>
__device__ __forceinline__ double ct_mul_M(double *W, int l, int nd, int vs, double v_l, double objM_l) {
    ct_fence();
    DLW(vs + l) = v_l;
    ct_fence();
    double acc = 0.0;
    if (l < nd) {
        for (int k = 0; k < nd; k++) {
            const int a = (k <= l) ? l : k, b = (k <= l) ? k : l;
            acc = fma(DLW(DL_F + a * (a + 1) / 2 + b), DLW(vs + k), acc);
        }
    } else acc = objM_l * v_l;
    return acc;
}
__device__ __forceinline__ double ct_rowsum(double ta, double tb, bool has_a, bool has_b) {
    double acc = has_a ? ta : 0.0;
    if (has_b) acc = acc + tb;
    return ct_sum16(acc);
}
constexpr int kCtLsEvals = 8;
template <int ST>
// lside / laref / lD: the joint-limit row of this lane's dof (side +-1, 0 = none; x = side q - aref; weight D): gradient entry, Hessian
// diagonal and its own term of the row sums, all lane-local; limf_l <- its generalised force
__device__ __forceinline__ int ct_newton(const CtHdr &ch, double *W, int l, int nd, int ncon, bool arm_touch, double a0_l, double objM_l, double &qacc_l,
                                         double lside, double laref, double lD, double &limf_l) {
    const int nv = (ch.obj_qadr >= 0) ? nd + 6 : nd;
    const int ts = ch.qv_slot, vs = ch.qv_slot + 48;       // LDS scratch over the (consumed) composite-inertia columns: T 3 x 16 | vector 16
    const int c0 = l >> 2, ri = l & 3;                     // this lane's rows: edge ri of contacts c0 and c0 + 4
    const bool has_a = c0 < ncon, has_b = c0 + 4 < ncon;
    double DrA = 0.0, DrB = 0.0, smA = 0.0, smB = 0.0;
    if (has_a) {
        const int s = ch.con_slot + kCtRec * c0;
        DrA = DLW(s + CT_INVD + ri); smA = (ri & 1) ? -DLW(s + CT_MU) : DLW(s + CT_MU);
    }
    if (has_b) {
        const int s = ch.con_slot + kCtRec * (c0 + 4);
        DrB = DLW(s + CT_INVD + ri); smB = (ri & 1) ? -DLW(s + CT_MU) : DLW(s + CT_MU);
    }
    const double diag_l = (l < nd) ? 0.0 : ((l < nv) ? objM_l : 1.0);
    bool run = true;
    int iters = 0;
    CT_TICK0();
#pragma unroll 1
    for (int it = 0; it < ch.iterations; it++) {
        if (!__any(run)) break;
        if (run) {
            iters++;
            const double dq_l = qacc_l - a0_l;
            const double Mg_l = ct_mul_M<ST>(W, l, nd, vs, dq_l, objM_l);
            double g_l = Mg_l;
            const double gauss = 0.5 * ct_sum16(dq_l * Mg_l);
            double H[15];
#pragma unroll
            for (int k = 0; k < 15; k++) {
                double h = (k == l) ? diag_l : 0.0;
                if (l < nd && k < nd) { const int a = (k <= l) ? l : k, b = (k <= l) ? k : l; h = DLW(DL_F + a * (a + 1) / 2 + b); }
                H[k] = h;
            }
            double xA = 0.0, xB = 0.0, t3A = 0.0, t3B = 0.0;
#pragma unroll 1
            for (int c = 0; c < ncon; c++) {
                const int s = ch.con_slot + kCtRec * c;
                const double J0 = DLW(s + CT_J + l), J1 = DLW(s + CT_J + 16 + l), J2 = DLW(s + CT_J + 32 + l);
                const double un = ct_sum16(J0 * qacc_l), u1 = ct_sum16(J1 * qacc_l), u2 = ct_sum16(J2 * qacc_l);
                const double mu = DLW(s + CT_MU);
                double fr[4], Da[4], xi[4], t3[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double sm = (i & 1) ? -mu : mu;
                    xi[i] = fma(sm, (i < 2) ? u1 : u2, un) - DLW(s + CT_AREF + i);
                    Da[i] = (xi[i] < 0.0) ? DLW(s + CT_INVD + i) : 0.0;
                    fr[i] = -(Da[i] * xi[i]);
                    t3[i] = (0.5 * Da[i] * xi[i]) * xi[i];
                }
                const double Fn = (fr[0] + fr[1]) + (fr[2] + fr[3]), F1 = mu * (fr[0] - fr[1]), F2 = mu * (fr[2] - fr[3]);
                g_l = g_l - fma(J2, F2, fma(J1, F1, J0 * Fn));
                const double mu2 = mu * mu;
                const double Wnn = (Da[0] + Da[1]) + (Da[2] + Da[3]), Wn1 = mu * (Da[0] - Da[1]), Wn2 = mu * (Da[2] - Da[3]);
                const double W11 = mu2 * (Da[0] + Da[1]), W22 = mu2 * (Da[2] + Da[3]);
                ct_fence();
                DLW(ts + l) = fma(Wn2, J2, fma(Wn1, J1, Wnn * J0));
                DLW(ts + 16 + l) = fma(W11, J1, Wn1 * J0);
                DLW(ts + 32 + l) = fma(W22, J2, Wn2 * J0);
                ct_fence();
                // (a contact that moves no arm dof -- object on the scene -- has zero rows / columns there, one that does not move the object
                //  zero ones there: adding them would change nothing, so a block is skipped when no env of the wave needs it)
                const bool nz = J0 != 0.0 || J1 != 0.0 || J2 != 0.0;
                if (__any(nz && l < kDynMax)) {
#pragma unroll
                    for (int k = 0; k < kDynMax; k++)
                        if (k <= l) H[k] = fma(J2, DLW(ts + 32 + k), fma(J1, DLW(ts + 16 + k), fma(J0, DLW(ts + k), H[k])));
                }
                if (__any(nz && l >= kDynMax)) {
#pragma unroll
                    for (int k = kDynMax; k < 15; k++)
                        if (k <= l) H[k] = fma(J2, DLW(ts + 32 + k), fma(J1, DLW(ts + 16 + k), fma(J0, DLW(ts + k), H[k])));
                }
                if ((c & 3) == c0) {
                    const double xo = (ri == 0) ? xi[0] : ((ri == 1) ? xi[1] : ((ri == 2) ? xi[2] : xi[3]));
                    const double to = (ri == 0) ? t3[0] : ((ri == 1) ? t3[1] : ((ri == 2) ? t3[2] : t3[3]));
                    if (c < 4) { xA = xo; t3A = to; } else { xB = xo; t3B = to; }
                }
            }
            const double xl = lside * qacc_l - laref;
            {
                const double w = (lD > 0.0 && xl < 0.0) ? lD : 0.0;
                g_l = g_l - lside * (-(w * xl));
#pragma unroll
                for (int k = 0; k < 15; k++)
                    if (k == l) H[k] = H[k] + w;
            }
            const double p0 = (gauss + ct_rowsum(t3A, t3B, has_a, has_b)) + ct_sum16(((lD > 0.0 && xl < 0.0) ? (0.5 * lD * xl) * xl : (0.5 * 0.0 * xl) * xl));
            CT_TICK(12);
            // L D L^T, right-looking: row l in this lane's registers (entries k < l), the finished columns' entries L[k > l][l] in H[k > l].
            // Column j passes through the LDS scratch unscaled (one write, every lane reads the pivot and the entries it needs).
            // An env none of whose contacts touches the arm has no coupling between the arm's block (= M) and the object's, a zero
            // gradient on the arm's dofs and so a zero direction there: its arm columns change nothing and are skipped -- when no env
            // of the wave needs them (the oracle runs them: same numbers).
            const int jw = __any(arm_touch) ? 0 : nd;
            double mydinv = 1.0;
#pragma unroll
            for (int j = 0; j < 15; j++) {
                if (j >= jw) {
                    const double u = H[j];
                    ct_fence();
                    DLW(vs + l) = u;
                    ct_fence();
                    const double dinv = 1.0 / DLW(vs + j);
                    if (l == j) mydinv = dinv;
#pragma unroll
                    for (int k = j + 1; k < 15; k++) {
                        const double Lk = DLW(vs + k) * dinv;
                        if (l >= k) H[k] = fma(-u, Lk, H[k]);
                        if (l == j) H[k] = Lk;
                    }
                    if (l > j) H[j] = u * dinv;
                }
            }
            double dir_l = -g_l;
#pragma unroll
            for (int j = 0; j < 14; j++) {
                if (j >= jw) {
                    const double bj = __shfl(dir_l, j, 16);
                    if (l > j) dir_l = fma(-H[j], bj, dir_l);
                }
            }
            dir_l = dir_l * mydinv;
#pragma unroll
            for (int k = 14; k >= 1; k--) {
                if (k >= jw) {
                    const double bk = __shfl(dir_l, k, 16);
                    if (l < k) dir_l = fma(-H[k], bk, dir_l);
                }
            }
            CT_TICK(13);
            const double Md_l = ct_mul_M<ST>(W, l, nd, vs, dir_l, objM_l);
            const double qa = ct_sum16(dir_l * Md_l), qb = ct_sum16(dir_l * Mg_l), slope0 = ct_sum16(dir_l * g_l);
            double jdA = 0.0, jdB = 0.0;
#pragma unroll 1
            for (int c = 0; c < ncon; c++) {
                const int s = ch.con_slot + kCtRec * c;
                const double jn = ct_sum16(DLW(s + CT_J + l) * dir_l), j1 = ct_sum16(DLW(s + CT_J + 16 + l) * dir_l),
                             j2 = ct_sum16(DLW(s + CT_J + 32 + l) * dir_l);
                if ((c & 3) == c0) {
                    const double jt = (ri < 2) ? j1 : j2;
                    if (c < 4) jdA = fma(smA, jt, jn); else jdB = fma(smB, jt, jn);
                }
            }
            const double jl = lside * dir_l;
            // safeguarded Newton on p'(alpha), first trial the full step
            double alpha = 1.0, lo = 0.0, hi = -1.0, pa = p0;
            bool ls = true, exact = false;       // exact: the full step accepted at once, no row changed sides -- the minimiser of this piece
#pragma unroll 1
            for (int e = 0; e < kCtLsEvals; e++) {
                if (!__any(ls)) break;
                if (ls) {
                    const double xrA = fma(alpha, jdA, xA), xrB = fma(alpha, jdB, xB);
                    const double wA = (xrA < 0.0) ? DrA : 0.0, wB = (xrB < 0.0) ? DrB : 0.0;
                    const double xrl = fma(alpha, jl, xl);
                    const double wl = (lD > 0.0 && xrl < 0.0) ? lD : 0.0;
                    const double d1 = (fma(alpha, qa, qb) + ct_rowsum((wA * xrA) * jdA, (wB * xrB) * jdB, has_a, has_b)) + ct_sum16((wl * xrl) * jl);
                    const double d2 = (qa + ct_rowsum((wA * jdA) * jdA, (wB * jdB) * jdB, has_a, has_b)) + ct_sum16((wl * jl) * jl);
                    pa = (fma(alpha, fma(0.5 * alpha, qa, qb), gauss) + ct_rowsum((0.5 * wA * xrA) * xrA, (0.5 * wB * xrB) * xrB, has_a, has_b)) +
                         ct_sum16((0.5 * wl * xrl) * xrl);
                    if (fabs(d1) <= 1e-9 * fabs(slope0) || e == kCtLsEvals - 1) {
                        ls = false;
                        if (e == 0 && fabs(d1) <= 1e-9 * fabs(slope0)) {
                            const bool chg = (has_a && ((xA < 0.0) != (xrA < 0.0))) || (has_b && ((xB < 0.0) != (xrB < 0.0))) ||
                                             (lD > 0.0 && ((xl < 0.0) != (xrl < 0.0)));
                            exact = ((__ballot(chg) >> (16 * (threadIdx.x >> 4))) & 0xffffull) == 0ull;
                        }
                    } else {
                        if (d1 < 0.0) lo = alpha; else hi = alpha;
                        double an = alpha - d1 / d2;
                        if (an <= lo || (hi >= 0.0 && an >= hi)) an = (hi >= 0.0) ? 0.5 * (lo + hi) : 2.0 * alpha;
                        alpha = an;
                    }
                }
            }
            qacc_l = fma(alpha, dir_l, qacc_l);
            if ((p0 - pa) * ch.inv_scale < ch.tol || exact) run = false;
            CT_TICK(14);
        }
    }
    // the constraint forces at the solution
    for (int c = 0; c < ncon; c++) {
        const int s = ch.con_slot + kCtRec * c;
        const double un = ct_sum16(DLW(s + CT_J + l) * qacc_l), u1 = ct_sum16(DLW(s + CT_J + 16 + l) * qacc_l), u2 = ct_sum16(DLW(s + CT_J + 32 + l) * qacc_l);
        if (l < 4) {
            const double mu = DLW(s + CT_MU);
            const double xi = fma((l & 1) ? -mu : mu, (l < 2) ? u1 : u2, un) - DLW(s + CT_AREF + l);
            DLW(s + CT_F + l) = (xi < 0.0) ? -(DLW(s + CT_INVD + l) * xi) : 0.0;
        }
    }
    {
        const double x = lside * qacc_l - laref;
        limf_l = (lD > 0.0 && x < 0.0) ? lside * (-(lD * x)) : 0.0;
    }
    ct_fence();
    CT_TICK(15);
    return iters;
}

// The front half of a sub-step, shared by the solver forms: the arm's smooth dynamics (bias <- qfrc_bias, M packed over the F columns, body
// poses in the pose slots), the object's frames, and the three culling levels -- on return the HOT pairs' bits stand in the hot words.
template <int ST>
__device__ __forceinline__ void ct_front(const DynHdr &dh, const CtHdr &ch, const double *__restrict__ DD, const double *__restrict__ PR, const double *DC,
                                         double *W, int l, int it, CtObj &o, double (&bias)[kDynMax]) {
    const int nd = dh.nd;
    CT_TICK0();
    // ---- smooth dynamics of the arm: K6's routines, every lane of the group alike
    {
        // the serial walk on every lane alike (pose, S, V, A per body) ...
        ObjPass none{false, false, 0ull, 0ull};
        dyn_forward_pass<ST, false, true>(dh, DD, W, nullptr, none, ~0u, ch.xp_slot);
        ct_fence();
        CT_TICK(8);
        // ... each body's inertia about the origin and force on a lane of its own (dof records from the wave's LDS copy) ...
        DynOwnerIn oin;
        if (l < nd) oin = dyn_forward_owner_load<ST>(W, ch.xp_slot, l);
        ct_fence();
        if (l < nd) dyn_forward_owner_store<ST>(DC[kCtDc * l], ld3(DC + kCtDc * l + 1), DC + kCtDc * l + 4, W, l, oin);
        ct_fence();
        CT_TICK(9);
        // ... the two backward sweeps one COMPONENT per lane, the bias forces one body per lane (parked in the 9 slots the packed
        // M leaves free at the end of the F columns; every lane needs all of them for the generalised forces) ...
        dyn_backward_lanes<ST>(dh, W, l);
        ct_fence();
        double b_l = 0.0;
        if (l < nd) b_l = dyn_bias_of<ST>(W, l);
        ct_fence();
        if (l < nd) DLW(DL_F + 45 + l) = b_l;
        ct_fence();
#pragma unroll
        for (int i = 0; i < kDynMax; i++) bias[i] = (i < nd) ? DLW(DL_F + 45 + i) : 0.0;
        CT_TICK(10);
        // ... and the rows of M one per lane
        if (l < nd) dyn_crb_row<ST>(DC + 11, kCtDc, DC[kCtDc * l + 10], W, l);      // packed lower triangle of M over the F columns; the IC columns are free from here
        CT_TICK(11);
    }
    ct_obj_frames(ch, o);
    ct_fence();
    CT_TICK(0);
    // ---- pair culling, one PAIR per lane (16 per trip).  For the pair's shapes F, S the signed distance of F's centre in S, less
    // F's bounding radius, bounds every feature's (distance - radius) from below.  Pass 0 (every `every`-th sub-step, over all
    // pairs): pairs whose bound is below margin + precull margin stay ACTIVE for the next `every` sub-steps (`mask` words).
    // Pass 1 (every sub-step, over the active pairs): pairs whose bound is below the margin are HOT (`hot` words) -- only these
    // enter the narrow phase.  The checker applies the same bounds pair by pair.  One loop serves both passes (the kernel's
    // code has to stay inside the instruction cache: every wave of the CU walks all of it once per sub-step).
    // Three levels: pass 0 (every `every`-th sub-step) all pairs -> ACTIVE (`mask` words, within margin + precull margin); pass 1 (every
    // `near_every`-th) the active ones -> NEAR (within margin + near margin); pass 2 (every sub-step) the near ones -> HOT (within the
    // margin, and -- kernel only -- by the reverse bound too).  The hot words live in the scratch over the consumed inertia columns.
    for (int pass = (it % ch.every == 0) ? 0 : ((it % ch.near_every == 0) ? 1 : 2); pass < 3; pass++) {
        const int dst = pass == 0 ? ch.mask_slot : (pass == 1 ? ch.near_slot : ch.hot_slot);
        const int src = pass == 1 ? ch.mask_slot : ch.near_slot;
        const double extra = pass == 0 ? ch.margin_pre : (pass == 1 ? ch.margin_near : 0.0);
        const bool last = pass == 2;
        for (int w = l; w < ch.nwords; w += 16) DLW(dst + w) = __longlong_as_double(0ll);
        ct_fence();
        // the set bits of ALL source words are one list: a trip serves 16 pairs whichever words they sit in (ten near pairs spread
        // over four words are one trip, not four)
        int K = ch.np;
        if (pass != 0) {
            K = 0;
            for (int w = 0; w < ch.nwords; w++) K += __popcll((unsigned long long)__double_as_longlong(DLW(src + w)));
        }
        for (int base = 0; base < K; base += 16) {
            int rem = base + l;
            CT_TICK(25);
            if (rem < K) {
                int w, pos;
                if (pass == 0) { w = rem >> 6; pos = rem & 63; }
                else {
                    unsigned long long bits = 0ull;
                    for (w = 0; w < ch.nwords; w++) {
                        bits = (unsigned long long)__double_as_longlong(DLW(src + w));
                        const int k = __popcll(bits);
                        if (rem < k) break;
                        rem -= k;
                    }
                    pos = ct_nth_bit(bits, rem);
                }
                CT_TICK(16);
                double pr[kCtPrRec];
                const double *prg = PR + (size_t)kCtPrRec * (w * 64 + pos);
                ct_pair_load<0, kCtPrHead>(prg, pr);
                CT_TICK(17);
                bool pass_ = ct_pair_bound<ST>(W, ch.xp_slot, nd, o, pr) < pr[PR_PAR + 1] + extra;
                CT_TICK(18);
                if (pass_ && last && (int)pr[PR_TYPE] != G_PLANE) {
                    ct_pair_load<kCtPrHead, kCtPrRec>(prg, pr);
                    pass_ = ct_pair_bound_rev<ST>(W, ch.xp_slot, nd, o, pr) < pr[PR_PAR + 1];
                }
                CT_TICK(19);
                if (pass_)
                    atomicOr(reinterpret_cast<unsigned long long *>(&DLW(dst + w)), 1ull << pos);
            }
#ifdef MOPA_CT_PROF
            if (threadIdx.x == 0) atomicAdd(&g_ct_prof[20], 1ull);
#endif
        }
        ct_fence();
        if (pass == 0) { CT_TICK(1); }
    }
    CT_TICK(2);
}

// Euler step of the manipulated object (free body; angular velocity in its principal frame) under its smooth forces and the contact forces
// the constraint stage left in the tc slots (qv + 32 + nd ...)
template <int ST>
__device__ __forceinline__ void ct_obj_integrate(const DynHdr &dh, const CtHdr &ch, const double *W, int qv, CtObj &o, const V3 &wb, const V3 &Fo, const V3 &Tb) {
    const int nd = dh.nd;
    if (ch.obj_qadr >= 0) {
        const double h = dh.h;
        const V3 tlin{DLW(qv + 32 + nd), DLW(qv + 32 + nd + 1), DLW(qv + 32 + nd + 2)}, trot{DLW(qv + 32 + nd + 3), DLW(qv + 32 + nd + 4), DLW(qv + 32 + nd + 5)};
        o.v = V3{fma(h, (Fo.x + tlin.x) * ch.o_imass_d, o.v.x), fma(h, (Fo.y + tlin.y) * ch.o_imass_d, o.v.y), fma(h, (Fo.z + tlin.z) * ch.o_imass_d, o.v.z)};
        const V3 wb2{fma(h, (Tb.x + trot.x) * ch.o_iin0_d, wb.x), fma(h, (Tb.y + trot.y) * ch.o_iin1_d, wb.y), fma(h, (Tb.z + trot.z) * ch.o_iin2_d, wb.z)};
        const V3 w = mat_vec(o.RD, wb2);
        o.w = w;
        const V3 cn{fma(h, o.v.x, o.c.x), fma(h, o.v.y, o.c.y), fma(h, o.v.z, o.c.z)};
        const double hh = 0.5 * h;
        double q0 = o.q.w, q1 = o.q.x, q2 = o.q.y, q3 = o.q.z;
        const double dq0 = -(fma(w.z, q3, fma(w.y, q2, w.x * q1)));
        const double dq1 = fma(w.y, q3, fma(-w.z, q2, w.x * q0));
        const double dq2 = fma(w.z, q1, fma(-w.x, q3, w.y * q0));
        const double dq3 = fma(w.x, q2, fma(-w.y, q1, w.z * q0));
        q0 = fma(hh, dq0, q0); q1 = fma(hh, dq1, q1); q2 = fma(hh, dq2, q2); q3 = fma(hh, dq3, q3);
        const double qi = 1.0 / sqrt(fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0))));
        o.q = Q4{q0 * qi, q1 * qi, q2 * qi, q3 * qi};
        double R2[9];
        quat2mat(R2, o.q);
        o.p = sub3(cn, mat_vec(R2, V3{ch.o_ipx, ch.o_ipy, ch.o_ipz}));
    }
}

#include "mopa_contact_ell.inc"      // solver 2: elliptic cones of the pairs' condim (the XML's model)

// One mj_step of the env owned by this 16-lane group.  W: the env's LDS column (stride ST = 4), l: lane within the group,
// grp: group within the wave.  `it`: sub-step index within the call (the pair mask is rebuilt when it % every == 0).
template <int ST, int SOLVER>
__device__ __forceinline__ void ct_substep(const DynHdr &dh, const CtHdr &ch, const double *__restrict__ DD, const double *__restrict__ FT,
                                           const double *__restrict__ PR, const double *DC, double *W, int l, int grp, int it,
                                           CtObj &o, int &nwarm, CtCounters &cnt) {
    const int nd = dh.nd;
    double bias[kDynMax];
    ct_front<ST>(dh, ch, DD, PR, DC, W, l, it, o, bias);
    CT_TICK0();
    // Level 2, the hot pairs in order, one FEATURE per lane; first `maxpair` hits of a pair, `maxcon` in total
    int ncon = 0;
    bool arm_touch = false;
    for (int w = 0; w < ch.nwords; w++) {
        unsigned long long bits = (unsigned long long)__double_as_longlong(DLW(ch.hot_slot + w));
        while (bits) {
            const int p = w * 64 + __builtin_ctzll(bits);
            bits &= bits - 1ull;
            double pr[kCtPrRec];
            ct_pair_load<0, kCtPrHead>(PR + (size_t)kCtPrRec * p, pr);
            const double margin = pr[PR_PAR + 1];
            const int type = (int)pr[PR_TYPE];
            const int bs = (int)pr[PR_BS], bf = (int)pr[PR_BF];
            const double sz0 = pr[PR_SZ], sz1 = pr[PR_SZ + 1], sz2 = pr[PR_SZ + 2];
            // world pose of the shape whose distance function is evaluated, and of the body that carries the features
            V3 pg;
            double Rg[9];
            ct_pose_s<ST>(W, ch.xp_slot, nd, o, pr, pg, Rg);
            V3 fp{0.0, 0.0, 0.0};
            double fR[9];
            if (bf >= 0) ct_body_pose<ST>(W, ch.xp_slot, nd, o, bf, fp, fR);
            const int f0 = (int)pr[PR_F0], nfe = (int)pr[PR_NF];
            int npair = 0;
            for (int k0 = 0; k0 < nfe; k0 += 16) {
                const int k = f0 + k0 + l;
                bool hit = false;
                double dist = 0.0, rad = 0.0;
                V3 x{0.0, 0.0, 0.0}, y{0.0, 0.0, 0.0};
                if (k0 + l < nfe) {
                    const double *ft = FT + (size_t)kCtFtRec * k;
                    rad = ft[3];
                    if (bf >= 0) x = add3(fp, mat_vec(fR, ld3(ft)));
                    else x = ld3(ft);
                    V3 unused;
                    y = matT_vec(Rg, sub3(x, pg));
                    ct_sdf<false>(type, sz0, sz1, sz2, y, dist, unused);
                    dist = dist - rad;
                    hit = dist < margin;
                }
                const unsigned gb = (unsigned)((__ballot(hit) >> (16 * grp)) & 0xffffull);
                if (gb) {
                    const int before = __popc(gb & ((1u << l) - 1u)), total = __popc(gb);
                    int allowed = ch.maxpair - npair;
                    if (ch.maxcon - ncon < allowed) allowed = ch.maxcon - ncon;
                    if (allowed < 0) allowed = 0;
                    if (hit && before < allowed) {
                        const int s = ch.con_slot + kCtRec * (ncon + before);
                        V3 nl;
                        double d2;
                        ct_sdf<true>(type, sz0, sz1, sz2, y, d2, nl);
                        const V3 n = mat_vec(Rg, nl);
                        const V3 pos = addscl3(x, n, -fma(0.5, dist, rad));
                        DLW(s + CT_DIST) = dist;
                        DLW(s + CT_POS) = pos.x; DLW(s + CT_POS + 1) = pos.y; DLW(s + CT_POS + 2) = pos.z;
                        DLW(s + CT_NRM) = n.x; DLW(s + CT_NRM + 1) = n.y; DLW(s + CT_NRM + 2) = n.z;
                        const long long ids = (long long)p | ((long long)k << 16) | ((long long)(bf + 1) << 32) | ((long long)(bs + 1) << 40);
                        DLW(s + CT_IDS) = __longlong_as_double(ids);
                    }
                    const int taken = total < allowed ? total : allowed;
                    ncon += taken; npair += taken;
                    cnt.dropped += total - taken;
                    if (taken > 0 && ((bf >= 0 && bf < nd) || (bs >= 0 && bs < nd))) arm_touch = true;
                }
            }
        }
    }
    ct_fence();
    CT_TICK(7);
    // ---- constraint stage
    const int qv = ch.qv_slot;      // vel 16 | qacc 16 | tc 16 (over the IC columns)
    double tc_l = 0.0;
    const V3 wb = matT_vec(o.RD, o.w);
    V3 Fo{0.0, 0.0, 0.0}, Tb{0.0, 0.0, 0.0};
    {
        Fo = V3{fma(ch.o_mass, dh.gx, -(ch.o_damp * o.v.x)), fma(ch.o_mass, dh.gy, -(ch.o_damp * o.v.y)), fma(ch.o_mass, dh.gz, -(ch.o_damp * o.v.z))};
        const V3 Iw{ch.o_in0 * wb.x, ch.o_in1 * wb.y, ch.o_in2 * wb.z};
        const V3 g = cross3(wb, Iw);
        Tb = V3{-(ch.o_damp * wb.x) - g.x, -(ch.o_damp * wb.y) - g.y, -(ch.o_damp * wb.z) - g.z};
    }
    // joint limits as constraint rows (oracle orc_ct_step): the row of dof l on lane l
    double lside = 0.0, laref = 0.0, lD = 0.0, limf_l = 0.0;
    if (ch.limit_rows && l < nd && dh.limited[l]) {
        const double *rec = DD + kDynRec * l;
        const double q = DLW(DL_Q + l);
        const double dlo = q - rec[DR_LO], dhi = rec[DR_HI] - q;
        double dist = 0.0;
        if (dlo < 0.0) { lside = 1.0; dist = dlo; } else if (dhi < 0.0) { lside = -1.0; dist = dhi; }
        if (lside != 0.0) {
            const double imp = ct_impedance(ch.lim_par, dist);
            double Ri = ((1.0 - imp) / imp) * (1.0 / DLW(DL_F + l * (l + 1) / 2 + l));
            if (Ri < kMinVal) Ri = kMinVal;
            laref = fma(-ch.lim_par[3], lside * DLW(DL_V + l), -((ch.lim_par[2] * imp) * dist));
            lD = 1.0 / Ri;
        }
    }
    const bool lim_any = ((__ballot(lside != 0.0) >> (16 * grp)) & 0xffffull) != 0ull;
    if (lim_any) arm_touch = true;
    if (ncon > 0 || lim_any) {
        // this lane's dof: velocity, inverse inertia of the object's dofs
        double vel_l = 0.0, invM_l = 0.0, qacc_l = 0.0;
        if (l < nd) vel_l = DLW(DL_V + l);
        else if (l == nd) { vel_l = o.v.x; invM_l = ch.o_imass; qacc_l = Fo.x * ch.o_imass; }
        else if (l == nd + 1) { vel_l = o.v.y; invM_l = ch.o_imass; qacc_l = Fo.y * ch.o_imass; }
        else if (l == nd + 2) { vel_l = o.v.z; invM_l = ch.o_imass; qacc_l = Fo.z * ch.o_imass; }
        else if (l == nd + 3) { vel_l = wb.x; invM_l = ch.o_iin0; qacc_l = Tb.x * ch.o_iin0; }
        else if (l == nd + 4) { vel_l = wb.y; invM_l = ch.o_iin1; qacc_l = Tb.y * ch.o_iin1; }
        else if (l == nd + 5) { vel_l = wb.z; invM_l = ch.o_iin2; qacc_l = Tb.z * ch.o_iin2; }
        double A2[kDynMax * (kDynMax + 1) / 2], dinv[kDynMax];
        if (arm_touch) {       // M^-1 without the implicit damping: factor, qacc_smooth of the arm
            double tau[kDynMax];
            dyn_m_gather<ST>(dh, W, A2);
            ct_ldl_factor(nd, A2, dinv);
#pragma unroll
            for (int i = 0; i < kDynMax; i++) {
                if (i < nd) {
                    const double *rec = DD + kDynRec * i;
                    const double q = DLW(DL_Q + i), v = DLW(DL_V + i);
                    const double passive = -rec[DR_DAMP] * v;
                    const double applied = dh.gravcomp[i] ? DLW(DL_LAG + i) : 0.0;
                    double act = 0.0;
                    if (dh.actuated[i]) act = clampd(fma(-rec[DR_KP], q, rec[DR_KP] * DLW(DL_CTRL + i)), rec[DR_FLO], rec[DR_FHI]);
                    tau[i] = ((passive - bias[i]) + applied) + act;
                } else tau[i] = 0.0;
            }
            ct_ldl_apply(nd, A2, dinv, tau);
            if (l < nd) qacc_l = ct_pick9(tau, l);
        }
        // old forces for the warm start: lane c keeps contact c's key and pyramid forces of the previous sub-step
        long long okey = -1;
        double of0 = 0.0, of1 = 0.0, of2 = 0.0, of3 = 0.0;
        if (ch.warmstart && l < nwarm) {
            const int s = ch.con_slot + kCtRec * l;
            okey = __double_as_longlong(DLW(s + CT_KEY));
            of0 = DLW(s + CT_F); of1 = DLW(s + CT_F + 1); of2 = DLW(s + CT_F + 2); of3 = DLW(s + CT_F + 3);
        }
        ct_fence();
        const double a0_l = qacc_l;       // the unconstrained acceleration of this lane's dof (Newton: the Gauss term's centre)
        // Jacobian rows (one dof per lane)
        for (int c = 0; c < ncon; c++) {
            const int s = ch.con_slot + kCtRec * c;
            const V3 pos{DLW(s + CT_POS), DLW(s + CT_POS + 1), DLW(s + CT_POS + 2)};
            const V3 n{DLW(s + CT_NRM), DLW(s + CT_NRM + 1), DLW(s + CT_NRM + 2)};
            const double dist = DLW(s + CT_DIST);
            const long long ids = __double_as_longlong(DLW(s + CT_IDS));
            const int bf = (int)((ids >> 32) & 0xff) - 1, bs = (int)((ids >> 40) & 0xff) - 1;
            V3 e{1.0, 0.0, 0.0};
            if (!(fabs(n.x) < 0.5)) e = V3{0.0, 1.0, 0.0};
            V3 t1 = addscl3(e, n, -dot3(n, e));
            const double tn = sqrt(dot3(t1, t1));
            t1 = V3{t1.x / tn, t1.y / tn, t1.z / tn};
            const V3 t2 = cross3(n, t1);
            double j0 = 0.0, j1 = 0.0, j2 = 0.0;
            if (l < nd) {
                const int inF = (bf >= 0 && bf < nd) ? (int)((ch.anc[bf] >> l) & 1u) : 0;
                const int inS = (bs >= 0 && bs < nd) ? (int)((ch.anc[bs] >> l) & 1u) : 0;
                if (inF != inS) {
                    const SpV S = dl_ld6<ST>(W, DL_S + 6 * l);
                    const V3 vp = add3(S.v, cross3(S.w, pos));
                    const double a0 = dot3(n, vp), a1 = dot3(t1, vp), a2 = dot3(t2, vp);
                    j0 = inF ? a0 : -a0; j1 = inF ? a1 : -a1; j2 = inF ? a2 : -a2;
                }
            } else if (l < nd + 6) {
                const int sg = (bf == nd) ? 1 : ((bs == nd) ? -1 : 0);
                if (sg) {
                    const V3 r = sub3(pos, o.c);
                    const V3 r0 = matT_vec(o.RD, cross3(r, n)), r1 = matT_vec(o.RD, cross3(r, t1)), r2 = matT_vec(o.RD, cross3(r, t2));
                    const int j = l - nd;
                    double a0, a1, a2;
                    if (j == 0) { a0 = n.x; a1 = t1.x; a2 = t2.x; }
                    else if (j == 1) { a0 = n.y; a1 = t1.y; a2 = t2.y; }
                    else if (j == 2) { a0 = n.z; a1 = t1.z; a2 = t2.z; }
                    else if (j == 3) { a0 = r0.x; a1 = r1.x; a2 = r2.x; }
                    else if (j == 4) { a0 = r0.y; a1 = r1.y; a2 = r2.y; }
                    else { a0 = r0.z; a1 = r1.z; a2 = r2.z; }
                    j0 = (sg > 0) ? a0 : -a0; j1 = (sg > 0) ? a1 : -a1; j2 = (sg > 0) ? a2 : -a2;
                }
            }
            ct_fence();        // every lane has read the detection scratch before the rows overwrite it
            DLW(s + CT_J + l) = j0; DLW(s + CT_J + 16 + l) = j1; DLW(s + CT_J + 32 + l) = j2;
            // scalars every lane derives alike go to the record; dist / ids are kept for the rows below
            DLW(s + CT_AREF) = dist;                       // (parked: replaced by the row's reference acceleration below)
            DLW(s + CT_KEY) = __longlong_as_double(ids);
        }
        ct_fence();
        // M^-1 J^T of the arm dofs: one right-hand side (contact, direction) per lane
        for (int r0 = 0; r0 < 3 * ncon; r0 += 16) {
            const int r = r0 + l;
            if (r < 3 * ncon) {
                const int c = r / 3, a = r - 3 * c;
                const int s = ch.con_slot + kCtRec * c;
                double x[kDynMax];
                bool any = false;
#pragma unroll
                for (int k = 0; k < kDynMax; k++) {
                    x[k] = (k < nd) ? DLW(s + CT_J + 16 * a + k) : 0.0;
                    any = any || (k < nd && x[k] != 0.0);
                }
                if (arm_touch && any) ct_ldl_apply(nd, A2, dinv, x);
                else {
#pragma unroll
                    for (int k = 0; k < kDynMax; k++) x[k] = x[k] * 0.0;
                }
#pragma unroll
                for (int k = 0; k < kDynMax; k++)
                    if (k < nd) DLW(s + CT_B + 9 * a + k) = x[k];
            }
        }
        ct_fence();
        // Gram matrix, regulariser, reference acceleration, warm start
        for (int c = 0; c < ncon; c++) {
            const int s = ch.con_slot + kCtRec * c;
            const double dist = DLW(s + CT_AREF);
            const long long ids = __double_as_longlong(DLW(s + CT_KEY));
            const double *par = PR + (size_t)kCtPrRec * (int)(ids & 0xffff) + PR_PAR;
            const double Jn = DLW(s + CT_J + l), J1 = DLW(s + CT_J + 16 + l), J2 = DLW(s + CT_J + 32 + l);
            double Bn, B1, B2;
            if (l < nd) { Bn = DLW(s + CT_B + l); B1 = DLW(s + CT_B + 9 + l); B2 = DLW(s + CT_B + 18 + l); }
            else { Bn = Jn * invM_l; B1 = J1 * invM_l; B2 = J2 * invM_l; }
            const double G0 = ct_sum16(Jn * Bn), G1 = ct_sum16(Jn * B1), G2 = ct_sum16(Jn * B2), G3 = ct_sum16(J1 * B1), G4 = ct_sum16(J1 * B2),
                         G5 = ct_sum16(J2 * B2);
            const double jvn = ct_sum16(Jn * vel_l), jv1 = ct_sum16(J1 * vel_l), jv2 = ct_sum16(J2 * vel_l);
            const double mu = par[0];
            const double imp = ct_impedance(par, dist);
            const double kpos = (par[2] * imp) * (dist - par[1]);
            double f[4] = {0.0, 0.0, 0.0, 0.0};
            if (ch.warmstart) {
                const long long key = ids & 0xffffffffll;
                const unsigned m = (unsigned)((__ballot(okey >= 0 && (okey & 0xffffffffll) == key) >> (16 * grp)) & 0xffffull);
                if (m) {
                    const int src = 16 * grp + (__ffs(m) - 1);
                    f[0] = __shfl(of0, src, 64); f[1] = __shfl(of1, src, 64); f[2] = __shfl(of2, src, 64); f[3] = __shfl(of3, src, 64);
                    double Fn = (f[0] + f[1]) + (f[2] + f[3]);
                    double F1 = mu * (f[0] - f[1]), F2 = mu * (f[2] - f[3]);
                    qacc_l = fma(B2, F2, fma(B1, F1, fma(Bn, Fn, qacc_l)));
                }
            }
            ct_fence();
            DLW(s + CT_G) = G0; DLW(s + CT_G + 1) = G1; DLW(s + CT_G + 2) = G2; DLW(s + CT_G + 3) = G3; DLW(s + CT_G + 4) = G4; DLW(s + CT_G + 5) = G5;
            DLW(s + CT_MU) = mu;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double sm = (i & 1) ? -mu : mu;
                const double Gnt = (i < 2) ? G1 : G2, Gtt = (i < 2) ? G3 : G5;
                const double Aii = fma(sm * sm, Gtt, fma(2.0 * sm, Gnt, G0));
                double Ri = ((1.0 - imp) / imp) * Aii;
                if (Ri < kMinVal) Ri = kMinVal;
                const double Di = Aii + Ri;
                const double jv = fma(sm, (i < 2) ? jv1 : jv2, jvn);
                DLW(s + CT_R + i) = Ri;
                DLW(s + CT_D + i) = Di;
                DLW(s + CT_INVD + i) = 1.0 / ((SOLVER >= 1) ? Ri : Di);        // Newton: the row's weight D = 1 / R; Gauss-Seidel: 1 / (A + R)
                DLW(s + CT_AREF + i) = fma(-par[3], jv, -kpos);
                DLW(s + CT_F + i) = f[i];
            }
        }
        ct_fence();
        CT_TICK(3);
        // projected Gauss-Seidel.  The visits are software-pipelined over two register buffers (A: even contacts, B: odd ones):
        // the next contact's rows and scalars are fetched from LDS while the current one's four pyramid rows run their
        // dependent chain -- one wave per SIMD, nothing else hides that latency -- and no buffer is ever copied.
        int sweeps = 0;
        if (SOLVER >= 1) {
            double objM_l = 0.0;
            if (l == nd || l == nd + 1 || l == nd + 2) objM_l = ch.o_mass;
            else if (l == nd + 3) objM_l = ch.o_in0;
            else if (l == nd + 4) objM_l = ch.o_in1;
            else if (l == nd + 5) objM_l = ch.o_in2;
            sweeps = ct_newton<ST>(ch, W, l, nd, ncon, arm_touch, a0_l, objM_l, qacc_l, lside, laref, lD, limf_l);
        } else {
            CtVisit A, B;
            ct_visit_load<ST>(W, ch.con_slot, 0, l, nd, invM_l, A);
            bool run = true;
            for (int sw = 0; sw < ch.iterations; sw++) {
                if (!run) break;
                double improvement = 0.0;
                for (int c = 0; c < ncon; c += 2) {
                    const bool two = c + 1 < ncon;
                    if (two) ct_visit_load<ST>(W, ch.con_slot, c + 1, l, nd, invM_l, B);
                    improvement = improvement + ct_visit<ST>(W, ch.con_slot + kCtRec * c, A, qacc_l);
                    ct_visit_load<ST>(W, ch.con_slot, (c + 2 < ncon) ? c + 2 : 0, l, nd, invM_l, A);     // (after A's forces are stored)
                    if (two) improvement = improvement + ct_visit<ST>(W, ch.con_slot + kCtRec * (c + 1), B, qacc_l);
                }
                sweeps++;
                if (improvement * ch.inv_scale < ch.tol) run = false;
            }
        }
        CT_TICK(4);
        // the noslip pass (MuJoCo's noslip_iterations: Gauss-Seidel over the friction dimensions without the regulariser, normal
        // forces -- the sums of the opposing edge pairs -- kept) on a COPY of the forces: the regularised solution stays in CT_F
        // as the next sub-step's warm start.  Same arithmetic as oracle ct_noslip_contact.
        for (int c = 0; c < ncon; c++) {
            const int s = ch.con_slot + kCtRec * c;
            if (l < 4) DLW(s + CT_FS + l) = DLW(s + CT_F + l);
        }
        ct_fence();
        {
            bool run = true;
            for (int sw = 0; sw < ch.noslip_iters; sw++) {
                if (!run) break;
                double improvement = 0.0;
                for (int c = 0; c < ncon; c++) {
                    const int s = ch.con_slot + kCtRec * c;
                    const double J1 = DLW(s + CT_J + 16 + l), J2 = DLW(s + CT_J + 32 + l);
                    double B1, B2;
                    if (l < nd) { B1 = DLW(s + CT_B + 9 + l); B2 = DLW(s + CT_B + 18 + l); }
                    else { B1 = J1 * invM_l; B2 = J2 * invM_l; }
                    const double G3 = DLW(s + CT_G + 3), G4 = DLW(s + CT_G + 4), G5 = DLW(s + CT_G + 5);
                    const double m2 = 2.0 * DLW(s + CT_MU);
                    double fs[4], ar[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) { fs[i] = DLW(s + CT_FS + i); ar[i] = DLW(s + CT_AREF + i); }
                    double u1 = ct_sum16(J1 * qacc_l), u2 = ct_sum16(J2 * qacc_l);
                    double D1 = 0.0, D2 = 0.0, ic = 0.0;
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const int i0 = 2 * t, i1 = i0 + 1;
                        const double ut = t ? u2 : u1, Gtt = t ? G5 : G3;
                        const double K = 0.5 * (fs[i0] + fs[i1]), y0 = 0.5 * (fs[i0] - fs[i1]);
                        const double a = (m2 * m2) * Gtt;
                        const double dres = fma(m2, ut, -(ar[i0] - ar[i1]));
                        double y = y0 - dres / a;
                        if (y > K) y = K;
                        if (y < -K) y = -K;
                        const double dy = y - y0;
                        fs[i0] = K + y;
                        fs[i1] = K - y;
                        const double dT = m2 * dy;
                        u1 = fma(t ? G4 : G3, dT, u1);
                        u2 = fma(t ? G5 : G4, dT, u2);
                        if (t) D2 = D2 + dT; else D1 = D1 + dT;
                        ic = ic - dy * fma(0.5 * dy, a, dres);
                    }
                    if (l < 4) DLW(s + CT_FS + l) = (l == 0) ? fs[0] : ((l == 1) ? fs[1] : ((l == 2) ? fs[2] : fs[3]));
                    qacc_l = fma(B2, D2, fma(B1, D1, qacc_l));
                    improvement = improvement + ic;
                }
                if (improvement * ch.inv_scale < ch.noslip_tol) run = false;
            }
        }
        // generalised contact forces of this lane's dof
        for (int c = 0; c < ncon; c++) {
            const int s = ch.con_slot + kCtRec * c;
            const double f0 = DLW(s + CT_FS), f1 = DLW(s + CT_FS + 1), f2 = DLW(s + CT_FS + 2), f3 = DLW(s + CT_FS + 3), mu = DLW(s + CT_MU);
            double Fn = (f0 + f1) + (f2 + f3);
            double F1 = mu * (f0 - f1), F2 = mu * (f2 - f3);
            tc_l = fma(DLW(s + CT_J + 32 + l), F2, fma(DLW(s + CT_J + 16 + l), F1, fma(DLW(s + CT_J + l), Fn, tc_l)));
        }
        tc_l = tc_l + limf_l;
        cnt.contacts += ncon; cnt.sweeps += sweeps;
        if (ncon > cnt.maxc) cnt.maxc = ncon;
    }
    nwarm = ncon;
    ct_fence();
    CT_TICK(5);
    DLW(qv + 32 + l) = tc_l;
    ct_fence();
    // ---- integration: the arm as in stage A with the contact forces added, then the object
    {
        double A[kDynMax * (kDynMax + 1) / 2];
        dyn_m_gather<ST>(dh, W, A);
        dyn_solve_integrate<ST>(dh, DD, W, bias, A, qv + 32, ch.limit_rows == 0);
    }
    ct_obj_integrate<ST>(dh, ch, W, qv, o, wb, Fo, Tb);
    ct_fence();
    CT_TICK(6);
}

// Contact-force readout (mopa_env_set_contact_force), after the sub-step loop: what mj_contactForce would return for the `ncon` contacts of
// the launch's LAST constraint solve (the solve of the last sub-step, at the state that sub-step started from), read from the records that
// solve left in LDS -- the post-noslip forces, the ones that acted.  Elliptic cones (SOLVER 2): the contact's dim solver forces; pyramidal
// cones: normal and tangential sums of the four edge forces, the expression order of ct_substep's J^T f.  Lane c holds contact c and
// writes its row (pair, feature, f0 .. f5); s_c = |f0| + .. + |f5| and the sum over the contacts in contact order are plain adds, so the
// host reproduces `force` from the rows bit for bit; lane 0 writes the scalars.  PARITY UNPINNED like the solve it reads.
template <int ST, int SOLVER>
__device__ __forceinline__ void ct_force_readout(const CtHdr &ch, const double *W, int l, int grp, int nd, int ncon, bool write, long long e,
                                                 const CfOut &cf) {
    double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long ids = 0;
    if (l < ncon) {
        if constexpr (SOLVER == 2) {
            const CtRecRef r = ct_rec_w<6>(ch, (int)__double_as_longlong(DLW(ch.tab_slot + l)), l, nd);
            ids = __double_as_longlong(DLW(r.s + CT_IDS));
#pragma unroll
            for (int a = 0; a < kCtMaxDim; a++)
                if (a < r.dim) f[a] = DLW(r.row_s + 2 * r.dim + a);
        } else {
            const int s = ch.con_slot + kCtRec * l;
            ids = __double_as_longlong(DLW(s + CT_KEY));
            const double f0 = DLW(s + CT_FS), f1 = DLW(s + CT_FS + 1), f2 = DLW(s + CT_FS + 2), f3 = DLW(s + CT_FS + 3), mu = DLW(s + CT_MU);
            f[0] = (f0 + f1) + (f2 + f3);
            f[1] = mu * (f0 - f1);
            f[2] = mu * (f2 - f3);
        }
    }
    const double s_l = ((((fabs(f[0]) + fabs(f[1])) + fabs(f[2])) + fabs(f[3])) + fabs(f[4])) + fabs(f[5]);
    double force = 0.0;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const double s_c = __shfl(s_l, 16 * grp + c, 64);
        if (c < ncon) force = force + s_c;
    }
    if (!write) return;
    if (cf.rows && l < ncon) {
        double *row = cf.rows + ((size_t)e * (size_t)cf.K + (size_t)l) * 8;
        row[0] = (double)(int)(ids & 0xffff);
        row[1] = (double)(int)((ids >> 16) & 0xffff);
#pragma unroll
        for (int a = 0; a < 6; a++) row[2 + a] = f[a];
    }
    if (l == 0) {
        cf.force[e] = force;
        if (cf.total) cf.total[e] = cf.total[e] + force;
        if (cf.count) cf.count[e] = ncon;
    }
}

// mode 0: env.step's physics (ctrl from the action, prev_state / has_prev updated, dh.nsub sub-steps when the move flag is set);
// mode 1: n_steps sub-steps towards the given ctrl rows [E, nd].  qvel rows are [nd + 6].
// ch.cf (optional, cf.force != nullptr): the contact-force readout of the last sub-step, for the envs that ran one -- in the header the
// kernel reads through scalar loads anyway, so the kernel's arguments (and what it keeps in registers over the sub-step loop) stay as they were.
template <int SOLVER>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_env_dyn_ct(
    EnvHdr h, const DynHdr *__restrict__ dhp, const CtHdr *__restrict__ chp, const double *__restrict__ GD, const int32_t *__restrict__ GI,
    const double *__restrict__ DD, const double *__restrict__ FT, const double *__restrict__ PR, long long E,
    int mode, int n_steps, double *__restrict__ qpos, double *__restrict__ qvel, double *__restrict__ bias_lag, double *__restrict__ prev_state,
    unsigned char *__restrict__ has_prev, const double *__restrict__ action, int is_planner, const unsigned char *__restrict__ move_mask,
    const double *__restrict__ ctrl_in, int32_t *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ST = 4;
    const int lane = threadIdx.x, grp = lane >> 4, l = lane & 15;
    double *W = reinterpret_cast<double *>(smem) + grp;
    const DynHdr &dh = *dhp;
    const CtHdr &ch = *chp;
    // the wave's copy of the dof records (behind the four envs' columns): the lane-parallel phases index them by lane
    double *DC = reinterpret_cast<double *>(smem) + (size_t)ch.env_slots * 4;
    for (int k = lane; k < kCtDc * dh.nd; k += 64) {
        const int i = k / kCtDc, f = k - kCtDc * i;
        const double *rec = DD + kDynRec * i;
        DC[k] = f == 0 ? rec[DR_MASS] : (f < 4 ? rec[DR_IPOS + f - 1] : (f < 10 ? rec[DR_INERTIA + f - 4] : (f == 10 ? rec[DR_ARM] : (double)dh.parent[i])));
    }
    long long e = (long long)blockIdx.x * 4 + grp;
    bool live = e < E;
    if (!live) e = E - 1;
    const unsigned flags = move_mask ? move_mask[e] : 1u;
    if (flags & 2u) live = false;
    double *row = qpos + e * h.nq;
    // (all 16 lanes of an env's group fill its columns and form its command with the same values; lane 0 records it)
    dyn_cols_load<ST>(dh, W, e, row, qvel, bias_lag);
    CtObj o;
    const bool has_obj = ch.obj_qadr >= 0;       // (false: the contact-free form -- stage A's smooth dynamics in this kernel's 16-lane mapping)
    o.p = V3{0.0, 0.0, 0.0}; o.q = Q4{1.0, 0.0, 0.0, 0.0}; o.v = V3{0.0, 0.0, 0.0}; o.w = V3{0.0, 0.0, 0.0};
    if (has_obj) {
        o.p = V3{row[ch.obj_qadr], row[ch.obj_qadr + 1], row[ch.obj_qadr + 2]};
        o.q = Q4{row[ch.obj_qadr + 3], row[ch.obj_qadr + 4], row[ch.obj_qadr + 5], row[ch.obj_qadr + 6]};
        o.v = V3{qvel[e * dh.nv + dh.nd], qvel[e * dh.nv + dh.nd + 1], qvel[e * dh.nv + dh.nd + 2]};
        o.w = V3{qvel[e * dh.nv + dh.nd + 3], qvel[e * dh.nv + dh.nd + 4], qvel[e * dh.nv + dh.nd + 5]};
    }
    if (mode == 0) {
        // dyn_command's loop (mopa_dyn.inc), kept here with a fence before lane 0 records the command.  The fence ORDERS NOTHING and is
        // no correctness requirement: the 16 lanes of a group store the same values in program order within one wave, and the kernel
        // fences again after the loop; dyn_command in its place passes every bit-exact test.  It only holds the code generation: without
        // it the compiler allocates the registers of the sub-step loop differently, and Lift with contacts lost 1 % (profiles/r24)
        double *prev = prev_state + e * h.n_arm;
        const bool use_prev = is_planner && has_prev[e];
        const double *act = action + e * h.adim;
        for (int i = 0; i < dh.nd; i++) {
            const int k = dh.act_of[i];
            if (k < 0) continue;
            double target;
            if (k < h.n_arm) {
                target = env_desired(h, use_prev ? prev[k] : DLW(DL_Q + i), act[k], is_planner, false);
                ct_fence();
                if (live && l == 0) prev[k] = target;
            } else target = DLW(DL_Q + i) + act[h.n_arm];
            DLW(DL_CTRL + i) = clampd(target, GD[h.o_act_lo + k], GD[h.o_act_hi + k]);
        }
        if (live && l == 0) has_prev[e] = 1;
        if (!(flags & 1u)) live = false;
        n_steps = (flags & 1u) ? dh.nsub : 0;
    } else {
        for (int i = 0; i < dh.nd; i++) DLW(DL_CTRL + i) = ctrl_in[e * dh.nd + i];
    }
    ct_fence();
    int nwarm = 0;
    CtCounters cnt{0, 0, 0, 0};
#ifdef MOPA_CT_PROF
    const unsigned long long tw0_ = wall_clock64();
#endif
    if constexpr (SOLVER == 2) {
        CtWarmReg wr;
        wr.key = -1;
#pragma unroll
        for (int a = 0; a < kCtMaxDim; a++) wr.f[a] = 0.0;
#pragma unroll 1
        for (int it = 0; it < n_steps; it++) ct_substep_ell<ST>(dh, ch, DD, FT, PR, DC, W, l, grp, it, o, nwarm, wr, cnt);
    } else {
#pragma unroll 1
        for (int it = 0; it < n_steps; it++) ct_substep<ST, SOLVER>(dh, ch, DD, FT, PR, DC, W, l, grp, it, o, nwarm, cnt);
    }
#ifdef MOPA_CT_PROF
    cnt.maxc = (int)(wall_clock64() - tw0_);       // prof builds: the wave's time in the sub-step loop (100 MHz ticks) in the max-contacts word
#endif
    if (ch.cf.force) ct_force_readout<ST, SOLVER>(ch, W, l, grp, dh.nd, nwarm, live && n_steps > 0, e, ch.cf);
    if (live && l == 0) {
        dyn_cols_store<ST>(dh, W, e, row, qvel, bias_lag);
        if (has_obj) {
            row[ch.obj_qadr] = o.p.x; row[ch.obj_qadr + 1] = o.p.y; row[ch.obj_qadr + 2] = o.p.z;
            row[ch.obj_qadr + 3] = o.q.w; row[ch.obj_qadr + 4] = o.q.x; row[ch.obj_qadr + 5] = o.q.y; row[ch.obj_qadr + 6] = o.q.z;
            qvel[e * dh.nv + dh.nd] = o.v.x; qvel[e * dh.nv + dh.nd + 1] = o.v.y; qvel[e * dh.nv + dh.nd + 2] = o.v.z;
            qvel[e * dh.nv + dh.nd + 3] = o.w.x; qvel[e * dh.nv + dh.nd + 4] = o.w.y; qvel[e * dh.nv + dh.nd + 5] = o.w.z;
        }
        if (stats) { stats[4 * e] = cnt.contacts; stats[4 * e + 1] = cnt.sweeps; stats[4 * e + 2] = cnt.dropped; stats[4 * e + 3] = cnt.maxc; }
    }
}
#undef DLW

extern "C" int mopa_env_attach_contacts(MopaEnv *env, const MopaCtDesc *d) {
    if (!env || !d) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (!env->d_dyn) return fail(MOPA_ERR_INVALID_ARG, "attach the dynamics first (mopa_env_attach_dynamics)");
    if (env->dyn.obj_on) return fail(MOPA_ERR_INVALID_ARG, "the penalty-contact object model (MopaObjDesc) and the constraint stage exclude each other");
    const DynHdr &dh = env->dyn;
    const int nd = dh.nd;
    if (nd + 6 > 15) return fail(MOPA_ERR_LIMIT, "the contact stage keeps 9 arm dofs + the object's 6");
    // obj_qadr < 0 with no pairs: no contact stage and no object at all -- stage A's contact-free servo dynamics (joint limits = inelastic
    // stops) run through this kernel's mapping (16 lanes per env, one wave per SIMD over the whole chip) instead of K6's lane per env
    const bool smooth_only = d->obj_qadr < 0;
    if (smooth_only && (d->np != 0 || d->limit_rows)) return fail(MOPA_ERR_INVALID_ARG, "obj_qadr < 0 selects the contact-free form: no pairs, no limit rows");
    if (d->ns < 0 || (!smooth_only && d->ns == 0) || d->np < 0 || d->nf < 0 || d->np > 65535 || d->nf > 65535) return fail(MOPA_ERR_INVALID_ARG, "bad shape / pair / feature counts");
    if (d->maxcon < (smooth_only ? 0 : 1) || d->maxcon > 16 || d->maxpair < 1) return fail(MOPA_ERR_LIMIT, "the kernel keeps 1 .. 16 contacts per env and sub-step");
    if (!smooth_only && d->obj_qadr + 7 > env->hdr.nq) return fail(MOPA_ERR_INVALID_ARG, "object qadr out of range");
    if (d->iterations < 1 || d->precull_every < 1 || !(d->precull_margin >= 0.0) || d->noslip_iterations < 0)
        return fail(MOPA_ERR_INVALID_ARG, "bad solver / precull parameters");
    CtHdr ch{};
    ch.ns = d->ns; ch.nf = d->nf; ch.np = d->np; ch.maxcon = d->maxcon; ch.maxpair = d->maxpair; ch.iterations = d->iterations;
    ch.near_every = d->near_every; ch.margin_near = d->near_margin;
    if (d->near_every < 1 || d->precull_every % d->near_every != 0 || !(d->near_margin >= 0.0) || d->near_margin > d->precull_margin)
        return fail(MOPA_ERR_INVALID_ARG, "near_every must divide precull_every, 0 <= near_margin <= precull_margin");
    ch.every = d->precull_every; ch.warmstart = d->warmstart; ch.obj_qadr = d->obj_qadr; ch.nwords = (d->np + 63) / 64;
    for (int b = 0; b < nd; b++) {
        unsigned m = 0;
        for (int k = b; k >= 0; k = dh.parent[k]) m |= 1u << k;
        ch.anc[b] = m;
    }
    ch.o_mass = d->obj_mass; ch.o_in0 = d->obj_inertia[0]; ch.o_in1 = d->obj_inertia[1]; ch.o_in2 = d->obj_inertia[2];
    ch.o_ipx = d->obj_ipos[0]; ch.o_ipy = d->obj_ipos[1]; ch.o_ipz = d->obj_ipos[2];
    ch.o_iqw = d->obj_iquat[0]; ch.o_iqx = d->obj_iquat[1]; ch.o_iqy = d->obj_iquat[2]; ch.o_iqz = d->obj_iquat[3];
    ch.o_damp = d->obj_damping; ch.o_imass = d->obj_inv_mass; ch.o_iin0 = d->obj_inv_inertia[0]; ch.o_iin1 = d->obj_inv_inertia[1]; ch.o_iin2 = d->obj_inv_inertia[2];
    ch.o_imass_d = d->obj_inv_mass_d; ch.o_iin0_d = d->obj_inv_inertia_d[0]; ch.o_iin1_d = d->obj_inv_inertia_d[1]; ch.o_iin2_d = d->obj_inv_inertia_d[2];
    ch.tol = d->tolerance; ch.inv_scale = d->inv_scale; ch.margin_pre = d->precull_margin;
    ch.noslip_iters = d->noslip_iterations; ch.noslip_tol = d->noslip_tolerance;
    ch.limit_rows = d->limit_rows ? 1 : 0;
    for (int k = 0; k < 8; k++) ch.lim_par[k] = d->lim_par[k];
    if (d->limit_rows && d->solver != 1 && d->solver != 2) return fail(MOPA_ERR_INVALID_ARG, "joint limits as solver rows need the Newton solver");
    if (d->solver < 0 || d->solver > 2) return fail(MOPA_ERR_INVALID_ARG, "solver: 0 (projected Gauss-Seidel, pyramidal cones), 1 (Newton, pyramidal cones) or 2 (Newton, elliptic cones)");
    if (d->solver == 1 && d->maxcon > 8) return fail(MOPA_ERR_LIMIT, "the Newton solver with pyramidal cones keeps at most 8 contacts (32 constraint rows on 16 lanes)");
    if (d->maxcon > 16) return fail(MOPA_ERR_LIMIT, "at most 16 contacts per env (one per lane of its group)");
    // LDS slots of an env: K6's columns, then body poses, the pair mask, the contact records; vel | qacc | tc over the IC columns
    const int base = DL_SAVE + kDynSaveStride * dh.n_save;
    ch.xp_slot = base;
    ch.mask_slot = ch.xp_slot + 7 * nd;
    ch.near_slot = ch.mask_slot + ch.nwords;
    ch.tab_slot = ch.near_slot + ch.nwords;
    ch.con_slot = ch.tab_slot + (d->solver == 2 ? 16 : 0);
    ch.qv_slot = DL_IC;
    ch.hot_slot = ch.qv_slot + 64;      // consumed by the narrow phase before the constraint stage uses its scratch (48 + 16 slots)
    if (64 + ch.nwords > 10 * kDynMax) return fail(MOPA_ERR_LIMIT, "too many directed pairs for the contact stage's scratch");
    // the contact records: solvers 0 / 1 fixed records of kCtRec slots; solver 2 an arena of variable-size records (mopa_contact_ell.inc) --
    // by default what is left of the LDS share of an env when four waves (16 envs) keep a CU, at least one full-size record
    size_t rec_slots = (size_t)kCtRec * d->maxcon;
    if (d->solver == 2) {
        const int per_env = kMaxLdsBytes / 8 / 16 - (kCtDc * nd + 3) / 4;
        int arena = d->arena > 0 ? d->arena : per_env - ch.con_slot;
        const int one = ct_record_size(kCtMaxDim, true, true, nd);
        if (arena < one) arena = one;
        if (arena > 4095) arena = 4095;
        ch.arena = arena;
        rec_slots = (size_t)arena;
        for (int p = 0; p < d->np; p++) {
            const int dim = (int)d->pr_par[kCtPar * p + 8];
            if (dim != 3 && dim != 4 && dim != 6) return fail(MOPA_ERR_INVALID_ARG, "pr_par[:, 8] (condim) must be 3, 4 or 6");
        }
    }
    const size_t slots = (size_t)ch.con_slot + rec_slots;
    ch.env_slots = (int)slots;
    const size_t lds = (slots * 4 + (size_t)kCtDc * nd) * sizeof(double);
    if (lds > (size_t)kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "contact stage does not fit the LDS");
    std::vector<double> ft((size_t)kCtFtRec * std::max(d->nf, 1)), pr((size_t)kCtPrRec * std::max(d->np, 1), 0.0);
    for (int s = 0; s < d->ns; s++) {
        if (d->sh_body[s] < -1 || d->sh_body[s] > nd) return fail(MOPA_ERR_INVALID_ARG, "shape body out of range");
        if (d->sh_feat0[s + 1] < d->sh_feat0[s] || d->sh_feat0[s + 1] > d->nf) return fail(MOPA_ERR_INVALID_ARG, "feature ranges must ascend");
    }
    for (int k = 0; k < d->nf; k++) {
        std::memcpy(&ft[(size_t)kCtFtRec * k], d->ft_pos + 3 * k, 24);
        ft[(size_t)kCtFtRec * k + 3] = d->ft_rad[k];
    }
    for (int p = 0; p < d->np; p++) {
        const int sf = d->pr_f[p], ss = d->pr_s[p];
        if (sf < 0 || sf >= d->ns || ss < 0 || ss >= d->ns) return fail(MOPA_ERR_INVALID_ARG, "pair shape out of range");
        double *r = &pr[(size_t)kCtPrRec * p];
        r[0] = sf; r[1] = ss;
        std::memcpy(r + PR_PAR, d->pr_par + kCtPar * p, 8 * kCtPar);
        r[PR_BF] = d->sh_body[sf]; r[PR_BS] = d->sh_body[ss]; r[PR_TYPE] = d->sh_type[ss]; r[PR_RBF] = d->sh_rbound[sf];
        std::memcpy(r + PR_PF, d->sh_pos + 3 * sf, 24);
        std::memcpy(r + PR_PS, d->sh_pos + 3 * ss, 24);
        std::memcpy(r + PR_MS, d->sh_mat + 9 * ss, 72);
        std::memcpy(r + PR_SZ, d->sh_size + 3 * ss, 24);
        r[PR_F0] = d->sh_feat0[sf]; r[PR_NF] = d->sh_feat0[sf + 1] - d->sh_feat0[sf];
        r[PR_TYPEF] = d->sh_type[sf]; r[PR_RBS] = d->sh_rbound[ss];
        std::memcpy(r + PR_SZF, d->sh_size + 3 * sf, 24);
        std::memcpy(r + PR_MF, d->sh_mat + 9 * sf, 72);
    }
    DeviceGuard guard(env->device);
    if (!guard.ok()) return fail(MOPA_ERR_HIP, "hipSetDevice failed");
    // everything is allocated and uploaded into locals; env changes only once nothing can fail any more
    std::vector<double> all(ft);
    all.insert(all.end(), pr.begin(), pr.end());
    double *tab = nullptr;
    CtHdr *nh = nullptr;
    DynHdr dyn = env->dyn;
    dyn.nv = nd + (smooth_only ? 0 : 6);
    auto drop = [&](const char *what) {
        if (tab) (void)hipFree(tab);
        if (nh) (void)hipFree(nh);
        return fail(MOPA_ERR_HIP, what);
    };
    if (upload_array(all.data(), all.size(), &tab) != hipSuccess) return drop("upload of the contact tables failed");
    if (!env->d_cthdr && hipMalloc((void **)&nh, sizeof(CtHdr)) != hipSuccess) return drop("allocation of the contact header failed");
    if (hipMemcpy(nh ? nh : env->d_cthdr, &ch, sizeof(CtHdr), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(env->d_dynhdr, &dyn, sizeof(DynHdr), hipMemcpyHostToDevice) != hipSuccess)
        return drop("upload of the contact / dynamics headers failed");
    if (env->d_ct) {
        std::lock_guard<std::mutex> lock(env->mu);
        env->retired.push_back(env->d_ct);
    }
    env->d_ct = tab;
    env->ct_ft_off = 0; env->ct_pr_off = ft.size();
    if (nh) env->d_cthdr = nh;
    env->ct_lds = lds;
    env->ct_on = true;
    env->ct_solver = d->solver;
    env->ct_arena = ch.arena;
    env->ct_maxcon = d->maxcon;
    env->cf = CfOut{nullptr, nullptr, nullptr, nullptr, 0};
    env->dyn = dyn;
    for (const void *k : {(const void *)k_env_dyn_ct<0>, (const void *)k_env_dyn_ct<1>, (const void *)k_env_dyn_ct<2>})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    return MOPA_OK;
}

extern "C" int mopa_ct_desc_size(void) { return (int)sizeof(MopaCtDesc); }
extern "C" int mopa_env_contact_arena(const MopaEnv *env) { return (env && env->ct_on) ? env->ct_arena : -1; }
extern "C" int mopa_env_set_contact_stats(MopaEnv *env, int32_t *stats_dev) {
    if (!env || !env->ct_on) return fail(MOPA_ERR_INVALID_ARG, "env without the contact stage");
    env->ct_stats = stats_dev;
    return MOPA_OK;
}

static int env_ct_launch(MopaEnv *env, int64_t E, int mode, int n_steps, double *qpos, double *qvel, double *bias_lag, double *prev_state,
                         uint8_t *has_prev, const double *action, int is_planner, const uint8_t *move_mask, const double *ctrl, hipStream_t st) {
    const unsigned blocks = (unsigned)((E + 3) / 4);
    static constexpr decltype(&k_env_dyn_ct<0>) kerns[3] = {k_env_dyn_ct<0>, k_env_dyn_ct<1>, k_env_dyn_ct<2>};      // by solver (attach_contacts admits 0 .. 2)
    hipLaunchKernelGGL(kerns[env->ct_solver], dim3(blocks), dim3(64), env->ct_lds, st, env->hdr, env->d_dynhdr, env->d_cthdr, env->d_dbl, env->d_int, env->d_dyn,
                       env->d_ct + env->ct_ft_off, env->d_ct + env->ct_pr_off, (long long)E, mode, n_steps, qpos, qvel, bias_lag, prev_state,
                       has_prev, action, is_planner, move_mask, ctrl, env->ct_stats);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
