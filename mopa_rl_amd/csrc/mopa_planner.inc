// mopa_planner.inc -- K3: RRT-Connect, one wave64 per environment.
// (included at the end of mopa_hip.hip)
//
// Restates [3P] OMPL geometric::RRTConnect::solve/growTree as the reference
// configures it (reference motion_planners/KinematicPlanner.cpp:90,102-104,
// called at :188; goal check and sentinels :180-184,249-250), with
//   - an iteration budget instead of the wall-clock termination condition,
//   - a counter-based sample stream (seed, env id, iteration*na + dim),
//   - brute-force wave-parallel L1 nearest neighbour (exact, like GNAT; ties
//     resolve to the lowest node index),
//   - OMPL's DiscreteMotionValidator order (end state first, then breadth-first
//     bisection) so that the count of consumed validity checks is well defined.
// Trees live in HBM ([E][2][max_nodes][na] doubles + parents); the wave's
// working vectors live in its LDS slab.
//
// A planner wave is alone with its env, so what it pays for is the NUMBER of sequential validity passes times the latency
// of one (an FK chain, a broad phase, the pair classes one after the other).  Hence: (1) a pass poses up to kMS states
// side by side (plan_states_valid_ms); (2) its free slots carry states the algorithm will probably ask about next
// (plan_speculate: the connect step's first state, the next iteration's new state, the next states of a connect chain) --
// verdicts are a pure function of the state, they wait in a small memo and are consumed, and counted, only when the
// sequential algorithm asks for exactly that state; (3) every result -- status, path, consumed-check count -- stays
// bit-identical to the sequential oracle.  DESIGN.md section 4 (K3) has the measurements.
//
// Tried and rejected (round 1): one LANE per env (64 planners per wave, each validity request answered by
// a lane-per-state tile of the second-generation validity routine).  Same results, but a tile costs
// ~165 us however few lanes still need it, and every wave keeps a straggler (3 % of queries run out their
// iteration budget: ~10k sequential checks): 5.2 s per 4096-env batch against 0.14 s (now 0.055 s) for this kernel.
// Planning is latency-bound per env, so the wave-per-env mapping stays.

#if defined(__HIP_DEVICE_COMPILE__)
#define MOPA_ASSUME_LDS(p) __builtin_assume(__builtin_amdgcn_is_shared((const void *)(p)))
#else
#define MOPA_ASSUME_LDS(p) ((void)(p))
#endif
constexpr int kQCap = 256;   // bisection queue capacity == largest supported segment count per motion
enum { GROW_TRAPPED = 0, GROW_ADVANCED = 1, GROW_REACHED = 2 };

constexpr int kMS = 4;
#ifdef MOPA_PLAN_STATS   // debug builds: cycle accumulators of the planner phases (wave-latency view; tools/plan_passes.py)
__device__ unsigned long long g_plan_t[64];   // [8+c] ticks, [24+c] rounds of pair class c; [40] closed-form part, [41] refinement part of the narrow phase
__device__ unsigned g_plan_mpr_pairs[2 * 4096];        // entries into the portal refinement per (geom1, geom2), geoms < 64
#define PLAN_T0() const unsigned long long t0_ = wall_clock64()
// (timers and counters of the FIRST wave of a workgroup only: a launch of few queries puts one per workgroup there, and in the workgroup-per-
//  query build that wave is the one that evaluates what the algorithm asks)
#define PLAN_T(i) do { if (threadIdx.x == 0) atomicAdd(&g_plan_t[i], wall_clock64() - t0_); } while (0)
#else
#define PLAN_T0() do {} while (0)
#define PLAN_T(i) do {} while (0)
#endif
constexpr int kMemo = 8;    // states with a known verdict (ring)
constexpr int kSpec = 3;    // states queued for speculative evaluation
constexpr int kPlanVecs = 5 + kMemo + kSpec + 2;   // rs xs ns ts r2 | memo | spec | nn queries
MOPA_HD int plan_vec_bytes(int na) { return (kPlanVecs * na * 8 + 2 * kQCap * 2 + 15) & ~15; }
// ---- the workgroup-per-query build (tag K3WG, mopa_planner_k3.inc): four waves run ONE query --------------------------
// Table of FUTURE iterations, one slot per iteration modulo kFSlots: what waves 1-3 found out about iteration j while wave 0
// evaluated the states the sequential algorithm was asking about.  An entry is kFStride doubles:
//   8 ints: [0] iteration j  [1] flags  [2,3] nearest node of sample(j) in tree j&1: (tree size then, index)
//           [4,5] nearest node of D in the other tree: (tree size then, index)  [6,7] segment counts of the two motions
//   D  [8]: the state iteration j's first growTree creates (if the trees are still what they were)
//   ID [8]: the interior state of its motion when that has two segments (the common case beside one)
//   CF [8]: the state the first call of iteration j's connect step towards D creates;  IC [8]: the interior state of that motion
// flags: FF_NND / FF_NNC the nearest nodes are there; FF_DTRAP / FF_CTRAP steering from them gives no new state (growTree is trapped);
// FF_DS / FF_CS the state is stored (FF_DREACH / FF_CREACH: it is the target itself); FF_D / FF_C its verdict is known: FF_DOK / FF_COK;
// FF_DI / FF_CI the interior state's verdict is known: FF_DIOK / FF_CIOK.
constexpr int kFSlots = 8, kFStride = 36;
constexpr int FO_D = 4, FO_ID = 12, FO_C = 20, FO_IC = 28;
enum { FF_NND = 1, FF_D = 2, FF_DOK = 4, FF_NNC = 8, FF_C = 16, FF_COK = 32, FF_DTRAP = 64, FF_DREACH = 128, FF_DS = 256, FF_CTRAP = 512, FF_CREACH = 1024, FF_CS = 2048,
       FF_DI = 4096, FF_DIOK = 8192, FF_CI = 16384, FF_CIOK = 32768, FF_DIS = 65536, FF_CIS = 131072 /* interior state stored */ };
constexpr int kWgScratchVecs = 3;
// a wave's share of the pass mailbox: kMbHdr doubles of header (ints: states posed, verdict bits, entries, completions, then 4 x
// (iteration, flag bits) = verdicts of states the table already held) + 2 entries
constexpr int kMbHdr = 6, kMbStride = kMbHdr + 2 * kFStride;
MOPA_HD int plan_vec_bytes_wg(int na) { return (plan_vec_bytes(na) + kFSlots * kFStride * 8 + kWgScratchVecs * 8 * 8 + 15) & ~15; }
MOPA_HD int plan_wg_shared_bytes() { return 2 * kWavesPerBlock * kMbStride * 8 + 32; }   // mailbox (two parities) + the query-index words

struct MsLds {
    double *grec;      // [kMS][nmg * kGeomStride]
    double *qbuf;      // [kMS][na + n_pq + ms_sc_doubles]   joint values, then the joint table of the state
    unsigned *wl;      // [kMS * npair]   pair | state << 16
    double *qs;        // [kMS][na]       the states to test (active coordinates)
};
// doubles of a state's joint table: [nmb][4] = sin, cos of half the angle and the displacement of every moving body's first
// joint (ms_fk), or -- chains the planner FK does not take -- [nmj][2] sin / cos per joint (fk_one_geom)
MOPA_HD int ms_sc_doubles(int nmj, int nmb) { return (2 * nmj > 4 * nmb) ? 2 * nmj : 4 * nmb; }
MOPA_HD int ms_bytes_per_wave(int nmg, int na, int n_pq, int nsc /*ms_sc_doubles*/, int npair) {
    return ((kMS * (nmg * kGeomStride + na + n_pq + nsc + na) * 8 + kMS * npair * 4) + 15) & ~15;
}

struct PlanWs {
    double *tree_q;        // [E][2][max_nodes][na]
    int32_t *tree_parent;  // [E][2][max_nodes]
};

// One (non-inlined) copy of FK + collision for the whole planner: the routine is ~30 KB of code and the
// planner needs it at seven call sites; inlining them made a 400 KB kernel that lived in instruction-fetch stalls.
__device__ __noinline__ bool plan_state_valid_impl(const SceneHdr *hp, const double *dbl, const int *ints, double *grec,
                                                   double *qbuf, unsigned short *wl, int lane, const double *qa, const double *row) {
    // every pointer but `qa`/`row` is LDS: say so, or a non-inlined function reaches it through flat loads
    MOPA_ASSUME_LDS(hp); MOPA_ASSUME_LDS(dbl); MOPA_ASSUME_LDS(ints); MOPA_ASSUME_LDS(grec); MOPA_ASSUME_LDS(qbuf); MOPA_ASSUME_LDS(wl);
    const SceneHdr &h = *hp;
    LdsView v;
    v.dbl = dbl; v.ints = ints; v.grec = grec; v.qbuf = qbuf; v.sc = qbuf + h.na + h.n_pq + h.na; v.wl = wl;
    wave_load_state(h, v, lane, qa, row);
    wave_fk(h, v, lane);
    double md;
    // one copy of each instantiation; the branch is wave-uniform (scenes with a collidable mesh: Lift's can)
    return h.has_mesh ? wave_collide<false, true>(h, v, lane, md) : wave_collide<false, false>(h, v, lane, md);
}

// ---------------------------------------------------------------------------------------------------------
// Validity of up to kMS states in ONE pass.  A planner wave is latency-bound (one env, nothing else to overlap
// with): forward kinematics is a ~12-body dependent chain however many lanes run it, so the states a motion
// check needs next (end state + the first bisection points) are posed side by side -- 16 (or 32) lanes per
// state -- and their broad / narrow phases share the wave.  Verdicts per state are the same arithmetic as the
// single-state routine; OMPL's "stop at the first invalid state" only decides how many of them COUNT.
// ---------------------------------------------------------------------------------------------------------
template <bool MESH>
MOPA_D unsigned ms_collide(const SceneHdr &h, const LdsView &v0, const MsLds &m, int lane, int ns) {
    const int *I = v0.ints;
    const int gstride = h.nmg * kGeomStride;
    int cnt = 0;
    PLAN_T0();
    // broad phase: one pair per lane, all states of the pass side by side (kMS independent dependency chains per
    // lane -- a lone wave has nothing else to hide FP64 latency with); slabs of unused states hold stale data whose
    // results are discarded
    for (int base = 0; base < h.npair; base += 64) {
        const int p = base + lane;
        const bool live = p < h.npair;
        const int pk = live ? I[h.o_pairs + p] : 0;
        const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff;
        // pair_culled() for all states of the pass, written branch-free: what does not depend on the state is loaded
        // once, the centres of all states are fetched together, and the kMS chains of arithmetic are independent
        const double *D = v0.dbl;
        const int s1 = I[h.o_g_slot + g1], s2 = I[h.o_g_slot + g2];
        const bool plane = I[h.o_g_type + g1] == G_PLANE;
        const double *SA = D + h.o_g_rec + g1 * kGeomStride, *SB = D + h.o_g_rec + g2 * kGeomStride;
        const double rb1 = D[h.o_g_rbound + g1], rb2 = D[h.o_g_rbound + g2];
        const V3 nrm = col3(SA + GO_MAT, 2);
        const bool st1 = s1 < 0, st2 = s2 < 0;
        const bool use_aabb = !plane && (st1 != st2);
        const double *H = D + h.o_g_aabb + 3 * (st1 ? g1 : g2);
        const double h0 = H[0], h1 = H[1], h2 = H[2];
        const double rM = st1 ? rb2 : rb1, rs = rb1 + rb2, rs2 = rs * rs;
        V3 cA[kMS], cB[kMS];
#pragma unroll
        for (int s = 0; s < kMS; s++) {
            const double *gs = m.grec + s * gstride;
            cA[s] = ld3((st1 ? SA : gs + s1 * kGeomStride) + GO_POS);
            cB[s] = ld3((st2 ? SB : gs + s2 * kGeomStride) + GO_POS);
        }
        bool surv[kMS];
#pragma unroll
        for (int s = 0; s < kMS; s++) {
            const V3 diff = sub3(cB[s], cA[s]);
            const bool c_plane = dot3(diff, nrm) > rb2;
            const bool c_sph = dot3(diff, diff) > rs2;
            const bool c_box = (fabs(diff.x) > h0 + rM) | (fabs(diff.y) > h1 + rM) | (fabs(diff.z) > h2 + rM);
            const bool culled = (plane ? c_plane : c_sph) | (use_aabb & c_box);
            surv[s] = live & (s < ns) & !culled;
        }
#pragma unroll
        for (int s = 0; s < kMS; s++) {
            const unsigned long long mask = __ballot(surv[s]);
            if (surv[s]) m.wl[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned)p | ((unsigned)s << 16);
            cnt += __popcll(mask);
        }
    }
    wave_sync();
    PLAN_T(1);
    unsigned bad = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane;
        bool lane_bad = false;
        int ls = 0;
#ifdef MOPA_PLAN_STATS
        int mycode = -1;
#endif
        int code = -1, g1 = 0, g2 = 0;
        LdsView v = v0;
        if (i < cnt) {
            const unsigned w = m.wl[i];
            ls = (int)(w >> 16);
            v.grec = m.grec + ls * gstride;
            const int pk = I[h.o_pairs + (w & 0xffffu)];
            g1 = pk & 0xff; g2 = (pk >> 8) & 0xff; code = (pk >> 16) & 0xff;
#ifdef MOPA_PLAN_STATS
            mycode = code;
#endif
        }
        // closed-form classes first; the portal refinement (an order of magnitude slower) only for the states they
        // have not already condemned -- the verdict per state is an OR over its pairs, so the order is free
        const bool slow = code == PC_CONVEX || code == PC_CONVEX_MESH;
        if (code >= 0 && !slow) {
            const double d = geom_dist<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl);
            lane_bad = d <= h.thr;
        }
        for (int s = 0; s < ns; s++)
            if (__any(lane_bad && ls == s)) bad |= 1u << s;
        lane_bad = false;
        PLAN_T(40);
        if (slow && !((bad >> ls) & 1u)) {
            // (only the verdict is needed here: PC_CONVEX pairs that overlap deeper than the threshold skip the refinement)
            if (code == PC_CONVEX) lane_bad = convex_pair_bad(geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], h.thr);
            else lane_bad = geom_dist<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl) <= h.thr;
#if defined(MOPA_PLAN_STATS) && MOPA_PLAN_STATS >= 2   // which pairs the enclosing-capsule / separating-axis pre-tests let through (+1024: ... and penetrate)
            if (code == PC_CONVEX) {
                const double *A_ = geom_rec(h, v, g1), *B_ = geom_rec(h, v, g2);
                const int tb_ = I[h.o_g_type + g2];
                const double pre_ = (tb_ == G_BOX) ? d_capsule_box(A_, B_) : d_capsule_capsule(A_, B_);
                if (!(pre_ > 1e-9) && !convex_axes_separate(A_, I[h.o_g_type + g1], B_, tb_) &&
                    !convex_overlap_deeper_than(A_, I[h.o_g_type + g1], B_, tb_, convex_deep_delta(h.thr)))
                    atomicAdd(&g_plan_mpr_pairs[((g1 & 63) * 64 + (g2 & 63)) + (lane_bad ? 4096 : 0)], 1u);
            }
#endif
        }
#if defined(MOPA_PLAN_STATS) && MOPA_PLAN_STATS >= 2   // class-by-class replay, timed (results discarded; inflates the narrow-phase total)
        for (int cc = 0; cc < PC_COUNT; cc++) {
            if (!__any(mycode == cc)) continue;
            const unsigned long long t1_ = wall_clock64();
            double dd = 0.0;
            if (mycode == cc) {
                const unsigned w = m.wl[i];
                LdsView v = v0;
                v.grec = m.grec + (int)(w >> 16) * gstride;
                const int pk = I[h.o_pairs + (w & 0xffffu)];
                const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff;
                dd = geom_dist<MESH>(cc, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl);
            }
            asm volatile("" : "+v"(dd));
            if (__any(dd == 12345.678)) bad |= 1u << 31;
            if (threadIdx.x == 0) { atomicAdd(&g_plan_t[8 + cc], wall_clock64() - t1_); atomicAdd(&g_plan_t[24 + cc], 1ull); }
        }
#endif
        for (int s = 0; s < ns; s++)
            if (__any(lane_bad && ls == s)) bad |= 1u << s;
    }
    wave_sync();
    PLAN_T(2);
#ifdef MOPA_PLAN_STATS
    if (threadIdx.x == 0) { atomicAdd(&g_plan_t[3], (unsigned long long)cnt); atomicAdd(&g_plan_t[4], 1ull); atomicAdd(&g_plan_t[5], (unsigned long long)ns); }
#endif
    return ~bad & ((1u << ns) - 1u);
}

// ---------------------------------------------------------------------------------------------------------
// The planner's forward kinematics.  Same arithmetic, in the same order, over the same pieces (mopa_fk.hpp) as fk_one_geom
// (one lane per moving geom, its ancestor chain), restructured for a lone wave that waits on every dependent LDS read:
//   * the lane's chain comes packed in four words (h.o_pfk), so the body of step k is register arithmetic, not a read;
//   * sin / cos AND the displacement of a body's first joint sit in a per-state table indexed by BODY (written by the
//     pass's table phase), so everything a step needs is one level of reads off the body index ...
//     (issuing them a step ahead was tried: no gain, 50 registers -- the walk is bound by its ~200 FP64 instructions per
//     step at ~5 clocks each, tools/ubench/lone_wave.hip, not by the 64-clock LDS round trip);
//   * a body without joints or with one hinge anchored at its origin (every arm link) takes a branch-light step; anything
//     else (slide, free, off-centre hinge, several joints) the generic one.
// ---------------------------------------------------------------------------------------------------------
struct MsFkRec { V3 bp; Q4 bq; V3 ax; double sn, cs; int jn, w7, ja; };
MOPA_D MsFkRec ms_fk_load(const SceneHdr &h, const double *D, const int *I, const double *bt, int body) {
    MsFkRec r;
    const double *bd = D + h.o_mbd + 16 * body;
    r.bp = ld3(bd);
    r.bq = Q4{bd[3], bd[4], bd[5], bd[6]};
    r.ax = ld3(bd + 7);
    r.sn = bt[4 * body]; r.cs = bt[4 * body + 1];
    const int *ri = I + h.o_mbr + 8 * body;
    r.jn = ri[0]; r.ja = ri[1]; r.w7 = ri[7];
    return r;
}
MOPA_D void ms_fk(const SceneHdr &h, const double *D, const int *I, const double *qb, const double *bt, double *grec, int l) {
    const int *pw = I + h.o_pfk + 8 * l;
    const unsigned cw0 = (unsigned)pw[0], cw1 = (unsigned)pw[1], cw2 = (unsigned)pw[2], cw3 = (unsigned)pw[3];
    const int clen = pw[4], sf = pw[5];
    V3 pos;
    Q4 quat;
    double mat[9];
    sf_frame_ld(h, D, sf, pos, quat, mat);
    const int maxlen = h.pfk_maxlen;
    for (int k = 0; k < maxlen; k++) {
        if (k < clen) {
            const unsigned w = (k < 8) ? ((k < 4) ? cw0 : cw1) : ((k < 12) ? cw2 : cw3);
            const int body = (int)((w >> (8 * (k & 3))) & 0xffu);
            const MsFkRec cur = ms_fk_load(h, D, I, bt, body);
            const int jt0 = cur.w7 & 0x7f;
            const bool hinge0 = cur.jn == 1 && jt0 == J_HINGE && (cur.w7 & 0x80) != 0;
            if (cur.jn == 0 || hinge0) {
                pos = add3(pos, mat_vec(mat, cur.bp));
                Q4 q = quat_mul(quat, cur.bq);
                const Q4 qj = quat_mul(q, Q4{cur.cs, cur.ax.x * cur.sn, cur.ax.y * cur.sn, cur.ax.z * cur.sn});
                if (hinge0) q = qj;
                quat = quat_normalize(q);
            } else if (cur.jn == 1 && jt0 == J_FREE) {
                fk_free_step(qb + (cur.w7 >> 8), pos, quat);
            } else if (jt0 == J_GLUE) {     // the carried body of a glued scene: the jointless step, local pose out of the state's free-joint slots
                fk_glue_step(pos, quat, mat, qb + (cur.w7 >> 8), pos, quat);
                quat = quat_normalize(quat);
            } else {
                const double *bd = D + h.o_mbd + 16 * body;
                pos = add3(pos, mat_vec(mat, cur.bp));
                quat = quat_mul(quat, cur.bq);
                apply_joint_sc(jt0, cur.ax, ld3(bd + 10), (cur.w7 & 0x80) != 0, bt[4 * body + 2], cur.sn, cur.cs, pos, quat);
                for (int j = cur.ja + 1; j < cur.ja + cur.jn; j++) {       // further joints of the body: the separate joint tables
                    const V3 ax = ld3(D + h.o_mj_axis + 3 * j), jp = ld3(D + h.o_mj_pos + 3 * j);
                    const double dq = qb[I[h.o_mj_qsrc + j]] - D[h.o_mj_ref + j];
                    apply_joint(I[h.o_mj_type + j], ax, jp, is_zero3(jp), dq, pos, quat);
                }
                quat = quat_normalize(quat);
            }
            quat2mat(mat, quat);
        }
    }
    V3 gp;
    Q4 gq;
    fk_geom_pose(pos, quat, mat, D + h.o_mgd + 8 * l, gp, gq);       // lpos[3] lquat[4] rbound of moving geom l
    fk_geom_rec_st(grec + l * kGeomStride, gp, gq, D + h.o_g_rec + I[h.o_mg_geom + l] * kGeomStride);
}

// bit s of the result = state s (active coordinates m.qs[s]) is valid.  K3 inlines this body at its ONE call site (the
// planner's main loop is written so that there is only one, see k_rrt_connect): a call would cost the device ABI's
// callee-saved registers -- 41 VGPRs stored to and loaded from scratch memory around every pass once the kernel is held to
// the 256 registers of two waves per SIMD.  The pull-back kernel calls the non-inlined copy below.
template <bool FILL_PASSIVE>
__device__ __forceinline__ unsigned plan_states_valid_ms_body(const SceneHdr *hp, const double *dbl, const int *ints, double *ms_grec,
                                                              double *ms_qbuf, unsigned *ms_wl, const double *ms_qs, int lane, int ns,
                                                              const double *row) {
    MOPA_ASSUME_LDS(hp); MOPA_ASSUME_LDS(dbl); MOPA_ASSUME_LDS(ints); MOPA_ASSUME_LDS(ms_grec); MOPA_ASSUME_LDS(ms_qbuf);
    MOPA_ASSUME_LDS(ms_wl); MOPA_ASSUME_LDS(ms_qs);
    const SceneHdr &h = *hp;
    LdsView v0;
    v0.dbl = dbl; v0.ints = ints; v0.grec = nullptr; v0.qbuf = nullptr; v0.sc = nullptr; v0.wl = nullptr;
    MsLds m;
    m.grec = ms_grec; m.qbuf = ms_qbuf; m.wl = ms_wl; m.qs = const_cast<double *>(ms_qs);
    const int nq_s = h.na + h.n_pq, qstride = nq_s + ms_sc_doubles(h.nmj, h.nmb), gstride = h.nmg * kGeomStride;
    PLAN_T0();
    // (FILL_PASSIVE false: the caller wrote the passive slots of every slab once -- they do not change during a query, and
    //  `row` is global memory: a microsecond per pass for values that were there all along)
    if (FILL_PASSIVE) {
        for (int s = 0; s < ns; s++)
            for (int i = lane; i < nq_s; i += 64)
                m.qbuf[s * qstride + i] = (i < h.na) ? m.qs[s * h.na + i] : row[ints[h.o_pq_adr + i - h.na]];
    } else {
        for (int idx = lane; idx < ns * h.na; idx += 64) {
            const int s = idx / h.na, i = idx - s * h.na;
            m.qbuf[s * qstride + i] = m.qs[idx];
        }
    }
    wave_sync();
    PLAN_T(42);
    const bool pfk = h.pfk_maxlen > 0;
    if (pfk) {
        // joint table of all states, one (state, moving body) per lane: sin / cos of half the angle and the displacement of
        // the body's first joint
        for (int idx = lane; idx < ns * h.nmb; idx += 64) {
            const int s = idx / h.nmb, b = idx - s * h.nmb;
            double *qb = m.qbuf + s * qstride;
            const int *ri = ints + h.o_mbr + 8 * b;
            const int jn = ri[0], w7 = ri[7], jt0 = w7 & 0x7f;
            double sn = 0.0, cs = 1.0, dq = 0.0;
            if (jn > 0 && jt0 != J_FREE) {
                dq = qb[w7 >> 8] - dbl[h.o_mbd + 16 * b + 13];
                if (jt0 == J_HINGE) mopa_sincos(0.5 * dq, sn, cs);
            }
            qb[nq_s + 4 * b] = sn; qb[nq_s + 4 * b + 1] = cs; qb[nq_s + 4 * b + 2] = dq;
        }
    } else {
        for (int idx = lane; idx < ns * h.nmj; idx += 64) {       // sin/cos tables of all states, one (state, joint) per lane
            const int s = idx / h.nmj, j = idx - s * h.nmj;
            double *qb = m.qbuf + s * qstride;
            double sn = 0.0, cs = 1.0;
            if (ints[h.o_mj_type + j] == J_HINGE) mopa_sincos(0.5 * (qb[ints[h.o_mj_qsrc + j]] - dbl[h.o_mj_ref + j]), sn, cs);
            qb[nq_s + 2 * j] = sn;
            qb[nq_s + 2 * j + 1] = cs;
        }
    }
    wave_sync();
    PLAN_T(43);
    // forward kinematics: G lanes per state (G = 16 covers the 14-15 moving geoms of the Sawyer scenes)
    const int G = (h.nmg <= 16) ? 16 : ((h.nmg <= 32) ? 32 : 64);
    const int per_pass = 64 / G;
    for (int s0 = 0; s0 < ns; s0 += per_pass) {
        const int s = s0 + lane / G, l = lane % G;
        if (s < ns && l < h.nmg) {
            if (pfk) ms_fk(h, dbl, ints, m.qbuf + s * qstride, m.qbuf + s * qstride + nq_s, m.grec + s * gstride, l);
            else {
                LdsView v = v0;
                v.grec = m.grec + s * gstride;
                v.qbuf = m.qbuf + s * qstride;
                v.sc = v.qbuf + nq_s;
                fk_one_geom(h, v, l);
            }
        }
    }
    wave_sync();
    PLAN_T(0);
    return h.has_mesh ? ms_collide<true>(h, v0, m, lane, ns) : ms_collide<false>(h, v0, m, lane, ns);
}
// a query's passive joint values into every slab of the wave (the FILL_PASSIVE = false form's precondition)
MOPA_D void ms_fill_passive(const SceneHdr &h, const int *ints, double *ms_qbuf, int lane, const double *row) {
    const int nq_s = h.na + h.n_pq, qstride = nq_s + ms_sc_doubles(h.nmj, h.nmb);
    for (int idx = lane; idx < kMS * h.n_pq; idx += 64) {
        const int s = idx / h.n_pq, i = idx - s * h.n_pq;
        ms_qbuf[s * qstride + h.na + i] = row[ints[h.o_pq_adr + i]];
    }
    wave_sync();
}
__device__ __noinline__ unsigned plan_states_valid_ms(const SceneHdr *hp, const double *dbl, const int *ints, double *ms_grec,
                                                      double *ms_qbuf, unsigned *ms_wl, const double *ms_qs, int lane, int ns,
                                                      const double *row) {
    return plan_states_valid_ms_body<true>(hp, dbl, ints, ms_grec, ms_qbuf, ms_wl, ms_qs, lane, ns, row);
}
MOPA_D double wave_bcast_f64(double x, int src /*wave-uniform*/) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- wave reductions through DPP row rotations (an LDS-crossbar shuffle costs a lone wave ~64 clocks per step, three of them
// per (double, index) step of a butterfly; a DPP move ~5) ------------------------------------------------------------
template <int CTRL> MOPA_D int dpp_i32(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false); }
template <int CTRL> MOPA_D double dpp_f64(double x) {
    return __hiloint2double(dpp_i32<CTRL>(__double2hiint(x)), dpp_i32<CTRL>(__double2loint(x)));
}
MOPA_D int wave_min_i32(int v) {
    int o;
    o = dpp_i32<0x128>(v); v = o < v ? o : v;
    o = dpp_i32<0x124>(v); v = o < v ? o : v;
    o = dpp_i32<0x122>(v); v = o < v ? o : v;
    o = dpp_i32<0x121>(v); v = o < v ? o : v;
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16), r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    const int a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}
MOPA_D int wave_max_i32(int v) { return -wave_min_i32(-v); }
MOPA_D double wave_min_f64(double v) {
    double o;
    o = dpp_f64<0x128>(v); v = o < v ? o : v;
    o = dpp_f64<0x124>(v); v = o < v ? o : v;
    o = dpp_f64<0x122>(v); v = o < v ? o : v;
    o = dpp_f64<0x121>(v); v = o < v ? o : v;
    const double r0 = wave_bcast_f64(v, 0), r1 = wave_bcast_f64(v, 16), r2 = wave_bcast_f64(v, 32), r3 = wave_bcast_f64(v, 48);
    const double a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}
// the smallest (distance, index) pair of the wave: lowest index among the lanes that hold the smallest distance
MOPA_D int wave_argmin_f64(double bd, int bi) {
    const double m = wave_min_f64(bd);
    return wave_min_i32(bd == m ? bi : 0x7fffffff);
}

// The race's kernel-side declarations (everything else of the race is mopa_race.inc): the planner body names them.
struct RaceArgs {
    long long Eq;                  // queries of the launch (the kernel's E is Eq * K slots)
    int K;
    int no_abort;                  // nonzero: the comparison with the race word is off, every member runs to its own end
    unsigned long long *word;      // [Eq]
    long long *rec;                // [Eq * K][kRaceRec], slot order
};
constexpr int kRaceRec = 8;        // status | consumed checks | iterations | start motion | goal motion | rows of the solution | - | -
constexpr int kRaceCut = -100;     // record status of a member that stopped because it could no longer win
constexpr unsigned long long kRaceSeedStep = 0x9E3779B97F4A7C15ull;

// the planner body: k_rrt_connect<B> for the build tags K3W2, K3W1, K3WG and K3Race
#include "mopa_planner_k3.inc"


#ifdef MOPA_PLAN_STATS
// debug builds: the pose phases of a validity pass alone, `iters` times, one lone wave (tools/fk_bench.py)
__global__ __launch_bounds__(64) void k_debug_ms_fk(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                    const double *__restrict__ row, const double *__restrict__ qs, int ns, int iters,
                                                    unsigned long long *__restrict__ ticks, double *__restrict__ sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *s_dbl = reinterpret_cast<double *>(smem);
    int *s_int = reinterpret_cast<int *>(s_dbl + h.n_dbl);
    stage_scene(h, g_dbl, g_int, s_dbl, s_int);
    const int lane = threadIdx.x;
    const int nq_s = h.na + h.n_pq, qstride = nq_s + ms_sc_doubles(h.nmj, h.nmb), gstride = h.nmg * kGeomStride;
    double *grec = reinterpret_cast<double *>(s_int + ((h.n_int + 3) & ~3));
    double *qbuf = grec + kMS * gstride;
    double *lqs = qbuf + kMS * qstride;
    for (int i = lane; i < ns * h.na; i += 64) lqs[i] = qs[i];
    ms_fill_passive(h, s_int, qbuf, lane, row);
    unsigned long long t_fill = 0, t_tab = 0, t_fk = 0;
    for (int it = 0; it < iters; it++) {
        unsigned long long t0 = wall_clock64();
        for (int idx = lane; idx < ns * h.na; idx += 64) {
            const int s = idx / h.na, i = idx - s * h.na;
            qbuf[s * qstride + i] = lqs[idx];
        }
        wave_sync();
        unsigned long long t1 = wall_clock64();
        for (int idx = lane; idx < ns * h.nmb; idx += 64) {
            const int s = idx / h.nmb, b = idx - s * h.nmb;
            double *qb = qbuf + s * qstride;
            const int *ri = s_int + h.o_mbr + 8 * b;
            const int jn = ri[0], w7 = ri[7], jt0 = w7 & 0x7f;
            double sn = 0.0, cs = 1.0, dq = 0.0;
            if (jn > 0 && jt0 != J_FREE) {
                dq = qb[w7 >> 8] - s_dbl[h.o_mbd + 16 * b + 13];
                if (jt0 == J_HINGE) mopa_sincos(0.5 * dq, sn, cs);
            }
            qb[nq_s + 4 * b] = sn; qb[nq_s + 4 * b + 1] = cs; qb[nq_s + 4 * b + 2] = dq;
        }
        wave_sync();
        unsigned long long t2 = wall_clock64();
        {
            const int s = lane / 16, l = lane % 16;
            if (s < ns && l < h.nmg) ms_fk(h, s_dbl, s_int, qbuf + s * qstride, qbuf + s * qstride + nq_s, grec + s * gstride, l);
        }
        wave_sync();
        unsigned long long t3 = wall_clock64();
        t_fill += t1 - t0; t_tab += t2 - t1; t_fk += t3 - t2;
    }
    if (lane == 0) { ticks[0] = t_fill; ticks[1] = t_tab; ticks[2] = t_fk; }
    for (int i = lane; i < ns * gstride; i += 64) sink[i] = grec[i];
}
extern "C" int mopa_debug_fk_bench(MopaScene *S, const double *row_dev, const double *qs_dev, int ns, int iters, unsigned long long *ticks3, double *sink_dev) {
    if (!S) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the FK timing probe (mopa_debug_fk_bench)");
    ON_DEVICE(S->device);
    unsigned long long *d_t = nullptr;
    HIP_TRY(hipMalloc((void **)&d_t, 24));
    const SceneHdr &h = S->hdr;
    const int lds = h.n_dbl * 8 + ((h.n_int + 3) & ~3) * 4 + kMS * (h.nmg * kGeomStride + h.na + h.n_pq + ms_sc_doubles(h.nmj, h.nmb) + h.na) * 8 + 64;
    (void)hipFuncSetAttribute((const void *)k_debug_ms_fk, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    hipLaunchKernelGGL(k_debug_ms_fk, dim3(1), dim3(64), lds, nullptr, S->hdr, S->d_dbl, S->d_int, row_dev, qs_dev, ns, iters, d_t, sink_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ticks3, d_t, 24, hipMemcpyDeviceToHost));
    (void)hipFree(d_t);
    return MOPA_OK;
}
#endif

#ifdef MOPA_PLAN_STATS
extern "C" int mopa_debug_plan_times(unsigned long long *out48, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_plan_t), sizeof(unsigned long long) * 64));
    if (reset) { unsigned long long z[64] = {0}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_plan_t), z, sizeof(z))); }
    return MOPA_OK;
}
#endif

#ifdef MOPA_PLAN_STATS
extern "C" int mopa_debug_plan_mpr_pairs(unsigned *out8192, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out8192, HIP_SYMBOL(g_plan_mpr_pairs), sizeof(unsigned) * 8192));
    if (reset) { static unsigned z[8192]; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_plan_mpr_pairs), z, sizeof(z))); }
    return MOPA_OK;
}
#endif

// Launch geometry of the K3 builds that run four queries per workgroup (K3W2 / K3W1 / K3Race), worked out once for mopa_plan_batch
// and mopa_plan_race_batch: the LDS of a workgroup, the launch's counter, the workgroup count, the FP32 tree mirrors' share.
struct PlanGeom {
    int scene_bytes, lds;              // scene blobs; + the four waves' planner slabs + the header's copy
    int lds_launch, nn_cap;            // what the launch asks for; nodes per query that the FP32 tree mirror holds (nn_fast)
    int64_t nblk;
    unsigned long long *ctr;
};
// n queries (the race: slots).  `lone`: the launch keeps its CUs to itself whatever the parameters say and reads no A/B knob (the race,
// whose build holds one wave per SIMD: a CU holds one workgroup at a time).
static int plan_geometry(MopaScene *S, StreamScratch &sc, int64_t n, int max_workgroups, int max_nodes, bool lone, int exclusive_cu /* read unless lone */, PlanGeom &g) {
    if (!sc.plan_ctr.p) {       // [next query | waves done]: zeroed once, self-resetting afterwards (tile_ctr_release)
        HIP_TRY(grow(S, sc.plan_ctr, 64));
        HIP_TRY(hipMemset(sc.plan_ctr.p, 0, 64));       // (synchronously, once: see the validity kernels' counter in mopa_hip.hip)
        HIP_TRY(hipStreamSynchronize(nullptr));         // (a device memset may return before it has run)
    }
    g.ctr = sc.plan_ctr.as<unsigned long long>();
    const int per_wave = plan_vec_bytes(S->na) + ms_bytes_per_wave(S->hdr.nmg, S->na, S->hdr.n_pq, ms_sc_doubles(S->hdr.nmj, S->hdr.nmb), S->hdr.npair);
    // (the kernel poses states in its multi-state slabs only: the single-state slabs behind the scene blobs are not laid out)
    g.scene_bytes = S->lds_bytes - kWavesPerBlock * S->hdr.wave_bytes;
    const int lds = g.lds = g.scene_bytes + kWavesPerBlock * per_wave + (int)sizeof(SceneHdr);
    if (lds > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "planner LDS does not fit");
    // persistent workgroups: max_workgroups > 0 caps them, < 0 asks for as many as the chip holds at once (two per CU where
    // LDS allows: throughput, for launches that overlap others), 0 = one per CU -- a lone launch ends with its slowest
    // query, and two budget-exhausting queries on one SIMD slow each other down
    const int64_t resident = (int64_t)S->n_cu * (lone ? 1 : std::min(2, std::max(1, kMaxLdsBytes / lds)));
    // (a launch that keeps the chip to itself spreads few queries one per workgroup -- the kernel's first-query rule; launches that share
    //  it stay packed four to a workgroup: spread over every CU's LDS they block the launches they overlap with: ladder 478 -> 274 k plans/s)
    g.nblk = std::min<int64_t>(max_workgroups == 0 ? n : (n + kWavesPerBlock - 1) / kWavesPerBlock, resident);
    if (max_workgroups > 0) g.nblk = std::min<int64_t>(g.nblk, max_workgroups);
    else if (max_workgroups == 0) g.nblk = std::min<int64_t>(g.nblk, S->n_cu);
    // a launch of at most one workgroup per CU asks for more than half a CU's LDS: no second planner workgroup (of this or
    // of an overlapping launch) can then land on its CUs, whatever the dispatcher's placement
    bool excl = lone;
    if (!lone) {
        const char *ex = std::getenv("MOPA_PLAN_EXCLUSIVE");       // A/B knob: 0 = never, 1 = every launch of <= n_cu workgroups
        excl = ex ? (ex[0] == '1' && g.nblk <= S->n_cu) : (max_workgroups == 0 || exclusive_cu != 0);
    }
    g.lds_launch = excl ? std::max(lds, kMaxLdsBytes / 2 + 1024) : lds;
    // the rest of the launch's LDS share holds the FP32 tree mirrors of the workgroup's four queries (nn_fast)
    // (a launch that keeps its CUs to itself takes all of a CU's LDS; one that shares them two workgroups per CU, half)
    const int share = (g.lds_launch > lds || 2 * lds > kMaxLdsBytes) ? kMaxLdsBytes : kMaxLdsBytes / 2;
    const int mirror_off = lds + 16;
    g.nn_cap = ((share - mirror_off) / kWavesPerBlock / (4 * std::max(1, S->na))) & ~63;
    g.nn_cap = std::max(0, std::min(g.nn_cap, 2 * max_nodes));
    if (g.lds_launch <= kMaxLdsBytes / 2) g.nn_cap = 0;      // (the two-waves-per-SIMD build does not use the mirror)
    if (!lone)
        if (const char *ev = std::getenv("MOPA_PLAN_NN_CAP")) g.nn_cap = std::min(g.nn_cap, std::max(0, atoi(ev)) & ~63);      // A/B knob
    g.lds_launch = std::max(g.lds_launch, mirror_off + kWavesPerBlock * g.nn_cap * 4 * S->na);
    return MOPA_OK;
}

extern "C" int mopa_plan_batch(MopaScene *S, const double *start, const double *goal, int64_t E, const MopaPlanParams *params,
                               double *path, int32_t *path_len, int32_t *status, int64_t *n_checks, void *stream) {
    if (!S || !params || (E > 0 && (!start || !goal || !path || !path_len || !status)))
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E < 0 || params->max_nodes < 2 || params->max_path < 2 || params->max_iters < 0)
        return fail(MOPA_ERR_INVALID_ARG, "bad plan parameters");
    if ((params->tree_q_dev == nullptr) != (params->tree_p_dev == nullptr) || (params->state_dev && !params->tree_q_dev))
        return fail(MOPA_ERR_INVALID_ARG, "keeping planner state needs tree_q_dev, tree_p_dev and state_dev together");
    if (params->resume_state && (!params->resume_tree_q || !params->resume_tree_p))
        return fail(MOPA_ERR_INVALID_ARG, "resume_state needs resume_tree_q and resume_tree_p");
    if (S->glue_b >= 0 && (params->tree_q_dev || params->state_dev || params->resume_state))
        return fail(MOPA_ERR_UNSUPPORTED, "planner continuation (kept / resumed planner state) is not built for a glued scene (glue_bodies)");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    // glued scene: the start row attaches (passive values come from it, the goal row's free-joint slots are never read); k_glue_rows
    // behind the planner writes the carried body's pose into the free-joint columns of the solved paths
    const double *glue_att = nullptr;
    if (S->glue_b >= 0) {
        const int rc = glue_attach_scratch(S, start, E, (hipStream_t)stream, &glue_att);
        if (rc) return rc;
        start = glue_att;
    }
    StreamScratch &sc = scratch_for(S, (hipStream_t)stream);
    HIP_TRY(grow(S, sc.plan_q, (size_t)E * 2 * (size_t)params->max_nodes * S->na * sizeof(double) + 64));   // + pad: nn_node8 reads 8 doubles per node
    HIP_TRY(grow(S, sc.plan_p, (size_t)E * 2 * (size_t)params->max_nodes * sizeof(int32_t)));
    PlanWs ws{sc.plan_q.as<double>(), sc.plan_p.as<int32_t>()};
    PlanGeom g;
    if (const int rc = plan_geometry(S, sc, E, params->max_workgroups, params->max_nodes, false, params->exclusive_cu, g)) return rc;
    if (std::getenv("MOPA_DEBUG")) fprintf(stderr, "[mopa] plan launch: %lld queries, %lld workgroups, LDS %d + mirror %d nodes/query = %d bytes\n", (long long)E, (long long)g.nblk, g.lds, g.nn_cap, g.lds_launch);
    dim3 block(kBlock);
    // a launch that keeps its CUs to itself (lds_launch forces one workgroup per CU) runs a one-wave-per-SIMD build: the workgroup-per-
    // query one (K3WG: four waves on one query) where it applies, else four queries per workgroup (K3W1).  MOPA_PLAN_BUILD = w1 | w2 | wg
    // is the A/B knob (results are the same whatever runs).
    const bool lone = g.lds_launch > kMaxLdsBytes / 2;
    const char *bsel = std::getenv("MOPA_PLAN_BUILD");
    const int per_wave_wg = plan_vec_bytes_wg(S->na) + ms_bytes_per_wave(S->hdr.nmg, S->na, S->hdr.n_pq, ms_sc_doubles(S->hdr.nmj, S->hdr.nmb), S->hdr.npair);
    const int wg_mirror_off = g.scene_bytes + kWavesPerBlock * per_wave_wg + (((int)sizeof(SceneHdr) + 15) & ~15) + plan_wg_shared_bytes();
    const bool wg_fits = S->na <= 8 && wg_mirror_off + 64 * 4 * S->na <= kMaxLdsBytes;
    bool use_wg = lone && wg_fits;
    if (bsel && bsel[0] == 'w' && bsel[1] == 'g') use_wg = wg_fits;
    else if (bsel && bsel[0] == 'w' && (bsel[1] == '1' || bsel[1] == '2')) use_wg = false;
    if (use_wg) {
        int64_t nb = std::min<int64_t>(E, S->n_cu);
        if (params->max_workgroups > 0) nb = std::min<int64_t>(nb, params->max_workgroups);
        int cap = ((kMaxLdsBytes - wg_mirror_off) / (4 * std::max(1, S->na))) & ~63;
        cap = std::max(0, std::min(cap, (2 * params->max_nodes + 63) & ~63));
        if (const char *ev = std::getenv("MOPA_PLAN_NN_CAP")) cap = std::min(cap, std::max(0, atoi(ev)) & ~63);
        const int lds_wg = std::max(wg_mirror_off + cap * 4 * S->na, kMaxLdsBytes / 2 + 1024);
        if (std::getenv("MOPA_DEBUG")) fprintf(stderr, "[mopa] plan launch (workgroup per query): %lld queries, %lld workgroups, mirror %d nodes, LDS %d bytes\n", (long long)E, (long long)nb, cap, lds_wg);
        hipLaunchKernelGGL(k_rrt_connect<K3WG>, dim3((unsigned)nb), block, lds_wg, (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, start, goal, (long long)E,
                           *params, ws, path, path_len, status, (long long *)n_checks, g.scene_bytes, g.ctr, cap, K3NoArgs{});
    } else {
        const bool w1 = (bsel && bsel[0] == 'w' && bsel[1] == '2') ? false : lone;
        hipLaunchKernelGGL(w1 ? k_rrt_connect<K3W1> : k_rrt_connect<K3W2>, dim3((unsigned)g.nblk), block, g.lds_launch, (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, start, goal, (long long)E,
                           *params, ws, path, path_len, status, (long long *)n_checks, g.scene_bytes, g.ctr, g.nn_cap, K3NoArgs{});
    }
    HIP_TRY(hipGetLastError());
    if (glue_att) return mopa_glue_rows_batch(S, path, path_len, glue_att, E, params->max_path, stream);
    return MOPA_OK;
}

// The single-query host form of a planner entry (mopa_plan, mopa_plan_race, mopa_plan_star): one device block (start | goal | path |
// path length, status | the entry's further outputs, `extra_bytes` of them, 8-byte aligned), the batch entry on the default stream
// through `launch(start, goal, path, path_len, status, extra)`, then length and status, `copy_extra(extra)` and the path's rows back.
// Synchronous; the block is freed on every path.
template <class Launch, class CopyExtra>
static int plan_single(MopaScene *S, const double *start_host, const double *goal_host, int max_path, double *path_host, int32_t *path_len_out,
                       int32_t *status_out, size_t extra_bytes, Launch launch, CopyExtra copy_extra) {
    ON_DEVICE(S->device);
    const size_t nq = (size_t)S->nq, path_d = (size_t)max_path * nq;
    double *d_buf = nullptr;
    HIP_TRY(hipMalloc((void **)&d_buf, sizeof(double) * (2 * nq + path_d) + 8 + extra_bytes));
    double *d_start = d_buf, *d_goal = d_buf + nq, *d_path = d_buf + 2 * nq;
    int32_t *d_len = reinterpret_cast<int32_t *>(d_path + path_d), *d_status = d_len + 1;
    hipError_t e = hipMemcpy(d_start, start_host, sizeof(double) * nq, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_goal, goal_host, sizeof(double) * nq, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_buf); return fail(MOPA_ERR_HIP, hipGetErrorString(e)); }
    int rc = launch(d_start, d_goal, d_path, d_len, d_status, static_cast<void *>(d_len + 2));
    if (rc == MOPA_OK) {
        int32_t ls[2];
        e = hipMemcpy(ls, d_len, 8, hipMemcpyDeviceToHost);        // (the default stream: waits for the launch)
        if (e == hipSuccess) e = copy_extra(static_cast<const void *>(d_len + 2));
        if (e == hipSuccess && ls[0] > 0) e = hipMemcpy(path_host, d_path, sizeof(double) * (size_t)ls[0] * nq, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(MOPA_ERR_HIP, hipGetErrorString(e));
        else {
            *path_len_out = ls[0];
            *status_out = ls[1];
            // OMPL PlannerStatus::asString() equivalents (KinematicPlanner.cpp:189)
            S->status = (ls[1] == MOPA_PLAN_OK) ? "Exact solution" : (ls[1] == MOPA_PLAN_INVALID_GOAL ? "Invalid goal" : "Timeout");
        }
    }
    (void)hipFree(d_buf);
    return rc;
}

extern "C" int mopa_plan(MopaScene *S, const double *start_host, const double *goal_host, const MopaPlanParams *params,
                         double *path_host, int32_t *path_len_out, int32_t *status_out, int64_t *n_checks_out) {
    if (!S || !start_host || !goal_host || !params || !path_host || !path_len_out || !status_out)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MopaPlanParams one = *params;
    one.env_ids_dev = nullptr;   // single query: the stream id is env_id_base
    one.seeds_dev = nullptr;
    one.max_workgroups = 0;
    long long chk = 0;
    const int rc = plan_single(S, start_host, goal_host, params->max_path, path_host, path_len_out, status_out, 8,
        [&](const double *s, const double *g, double *p, int32_t *len, int32_t *st, void *x) { return mopa_plan_batch(S, s, g, 1, &one, p, len, st, (int64_t *)x, nullptr); },
        [&](const void *x) { return hipMemcpy(&chk, x, 8, hipMemcpyDeviceToHost); });
    if (rc == MOPA_OK && n_checks_out) *n_checks_out = chk;
    return rc;
}

// K3 race: RaceArgs, k_race_pick, mopa_plan_race_batch / mopa_plan_race
#include "mopa_race.inc"

static const LdsKernels kPlanLds({(const void *)k_rrt_connect<K3W2>, (const void *)k_rrt_connect<K3W1>, (const void *)k_rrt_connect<K3WG>,
                                  (const void *)k_rrt_connect<K3Race>});
