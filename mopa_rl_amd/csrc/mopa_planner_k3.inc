// mopa_planner_k3.inc -- the body of K3 (planner context, motion validation, nearest neighbour, speculation, growTree and the
// kernel), included once by mopa_planner.inc.  The kernel and the few helpers that differ between builds are templates over a
// build tag B; k_rrt_connect<B> is instantiated for four tags (their names are the kernels' names in traces and resource tables):
//   K3W2    kWaves 2: two waves per SIMD (256 registers) -- launches that share the chip (the ladder's first launches, the
//           rollouts' planner streams): a second wave on the SIMD is nearly free throughput.  The FP32 mirror sweeps (nn_fast)
//           are not instantiated and no first-query flag is kept.
//   K3W1    kWaves 1: one wave per SIMD (512 registers, nothing spilled) -- launches that keep their CUs to themselves (a lone
//           full-budget launch, retry launches): what counts there is the latency of one query.  A wave's first query is fixed
//           by its place; nearest neighbours go through the FP32 mirror in LDS.
//   K3WG    kWg (kWaves 1): ONE query per workgroup of four waves -- a budget-exhausting query alone on its CU gets all four
//           SIMDs.  Every wave runs the sequential algorithm (same data, same control flow, so no wave ever waits for another
//           outside a validity pass); AT a pass wave 0 evaluates the states the algorithm asks about while waves 1-3 work out
//           what the NEXT iterations will ask (their samples are known in advance: nearest node, steered state, first connect
//           state) and evaluate those.  Nearest neighbours and verdicts of future iterations wait in a small table (kFSlots
//           entries) and are used only when the sequential algorithm arrives at exactly that query / that state: results and
//           consumed-check counts cannot change.  Changes: the query fetch, the pass of plan_check_motion, the first
//           speculation and the table look-ups of plan_grow; only wave 0 writes outputs.
//   K3Race  kRace on the K3W1 settings (mopa_race.inc): launch slot v is member v / Eq of query v % Eq; a member leaves a
//           record instead of path rows and stops when the query's race word says that it can no longer win.  The kernel takes
//           one more argument (RaceArgs).
// Same source, same results; only register allocation and the `if constexpr` switches on the tag below differ.
struct K3W2 { static constexpr int kWaves = 2; static constexpr bool kWg = false, kRace = false; };
struct K3W1 { static constexpr int kWaves = 1; static constexpr bool kWg = false, kRace = false; };
struct K3WG { static constexpr int kWaves = 1; static constexpr bool kWg = true, kRace = false; };
struct K3Race { static constexpr int kWaves = 1; static constexpr bool kWg = false, kRace = true; };
struct K3NoArgs {};    // what the builds other than K3Race take in place of RaceArgs (mopa_planner.inc, in front of this file)
struct PlanCtx {
    LdsView v;
    const SceneHdr *lh;    // the scene header's copy in LDS (what the non-inlined validity routines read)
    int lane;
    const double *row;     // env's start qpos row (passive values)
    double *rs, *xs, *ns, *ts;   // LDS vectors [na]: target, steered, nearest, scratch
    double *r2;                  // LDS [na]: the NEXT iteration's sample (speculation)
    // Speculation (see plan_speculate): verdicts are a pure function of the state, so states the sequential
    // algorithm is LIKELY to ask about next ride along in the free slots of a validity pass; their verdicts are
    // kept here and consumed -- and counted -- only when the sequential algorithm really asks for that exact state.
    double *memo_q;              // LDS [kMemo][na]
    unsigned memo_ok;            // bit k = verdict of memo entry k
    int memo_cnt;                // entries written so far (ring position = memo_cnt % kMemo)
    double *spec_q;              // LDS [kSpec][na]
    int spec_n;
    double *nn_q;                // LDS [2][na]: queries whose nearest neighbour is already known
    int nn_tree0, nn_size0, nn_idx0, nn_tree1, nn_size1, nn_idx1;
    // FP32 mirror of the first nodes of both trees in LDS (nn_fast): [na][nn_cap] floats, tree 0 from slot 0 upwards, tree 1 from
    // the last slot downwards; nn_cnt = nodes mirrored per tree (always a prefix of the tree)
    float *nn_f;
    int nn_cap, nn_cnt0, nn_cnt1;
    float nn_eps2;               // 2 x (bound on |key - FP64 distance|): keys closer than this to the smallest are candidates
    uint64_t seed, stream, rng_k;   // rng_k = rng_key(seed, stream)
    int max_iters;
    unsigned long long so2;      // bit a = active coordinate a is an SO(2) angle (wraps)
#ifdef MOPA_PLAN_STATS
    long long st_pass = 0, st_states = 0, st_nn = 0;
#endif
    short *queue;          // LDS [2*kQCap]
    MsLds ms;              // multi-state validity slabs of this wave
    double *tq0, *tq1;     // this env's two trees (two named members, not arrays: an array indexed by the runtime
    int32_t *tp0, *tp1;    // tree id would put the whole context in scratch memory)
    int n0, n1;
    int cap;
    long long n_checks;
    int xmotion;
    bool overflow;
};
// the workgroup-per-query build's context (a type of its own: K3W1 and K3Race keep the context in their scratch frame, where members
// that those builds never touch would still take their 80 bytes per lane)
struct PlanCtxWg : PlanCtx {
    int wave;              // 0: evaluates what the algorithm asks; 1-3: future iterations
    double *ftab;          // LDS [kFSlots][kFStride], this wave's copy of the future table (all copies are equal)
    double *mbox;          // LDS, shared: [2 parities][4 waves][kMbStride]
    int pass_par;
    double *f0, *f1, *f2;  // LDS [8] scratch vectors of the speculation
    bool sp_pending;       // growTree of an iteration's first call wants the connect step's first state worked out at its pass
    int sp_it, cur_it, cur_role;
#ifdef MOPA_PLAN_STATS
    long long st_fnn = 0, st_fmemo = 0, st_fstates = 0, st_fast = 0, st_c0 = 0, st_c1 = 0, st_c2 = 0, st_c3 = 0;
#endif
};
template <class B> using K3Ctx = std::conditional_t<B::kWg, PlanCtxWg, PlanCtx>;

MOPA_D int tree_n(const PlanCtx &c, int t) { return t ? c.n1 : c.n0; }
MOPA_D double *tree_q(const PlanCtx &c, int t) { return t ? c.tq1 : c.tq0; }
MOPA_D int32_t *tree_p(const PlanCtx &c, int t) { return t ? c.tp1 : c.tp0; }

// K3's own non-inlined copy for its two cold checks (goal, start): a device function inherits a kernel's register limit only
// when ALL its callers carry it, and k_rrt_connect is held to two waves per SIMD while the pull-back kernel is not.
// (a template over the build tag for the same reason: one copy per build, called by that build's kernel alone)
template <class B>
__device__ __noinline__ unsigned plan_states_valid_ms_k3(const SceneHdr *hp, const double *dbl, const int *ints, double *ms_grec,
                                                         double *ms_qbuf, unsigned *ms_wl, const double *ms_qs, int lane, int ns,
                                                         const double *row) {
    return plan_states_valid_ms_body<false>(hp, dbl, ints, ms_grec, ms_qbuf, ms_wl, ms_qs, lane, ns, row);
}

// dist_dim / interp_dim with the wrap-around flag of the coordinate from the query's SO(2) mask (a register) instead of an LDS read
MOPA_D double k3_dist_dim(unsigned long long so2, int a, double x, double y) {
    double d = fabs(x - y);
    if (((so2 >> a) & 1ull) && d > kPi) d = 2.0 * kPi - d;
    return d;
}
MOPA_D double k3_interp_dim(unsigned long long so2, int a, double from, double to, double t) {
    double diff = to - from;
    if (!((so2 >> a) & 1ull) || fabs(diff) <= kPi) return fma(diff, t, from);
    if (diff > 0.0) diff = 2.0 * kPi - diff; else diff = -2.0 * kPi - diff;
    double r = fma(-diff, t, from);
    if (r > kPi) r -= 2.0 * kPi; else if (r < -kPi) r += 2.0 * kPi;
    return r;
}
// CompoundStateSpace::distance with unit weights = sum of the 1-D subspace distances
MOPA_D double plan_dist_l1(const SceneHdr &h, const LdsView &v, const double *a, const double *b) {
    double d = 0.0;
    for (int i = 0; i < h.na; i++) d += dist_dim(h, v, i, a[i], b[i]);
    return d;
}
// The same sum, in the same order, with the terms computed one per lane: the loop that is left is na dependent
// additions of broadcast values instead of na rounds of LDS reads + arithmetic.
MOPA_D double wave_dist_l1(const SceneHdr &h, const LdsView &v, int lane, unsigned long long so2, const double *a, const double *b) {
    if (h.na > 64) return plan_dist_l1(h, v, a, b);
    double t = 0.0;
    if (lane < h.na) {
        t = fabs(a[lane] - b[lane]);
        if (((so2 >> lane) & 1ull) && t > kPi) t = 2.0 * kPi - t;
    }
    double d = 0.0;
    for (int i = 0; i < h.na; i++) d += wave_bcast_f64(t, i);
    return d;
}
// validSegmentCount: the per-coordinate counts one per lane, their maximum by reduction (order-free)
MOPA_D int wave_segment_count(const SceneHdr &h, const LdsView &v, int lane, unsigned long long so2, const double *qa, const double *qb) {
    if (h.na > 64) return valid_segment_count(h, v, qa, qb);
    int c = 0;
    if (lane < h.na) {
        const double seg = h.resolution * v.dbl[h.o_act_ext + lane];
        c = (int)ceil(k3_dist_dim(so2, lane, qa[lane], qb[lane]) / seg);
    }
    c = wave_max_i32(c);
    return c < 0 ? 0 : c;
}

// ---- verdict memo / speculation queue ---------------------------------------------------------------------
MOPA_D bool plan_same_state(const PlanCtx &c, int na, const double *a, const double *b) {
    bool eq = true;
    if (c.lane < na) eq = __double_as_longlong(a[c.lane]) == __double_as_longlong(b[c.lane]);
    return __all(eq);
}
MOPA_D int memo_find(const SceneHdr &h, const PlanCtx &c, const double *q) {
    const int n = c.memo_cnt < kMemo ? c.memo_cnt : kMemo;
    if (h.na <= 8 && kMemo <= 8) {
        // all entries at once: lane = 8 * entry + coordinate, one ballot, a byte of the mask per entry
        const int k = c.lane >> 3, j = c.lane & 7;
        bool eq = true;
        if (j < h.na) eq = __double_as_longlong(c.memo_q[k * h.na + j]) == __double_as_longlong(q[j]);
        const unsigned long long m = __ballot(eq);
        for (int e = 0; e < n; e++)
            if (((m >> (8 * e)) & 0xffull) == 0xffull) return e;
        return -1;
    }
    for (int k = 0; k < n; k++)
        if (plan_same_state(c, h.na, c.memo_q + k * h.na, q)) return k;
    return -1;
}
MOPA_D void memo_put(const SceneHdr &h, PlanCtx &c, const double *q, bool ok) {
    const int k = c.memo_cnt % kMemo;
    if (c.lane < h.na) c.memo_q[k * h.na + c.lane] = q[c.lane];
    c.memo_ok = (c.memo_ok & ~(1u << k)) | ((ok ? 1u : 0u) << k);
    c.memo_cnt++;
    wave_sync();
}

// Brute-force nearest neighbour over a tree in HBM.  Up to 8 active coordinates (every scene of the reference) take
// the register path: the query lives in registers, a node is fetched as 8 doubles in one go (one memory latency per
// node; the 8th read may run into the next node -- the tree buffer is padded for the very last one) and missing
// coordinates are zeros on both sides, which add +0.0 to a non-negative sum: the distance is the same sum, in the same
// order, as plan_dist_l1.  No branch inside, so the two queries of the fused sweep interleave.
constexpr int kNnU = 4, kNnU2 = 2;   // nodes per trip: single query / fused two-query sweep
struct NnQuery { double q[8]; };
MOPA_D NnQuery nn_query(const double *q, int na) {
    NnQuery r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.q[j] = (j < na) ? q[j] : 0.0;
    return r;
}
MOPA_D void nn_node8(const double *p, int na, double (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = p[j];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = (j < na) ? x[j] : 0.0;
}
MOPA_D double nn_dist8(const double (&x)[8], const NnQuery &Q, unsigned long long so2) {
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const double dd = fabs(x[j] - Q.q[j]);
        const double wr = 2.0 * kPi - dd;
        const bool wrap = (((so2 >> j) & 1ull) != 0ull) & (dd > kPi);
        d += wrap ? wr : dd;
    }
    return d;
}
MOPA_D int plan_nearest(const SceneHdr &h, PlanCtx &c, int t, const double *q) {
    double bd = 1.0e300;
    int bi = 0x7fffffff;
    const int n = tree_n(c, t), na = h.na;
    const double *tq = tree_q(c, t);
    if (na <= 8) {
        const NnQuery Q = nn_query(q, na);
        for (int i = c.lane; i < n; i += 64 * kNnU) {   // kNnU nodes per trip: their fetches overlap
            double x[kNnU][8];
#pragma unroll
            for (int u = 0; u < kNnU; u++) {
                const int iu = i + 64 * u;
                nn_node8(tq + (size_t)(iu < n ? iu : i) * na, na, x[u]);
            }
#pragma unroll
            for (int u = 0; u < kNnU; u++) {
                const int iu = i + 64 * u;
                const double d = nn_dist8(x[u], Q, c.so2);
                if (iu < n && d < bd) { bd = d; bi = iu; }
            }
        }
    } else {
        for (int i = c.lane; i < n; i += 64) {
            const double d = plan_dist_l1(h, c.v, tq + (size_t)i * na, q);
            if (d < bd) { bd = d; bi = i; }
        }
    }
    return wave_argmin_f64(bd, bi);
}
// two queries in one sweep over tree t (same arithmetic per query as plan_nearest; each node is loaded once)
MOPA_D void plan_nearest2(const SceneHdr &h, PlanCtx &c, int t, const double *qa, const double *qb, int &ia, int &ib) {
    double bda = 1.0e300, bdb = 1.0e300;
    int bia = 0x7fffffff, bib = 0x7fffffff;
    const int n = tree_n(c, t), na = h.na;
    const double *tq = tree_q(c, t);
    if (na <= 8) {
        const NnQuery QA = nn_query(qa, na), QB = nn_query(qb, na);
        for (int i = c.lane; i < n; i += 64 * kNnU2) {
            double x[kNnU2][8];
#pragma unroll
            for (int u = 0; u < kNnU2; u++) {
                const int iu = i + 64 * u;
                nn_node8(tq + (size_t)(iu < n ? iu : i) * na, na, x[u]);
            }
#pragma unroll
            for (int u = 0; u < kNnU2; u++) {
                const int iu = i + 64 * u;
                const double da = nn_dist8(x[u], QA, c.so2), db = nn_dist8(x[u], QB, c.so2);
                if (iu < n && da < bda) { bda = da; bia = iu; }
                if (iu < n && db < bdb) { bdb = db; bib = iu; }
            }
        }
    } else {
        for (int i = c.lane; i < n; i += 64) {
            const double *p = tq + (size_t)i * na;
            const double da = plan_dist_l1(h, c.v, p, qa), db = plan_dist_l1(h, c.v, p, qb);
            if (da < bda) { bda = da; bia = i; }
            if (db < bdb) { bdb = db; bib = i; }
        }
    }
    ia = wave_argmin_f64(bda, bia);
    ib = wave_argmin_f64(bdb, bib);
}


// ---- nearest neighbour, fast form ---------------------------------------------------------------------------
// Every node gets an FP32 KEY within h.nn_eps of its FP64 distance: for the nodes mirrored in LDS (coordinates rounded to
// FP32, SoA, conflict-free reads) the L1 distance in FP32, for the tail of a tree that outgrew the mirror the FP64 distance
// of plan_dist_l1 rounded to FP32.  If exactly one node's key lies within 2 nn_eps of the smallest key, its FP64 distance is
// strictly the smallest -- it IS the node the exact sweep returns (ties cannot occur).  Otherwise (two candidates: a few
// sweeps in a thousand) the caller runs the exact FP64 sweep.  Results are therefore those of plan_nearest, bit for bit.
struct NnKey { float b1, b2; int i1; };
MOPA_D void nn_key_update(NnKey &k, float d, int i, bool live) {
    const bool better = live & (d < k.b1);
    const bool second = live & !better & (d < k.b2);
    k.b2 = better ? k.b1 : (second ? d : k.b2);
    k.b1 = better ? d : k.b1;
    k.i1 = better ? i : k.i1;
}
MOPA_D float wave_min_f32(float v) {
    // butterfly inside each DPP row of 16 lanes, then the four row results through scalar registers
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false)));
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false)));
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false)));
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false)));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
// index of the unique candidate, or -1 (ambiguous)
MOPA_D int nn_resolve(const NnKey &k, float eps2) {
    const float thr = wave_min_f32(k.b1) + eps2;
    const bool cand = k.b1 <= thr;
    const unsigned long long m = __ballot(cand);
    if (__popcll(m) != 1 || __any(cand && k.b2 <= thr)) return -1;
    return __builtin_amdgcn_readlane(k.i1, __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1));
}
// one mirrored node against one or two queries (NA > 0: that many coordinates, none an SO(2) angle -- the arm scenes; NA == 0:
// any na <= 8, wrap-around coordinates allowed)
template <bool TWO, int NA>
MOPA_D void nn_mirror_node(const PlanCtx &c, int na, int CAP, int slot, const float (&fa)[8], const float (&fb)[8], float &da, float &db) {
    const float PI_F = 3.14159265358979323846f;
    da = 0.f; db = 0.f;
    if (NA > 0) {
        float x[NA > 0 ? NA : 1];
#pragma unroll
        for (int j = 0; j < NA; j++) x[j] = c.nn_f[j * CAP + slot];
#pragma unroll
        for (int j = 0; j < NA; j++) {
            da += fabsf(x[j] - fa[j]);
            if (TWO) db += fabsf(x[j] - fb[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float x = c.nn_f[(j < na ? j : 0) * CAP + slot];
            const bool so2 = ((c.so2 >> j) & 1ull) != 0ull;
            float dd = fabsf(x - fa[j]);
            dd = (so2 & (dd > PI_F)) ? 2.f * PI_F - dd : dd;
            da += (j < na) ? dd : 0.f;
            if (TWO) {
                float de = fabsf(x - fb[j]);
                de = (so2 & (de > PI_F)) ? 2.f * PI_F - de : de;
                db += (j < na) ? de : 0.f;
            }
        }
    }
}
template <bool TWO, int NA>
MOPA_D void nn_mirror_sweep(const PlanCtx &c, int na, int t, int cnt, const double *qa, const double *qb, NnKey &ka, NnKey &kb) {
    const int CAP = c.nn_cap;
    float fa[8], fb[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { fa[j] = (j < na) ? (float)qa[j] : 0.f; fb[j] = (TWO && j < na) ? (float)qb[j] : 0.f; }
    for (int i = c.lane; i < cnt; i += 128) {       // two nodes per trip: their LDS reads overlap
        const int i2 = i + 64;
        const bool live2 = i2 < cnt;
        const int s1 = t ? CAP - 1 - i : i, s2 = live2 ? (t ? CAP - 1 - i2 : i2) : s1;
        float da1, db1, da2, db2;
        nn_mirror_node<TWO, NA>(c, na, CAP, s1, fa, fb, da1, db1);
        nn_mirror_node<TWO, NA>(c, na, CAP, s2, fa, fb, da2, db2);
        nn_key_update(ka, da1, i, true);
        nn_key_update(ka, da2, i2, live2);
        if (TWO) { nn_key_update(kb, db1, i, true); nn_key_update(kb, db2, i2, live2); }
    }
}
template <class B, bool TWO>
MOPA_D bool nn_fast(const SceneHdr &h, PlanCtx &c, int t, const double *qa, const double *qb, int &ia, int &ib) {
    if constexpr (B::kWaves == 2) return false;       // (256-register build: the sweep's registers would be spilled around every call; it keeps the FP64 sweeps)
    else {
        const int n = tree_n(c, t), na = h.na;
        if (na > 8) return false;
        const int cnt = t ? c.nn_cnt1 : c.nn_cnt0;
        NnKey ka{3.0e38f, 3.0e38f, 0x7fffffff}, kb{3.0e38f, 3.0e38f, 0x7fffffff};
        if (cnt > 0) {
            if (na == 7 && c.so2 == 0ull) nn_mirror_sweep<TWO, 7>(c, na, t, cnt, qa, qb, ka, kb);
            else nn_mirror_sweep<TWO, 0>(c, na, t, cnt, qa, qb, ka, kb);
        }
        if (cnt < n) {       // the part of the tree that is not mirrored: FP64 from HBM, as plan_nearest
            const double *tq = tree_q(c, t);
            const NnQuery QA = nn_query(qa, na), QB = nn_query(TWO ? qb : qa, na);
            for (int i = cnt + c.lane; i < n; i += 64 * kNnU2) {
                double x[kNnU2][8];
#pragma unroll
                for (int u = 0; u < kNnU2; u++) {
                    const int iu = i + 64 * u;
                    nn_node8(tq + (size_t)(iu < n ? iu : i) * na, na, x[u]);
                }
#pragma unroll
                for (int u = 0; u < kNnU2; u++) {
                    const int iu = i + 64 * u;
                    nn_key_update(ka, (float)nn_dist8(x[u], QA, c.so2), iu, iu < n);
                    if (TWO) nn_key_update(kb, (float)nn_dist8(x[u], QB, c.so2), iu, iu < n);
                }
            }
        }
        ia = nn_resolve(ka, c.nn_eps2);
        if (ia < 0) return false;
        if (TWO) {
            ib = nn_resolve(kb, c.nn_eps2);
            if (ib < 0) return false;
        }
        return true;
    }
}
// a node joins the mirror when every earlier node of its tree is in it and a slot is free
MOPA_D void nn_mirror_put(const SceneHdr &h, PlanCtx &c, int t, int i, const double *q /*[na]*/) {
    const int cnt = t ? c.nn_cnt1 : c.nn_cnt0;
    if (i != cnt || c.nn_cnt0 + c.nn_cnt1 >= c.nn_cap) return;
    const int slot = t ? c.nn_cap - 1 - i : i;
    if (c.lane < h.na) c.nn_f[c.lane * c.nn_cap + slot] = (float)q[c.lane];
    if (t) c.nn_cnt1++; else c.nn_cnt0++;
}

// ---- workgroup-per-query build: the future table (reached from the kWg branches only) ---------------------------
MOPA_D int wg_rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }
// FP64 distance of a tree node (global memory) from q (LDS): the sum of plan_dist_l1 / nn_dist8, same terms in the same order
MOPA_D double wg_dist_node(const SceneHdr &h, const PlanCtx &c, const double *node, const double *q) {
    double t = 0.0;
    if (c.lane < h.na) {
        t = fabs(node[c.lane] - q[c.lane]);
        if (((c.so2 >> c.lane) & 1ull) && t > kPi) t = 2.0 * kPi - t;
    }
    double d = 0.0;
    for (int i = 0; i < h.na; i++) d += wave_bcast_f64(t, i);
    return d;
}
// the state growTree creates from `node` towards `target` (both LDS): 0 = none (it would equal the node: trapped), 1 = steered state
// written to `out`, 2 = the target itself is within range (nothing written)
MOPA_D int wg_steer(const SceneHdr &h, const PlanCtx &c, const double *node, const double *target, double *out) {
    const double d = wave_dist_l1(h, c.v, c.lane, c.so2, node, target);
    if (!(d > h.range)) return 2;
    const double tt = h.range / d;
    double x = 0.0;
    bool same = true;
    if (c.lane < h.na) {
        x = k3_interp_dim(c.so2, c.lane, node[c.lane], target[c.lane], tt);
        same = !(fabs(x - node[c.lane]) > 2.0 * kCcdEps);
    }
    if (__all(same)) return 0;
    if (c.lane < h.na) out[c.lane] = x;
    wave_sync();
    return 1;
}
// nearest node of q among node `idx` (the nearest of the first `size` nodes) and the nodes size .. cur-1 of tree t: one candidate per
// lane, the arithmetic and the tie rule (lowest index) of plan_nearest
MOPA_D int wg_refine(const SceneHdr &h, PlanCtx &c, int t, const double *q, int idx, int size, int cur) {
    const NnQuery Q = nn_query(q, h.na);
    const bool live = c.lane <= cur - size;
    const int node = (c.lane == 0 || !live) ? idx : size + c.lane - 1;
    double x[8];
    nn_node8(tree_q(c, t) + (size_t)node * h.na, h.na, x);
    const double d = nn_dist8(x, Q, c.so2);
    return wave_argmin_f64(live ? d : 1.0e300, live ? node : 0x7fffffff);
}
// What the table knows for the sequential algorithm.  role 0: an iteration's first growTree (query = the iteration's sample, by
// construction of the entry); role 1: the first call of its connect step (query = the state the first call created, compared);
// anything else: nothing.  A tree that grew by a few nodes since the entry was made is caught up exactly: the recorded node is the
// nearest of the first `size` nodes (lowest index among equals), so only the new ones are compared -- strictly smaller wins, as in
// the sweep.
MOPA_D int wg_nn_lookup(const SceneHdr &h, PlanCtxWg &c, int t, int it, int role, const double *q) {
    if (role > 1) return -1;
    const double *e = c.ftab + (it & (kFSlots - 1)) * kFStride;
    const int *ei = reinterpret_cast<const int *>(e);
    if (wg_rfl(ei[0]) != it) return -1;
    const int fl = wg_rfl(ei[1]);
    int size, idx;
    if (role == 0) {
        if (!(fl & FF_NND)) return -1;
        size = wg_rfl(ei[2]); idx = wg_rfl(ei[3]);
    } else {
        if ((fl & (FF_NNC | FF_DS)) != (FF_NNC | FF_DS) || !plan_same_state(c, h.na, e + FO_D, q)) return -1;
        size = wg_rfl(ei[4]); idx = wg_rfl(ei[5]);
    }
    const int cur = tree_n(c, t);
    if (size > cur || cur - size > 32) return -1;
    if (size < cur) idx = wg_refine(h, c, t, q, idx, size, cur);
#ifdef MOPA_PLAN_STATS
    c.st_fnn++;
#endif
    return idx;
}
// verdict of `dstate` if the table holds exactly that state for this call: 0 / 1, else -1
MOPA_D int wg_memo_lookup(const SceneHdr &h, PlanCtxWg &c, int it, int role, const double *dstate) {
    if (role > 1) return -1;
    const double *e = c.ftab + (it & (kFSlots - 1)) * kFStride;
    const int *ei = reinterpret_cast<const int *>(e);
    if (wg_rfl(ei[0]) != it) return -1;
    const int fl = wg_rfl(ei[1]);
    int v = -1;
    if (role == 1 && (fl & (FF_C | FF_CS)) == (FF_C | FF_CS) && plan_same_state(c, h.na, e + FO_C, dstate)) v = (fl & FF_COK) ? 1 : 0;
    else if ((fl & (FF_D | FF_DS)) == (FF_D | FF_DS) && plan_same_state(c, h.na, e + FO_D, dstate)) v = (fl & FF_DOK) ? 1 : 0;   // (role 1: the connect step reaches the new state itself)
#ifdef MOPA_PLAN_STATS
    if (v >= 0) c.st_fmemo++;
#endif
    return v;
}
// which future iterations wave 1 / 2 / 3 takes at this pass: the not yet tabulated ones among it+1 .. it+kFSlots-1, in pairs of the same
// parity (their nearest-neighbour sweeps run over the same tree and are fused), the nearest iteration's parity first
MOPA_D void wg_assign(const SceneHdr &h, const PlanCtxWg &c, int it, int &ja, int &jb, unsigned &idle /* bit w: wave w has no iteration to work out */) {
    bool und = false;
    if (c.lane >= 1 && c.lane < kFSlots) {
        const int j = it + c.lane;
        und = j < c.max_iters && reinterpret_cast<const int *>(c.ftab + (j & (kFSlots - 1)) * kFStride)[0] != j;
    }
    const unsigned U = (unsigned)__ballot(und);
    ja = jb = -1;
    idle = 0xeu;
    if (!U) return;
    const unsigned PA = ((__ffs(U) - 1) & 1) ? 0xaaaaaaaau : 0x55555555u;
    unsigned UA = U & PA, UB = U & ~PA;
    auto pop = [](unsigned &m) -> int { if (!m) return -1; const int b = __ffs(m) - 1; m &= m - 1u; return b; };
    const int a1 = pop(UA), a2 = pop(UA), b1 = pop(UB), b2 = pop(UB);
    int c1, c2;
    if (UA) { c1 = pop(UA); c2 = pop(UA); } else { c1 = pop(UB); c2 = pop(UB); }
    const int x = c.wave == 1 ? a1 : (c.wave == 2 ? b1 : c1), y = c.wave == 1 ? a2 : (c.wave == 2 ? b2 : c2);
    if (x >= 0) ja = it + x;
    if (y >= 0) jb = it + y;
    idle = (a1 < 0 ? 2u : 0u) | (b1 < 0 ? 4u : 0u) | (c1 < 0 ? 8u : 0u);
}
// PREPARES iterations ja (and jb, same parity, or -1) as far as the current trees tell: nearest node of the sample, the state D the
// first growTree creates (and the interior state of its motion if that has two segments), nearest node of D in the other tree, the
// connect step's first state CF (and its interior state).  The two entries go to the wave's mailbox block `mb`; nothing is evaluated
// here -- after the pass's first barrier every wave has every entry and the states without a verdict are shared out over all sixteen
// slots of the workgroup (wg_complete).  Da_given (wave 0): iteration ja's D is the state the algorithm is testing now -- only its
// connect step is prepared (Da_valid: its verdict is already known to be "valid").
template <class B>
MOPA_D void wg_speculate(const SceneHdr &h, PlanCtxWg &c, int ja, int jb, const double *Da_given, bool Da_valid, double *mb, int &n_ent) {
    const int na = h.na, lane = c.lane;
    double *ea = mb + kMbHdr, *eb = ea + kFStride;
    int *ia = reinterpret_cast<int *>(ea), *ib = reinterpret_cast<int *>(eb);
    const bool two = jb >= 0;
    const int t = ja & 1, o = 1 - t;
    int fa = 0, fb = 0;
    bool a_live = true, b_live = two;
    const double *Da = ea + FO_D, *Db = eb + FO_D;
    if (Da_given) {
        const double *e = c.ftab + (ja & (kFSlots - 1)) * kFStride;
        const int *ei = reinterpret_cast<const int *>(e);
        const int fl = wg_rfl(ei[1]);
        if (wg_rfl(ei[0]) == ja && (fl & (FF_NNC | FF_DS)) == (FF_NNC | FF_DS) && plan_same_state(c, na, e + FO_D, Da_given)) { n_ent = 0; return; }
        if (lane < na) ea[FO_D + lane] = Da_given[lane];
        wave_sync();
        fa |= FF_DS | (Da_valid ? (FF_D | FF_DOK) : 0);
    }
    for (int stage = Da_given ? 1 : 0; stage < 2; stage++) {
        const int tr = stage ? o : t;
        if (stage == 0) {
            if (lane < na) {
                const double lo = c.v.dbl[h.o_act_lo + lane], hi = c.v.dbl[h.o_act_hi + lane];
                c.f0[lane] = fma(hi - lo, rng_uniform_k(c.rng_k, (uint64_t)ja * na + lane), lo);
                c.f1[lane] = fma(hi - lo, rng_uniform_k(c.rng_k, (uint64_t)(two ? jb : ja) * na + lane), lo);
            }
            wave_sync();
        } else if (!a_live && !b_live) break;
        const double *q0 = stage ? (a_live ? Da : Db) : c.f0;
        const double *q1 = stage ? (b_live ? Db : Da) : c.f1;
        int i0, i1;
        if (!nn_fast<B, true>(h, c, tr, q0, q1, i0, i1)) plan_nearest2(h, c, tr, q0, q1, i0, i1);
        const int sz = tree_n(c, tr);
        for (int x = 0; x < 2; x++) {
            if (!(x ? b_live : a_live)) continue;
            double *e = x ? eb : ea;
            int *ei = x ? ib : ia;
            int &fl = x ? fb : fa;
            const int idx = x ? i1 : i0;
            const double *target = stage ? (x ? Db : Da) : (x ? c.f1 : c.f0);
            if (lane == 0) { ei[stage ? 4 : 2] = sz; ei[stage ? 5 : 3] = idx; }
            fl |= stage ? FF_NNC : FF_NND;
            if (lane < na) c.f2[lane] = tree_q(c, tr)[(size_t)idx * na + lane];
            wave_sync();
            double *out = e + (stage ? FO_C : FO_D);
            const int r = wg_steer(h, c, c.f2, target, out);
            if (r == 0) {
                fl |= stage ? FF_CTRAP : FF_DTRAP;
                if (stage == 0) { if (x) b_live = false; else a_live = false; }
                continue;
            }
            if (r == 2) {
                if (lane < na) out[lane] = target[lane];
                wave_sync();
            }
            fl |= stage ? (FF_CS | (r == 2 ? FF_CREACH : 0)) : (FF_DS | (r == 2 ? FF_DREACH : 0));
            const int nd = wave_segment_count(h, c.v, lane, c.so2, c.f2, out);
            if (lane == 0) ei[stage ? 7 : 6] = nd;
            bool ok_known = false, ok = true;
            if (!(stage && r == 2)) {      // (a connect step that reaches D itself: D is in the tree by then)
                const int mk = memo_find(h, c, out);
                if (mk >= 0) {
                    ok_known = true;
                    ok = ((c.memo_ok >> mk) & 1u) != 0u;
                    fl |= stage ? (FF_C | (ok ? FF_COK : 0)) : (FF_D | (ok ? FF_DOK : 0));
                }
            }
            if (stage == 0 && (tree_n(c, t) >= c.cap || (ok_known && !ok))) { if (x) b_live = false; else a_live = false; }
            if (nd == 2 && !(ok_known && !ok) && !(Da_given && stage == 0)) {
                // DiscreteMotionValidator's interior state of a two-segment motion a -> b: interpolate(a, b, 1/2), a = the tree node when the
                // START tree grows, the new state when the goal tree does (plan_grow's call of plan_check_motion)
                double *oi = e + (stage ? FO_IC : FO_ID);
                const bool from_node = tr == 0;
                if (lane < na) oi[lane] = k3_interp_dim(c.so2, lane, from_node ? c.f2[lane] : out[lane], from_node ? out[lane] : c.f2[lane], 1.0 / 2.0);
                wave_sync();
                fl |= stage ? FF_CIS : FF_DIS;
                const int mk = memo_find(h, c, oi);
                if (mk >= 0) fl |= (stage ? FF_CI : FF_DI) | (((c.memo_ok >> mk) & 1u) ? (stage ? FF_CIOK : FF_DIOK) : 0);
            }
        }
    }
    if (lane == 0) { ia[0] = ja; ia[1] = fa; ib[0] = jb; ib[1] = fb; }
    n_ent = two ? 2 : 1;
    wave_sync();
}
// after the pass's first barrier: every wave copies every wave's entries into its own table (slot = iteration modulo kFSlots; the
// iterations of one pass are distinct modulo kFSlots: the current one and futures up to it+kFSlots-1)
MOPA_D void wg_merge(PlanCtxWg &c) {
    const double *base = c.mbox + (size_t)(c.pass_par * kWavesPerBlock) * kMbStride;
    for (int idx = c.lane; idx < kWavesPerBlock * 2 * kFStride; idx += 64) {
        const int ent = idx / kFStride, word = idx - ent * kFStride;
        const double *wb = base + (size_t)(ent >> 1) * kMbStride;
        if ((ent & 1) < reinterpret_cast<const int *>(wb)[2]) {
            const double *src = wb + kMbHdr + (ent & 1) * kFStride;
            const int tag = reinterpret_cast<const int *>(src)[0];
            c.ftab[(tag & (kFSlots - 1)) * kFStride + word] = src[word];
        }
    }
    wave_sync();
}
// The states the table holds without a verdict, shared out over the workgroup's batches.  Every wave lists the same candidates --
// iterations it .. it+kFSlots-1, nearest first; D, its interior state, CF, its interior state in that order (of the current iteration
// only the connect step: its D is what the algorithm is testing) -- and takes its share from the top: wave 0 what its own batch leaves
// (cap0), then four each for waves 1, 2, 3.  What a wave takes it records in its mailbox header (iteration, kind).
MOPA_D void wg_complete(const SceneHdr &h, PlanCtxWg &c, int it, double *mb, int &ns, int &n_comp, unsigned &comp_slots, int cap0) {
    n_comp = 0; comp_slots = 0u;
    int m = 0;
    if (c.lane < kFSlots) {
        const int j = it + c.lane;
        const int *ei = reinterpret_cast<const int *>(c.ftab + (j & (kFSlots - 1)) * kFStride);
        if (ei[0] == j) {
            const int fl = ei[1];
            const bool dead = (fl & FF_D) && !(fl & FF_DOK);      // D is known to be invalid: nothing else of the iteration will be asked
            if (c.lane > 0 && (fl & FF_DS) && !(fl & FF_D)) m |= 1;
            if (c.lane > 0 && !dead && (fl & FF_DIS) && !(fl & FF_DI)) m |= 2;
            if (!dead && (fl & FF_CS) && !(fl & (FF_C | FF_CREACH))) m |= 4;
            if (!dead && (fl & FF_CIS) && !(fl & FF_CI)) m |= 8;
        }
    }
    unsigned long long any = __ballot(m != 0);
    const int lo = c.wave == 0 ? 0 : cap0 + kMS * (c.wave - 1), hi = c.wave == 0 ? cap0 : lo + kMS;
    int *mbi = reinterpret_cast<int *>(mb);
    int g = 0;
    while (any && g < hi) {
        const int k = (int)__ffsll((long long)any) - 1;
        any &= any - 1ull;
        int mk = __builtin_amdgcn_readlane(m, k);
        const int j = it + k;
        const double *e = c.ftab + (j & (kFSlots - 1)) * kFStride;
        for (; mk && g < hi; g++) {
            const int kind = __ffs(mk) - 1;
            mk &= mk - 1;
            if (g < lo) continue;
            const double *src = e + (kind == 0 ? FO_D : (kind == 1 ? FO_ID : (kind == 2 ? FO_C : FO_IC)));
            if (c.lane < h.na) c.ms.qs[ns * h.na + c.lane] = src[c.lane];
            if (c.lane == 0) { mbi[4 + 2 * n_comp] = j; mbi[5 + 2 * n_comp] = kind; }
            comp_slots |= (unsigned)ns << (4 * n_comp);
            n_comp++; ns++;
        }
    }
    wave_sync();
}
// header of this wave's mailbox block: its batch's verdict bits, and the verdicts of the table states it took as flag bits
MOPA_D void wg_publish(const PlanCtxWg &c, double *mb, int my_ns, unsigned my_ok, int n_comp, unsigned comp_slots) {
    if (c.lane == 0) {
        int *mbi = reinterpret_cast<int *>(mb);
        mbi[0] = my_ns; mbi[1] = (int)my_ok; mbi[3] = n_comp;
        for (int r = 0; r < n_comp; r++) {
            const int kind = mbi[5 + 2 * r];
            const bool v = ((my_ok >> ((comp_slots >> (4 * r)) & 15u)) & 1u) != 0u;
            mbi[5 + 2 * r] = kind == 0 ? (FF_D | (v ? FF_DOK : 0)) : (kind == 1 ? (FF_DI | (v ? FF_DIOK : 0)) : (kind == 2 ? (FF_C | (v ? FF_COK : 0)) : (FF_CI | (v ? FF_CIOK : 0))));
        }
    }
}
// after the pass's second barrier: the verdicts every wave found, into this wave's table
MOPA_D void wg_apply(PlanCtxWg &c) {
    const double *base = c.mbox + (size_t)(c.pass_par * kWavesPerBlock) * kMbStride;
    if (c.lane < 4 * kWavesPerBlock) {
        const int *wh = reinterpret_cast<const int *>(base + (size_t)(c.lane >> 2) * kMbStride);
        const int r = c.lane & 3;
        if (r < wh[3]) {
            const int tag = wh[4 + 2 * r];
            int *fw = reinterpret_cast<int *>(c.ftab + (tag & (kFSlots - 1)) * kFStride);
            if (fw[0] == tag) atomicOr(fw + 1, wh[5 + 2 * r]);
        }
    }
    wave_sync();
}

// OMPL DiscreteMotionValidator::checkMotion(a, b), optionally preceded by isValid(pre) (growTree tests the new
// state before the motion when it grows the goal tree).  OMPL's order -- [pre], end state b, then the interior
// states in breadth-first bisection order -- is kept; the states are evaluated kMS at a time and the count of
// consumed checks is what the sequential loop would have consumed (up to and including the first invalid one).
// Free slots of a pass carry the queued speculative states (c.spec_q); a lead state whose verdict is already in
// the memo is counted but not evaluated again.
template <class B>
MOPA_D bool plan_check_motion(const SceneHdr &h, K3Ctx<B> &c, const double *a, const double *b, const double *pre, int lead_v /* verdict of the lead state if known: 0 / 1, else -1 */) {
    const int na = h.na;
    const double *lead = pre ? pre : b;
    bool lead_known = false;
    // with `pre`, b is a node of the tree: valid by construction (every node was validated before it was added), so
    // it is COUNTED where the sequential validator would test it -- right after a valid `pre` -- but not evaluated
    bool b_pending = pre != nullptr;
    if (lead_v >= 0) {       // verdict of `lead` known (looked up by the caller)
        c.n_checks++;
        if (!lead_v) return false;
        lead_known = true;
        if (b_pending) { c.n_checks++; b_pending = false; }
    }
    const int nd = wave_segment_count(h, c.v, c.lane, c.so2, a, b);
    const bool overflow = nd > kQCap;
    int head = 0, tail = 0;
    if (nd >= 2 && !overflow) { c.queue[0] = 1; c.queue[1] = (short)(nd - 1); tail = 1; }
    wave_sync();
    bool first = true;
    for (;;) {
        // fill up to kMS states in order
        int ns = 0;
        bool lead_in_batch = false;
        if (first) {
            if (!lead_known) { if (c.lane < na) c.ms.qs[ns * na + c.lane] = lead[c.lane]; ns++; }
            lead_in_batch = !lead_known;
            first = false;
        }
        while (ns < kMS && head < tail) {
            const int lo = c.queue[2 * head], hi = c.queue[2 * head + 1];
            const int mid = (lo + hi) / 2;
            const double t = (double)mid / (double)nd;
            if (c.lane < na) c.ms.qs[ns * na + c.lane] = k3_interp_dim(c.so2, c.lane, a[c.lane], b[c.lane], t);
            ns++;
            head++;
            wave_sync();   // queue reads above happen before the pushes below (same LDS array)
            if (lo < mid) { c.queue[2 * tail] = (short)lo; c.queue[2 * tail + 1] = (short)(mid - 1); tail++; }
            if (hi > mid) { c.queue[2 * tail] = (short)(mid + 1); c.queue[2 * tail + 1] = (short)hi; tail++; }
            wave_sync();
        }
        if (ns == 0) return !overflow;
        const int ns_real = ns;
        int n_spec = 0;
        while (ns < kMS && n_spec < c.spec_n) {
            if (c.lane < na) c.ms.qs[ns * na + c.lane] = c.spec_q[n_spec * na + c.lane];
            ns++; n_spec++;
        }
        wave_sync();
        unsigned ok;
        if constexpr (B::kWg) {
            // every wave arrives here with the same batch; wave 0 evaluates it (plus the connect step's first state), the others replace
            // it by states of future iterations; one barrier, then every wave takes wave 0's verdicts and files everybody's findings
            double *mb = c.mbox + (size_t)(c.pass_par * kWavesPerBlock + c.wave) * kMbStride;
            int n_ent = 0, ja, jb;
            unsigned idle;
            wg_assign(h, c, c.cur_it, ja, jb, idle);
            if (c.wave == 0) {
                if (c.sp_pending) wg_speculate<B>(h, c, c.sp_it, -1, lead, !lead_in_batch, mb, n_ent);
            } else if (ja >= 0) wg_speculate<B>(h, c, ja, jb, nullptr, false, mb, n_ent);
            if (c.lane == 0) reinterpret_cast<int *>(mb)[2] = n_ent;
            __syncthreads();
            wg_merge(c);
            int my_ns = c.wave == 0 ? ns : 0, n_comp;
            unsigned comp_slots;
            wg_complete(h, c, c.cur_it, mb, my_ns, n_comp, comp_slots, kMS - ns);
            unsigned my_ok = 0;
            if (my_ns > 0) my_ok = plan_states_valid_ms_body<false>(c.lh, c.v.dbl, c.v.ints, c.ms.grec, c.ms.qbuf, c.ms.wl, c.ms.qs, c.lane, my_ns, c.row);
            wg_publish(c, mb, my_ns, my_ok, n_comp, comp_slots);
            __syncthreads();
            const int *hdr0 = reinterpret_cast<const int *>(c.mbox + (size_t)(c.pass_par * kWavesPerBlock) * kMbStride);
            ok = (unsigned)__builtin_amdgcn_readfirstlane(hdr0[1]);
            wg_apply(c);
            c.pass_par ^= 1;
            c.sp_pending = false;
#ifdef MOPA_PLAN_STATS
            c.st_fstates += my_ns;
            { const int cause = lead_in_batch ? c.cur_role : 3; if (cause == 0) c.st_c0++; else if (cause == 1) c.st_c1++; else if (cause == 2) c.st_c2++; else c.st_c3++; }
#endif
        } else ok = plan_states_valid_ms_body<false>(c.lh, c.v.dbl, c.v.ints, c.ms.grec, c.ms.qbuf, c.ms.wl, c.ms.qs, c.lane, ns, c.row);
#ifdef MOPA_PLAN_STATS
        c.st_pass++; c.st_states += ns;
#endif
        for (int k = 0; k < n_spec; k++) memo_put(h, c, c.spec_q + k * na, (ok >> (ns_real + k)) & 1u);
        if (n_spec) c.spec_n = 0;
        if (lead_in_batch) memo_put(h, c, lead, ok & 1u);
        const unsigned bad = ~ok & ((1u << ns_real) - 1u);
        if (b_pending) {       // first batch, slot 0 = pre
            if (!(bad & 1u)) c.n_checks++;
            b_pending = false;
        }
        if (bad) {
            c.n_checks += __ffs(bad);   // the sequential validator stops at the first invalid state
            return false;
        }
        c.n_checks += ns_real;
        if (overflow) { c.overflow = true; return false; }
    }
}

// queue the state growTree would create from node nm of tree t towards `target` (nothing if it would be rejected
// as equal to the node, or if it IS the target and `skip_target`)
MOPA_D void spec_push_steer(const SceneHdr &h, PlanCtx &c, int t, int nm, const double *target, bool skip_target) {
    if (c.spec_n >= kSpec) return;
    const int na = h.na;
    if (c.lane < na) c.ts[c.lane] = tree_q(c, t)[(size_t)nm * na + c.lane];
    wave_sync();
    const double d = wave_dist_l1(h, c.v, c.lane, c.so2, c.ts, target);
    double *out = c.spec_q + c.spec_n * na;
    if (d > h.range) {
        const double tt = h.range / d;
        double x = 0.0;
        bool same = true;
        if (c.lane < na) {
            x = k3_interp_dim(c.so2, c.lane, c.ts[c.lane], target[c.lane], tt);
            same = !(fabs(x - c.ts[c.lane]) > 2.0 * kCcdEps);
        }
        if (__all(same)) return;
        if (c.lane < na) out[c.lane] = x;
    } else {
        if (skip_target) return;
        if (c.lane < na) out[c.lane] = target[c.lane];
    }
    c.spec_n++;
    wave_sync();
}

enum { SPEC_NONE = 0, SPEC_FIRST = 1, SPEC_CONNECT = 2 };

// What the algorithm will most likely ask next, queued before the validity pass of this growTree call:
//  SPEC_FIRST   (first growTree of iteration `it`, tree t, new state dstate): the first state of the connect step
//               (other tree's nearest node steered towards dstate) and the new state of iteration it+1 (which
//               grows the other tree from ITS sample) -- one fused nearest-neighbour sweep over the other tree,
//               whose results are kept for the calls that will ask for them (valid while that tree has not grown);
//  SPEC_CONNECT (greedy connect towards c.rs): the next states along the straight line, assuming the state
//               added now is the nearest node next time.
// A wrong guess costs a slot of a pass that runs anyway; verdicts are looked up by exact state, so it can
// never change a result.
template <class B>
MOPA_D void plan_speculate(const SceneHdr &h, K3Ctx<B> &c, int mode, int t, const double *dstate, bool reach, int it) {
    const int na = h.na;
    c.spec_n = 0;
    if constexpr (B::kWg) {
        if (mode == SPEC_FIRST) {       // worked out AT the pass, by wave 0, next to the other waves' future iterations (wg_speculate)
            c.sp_pending = true; c.sp_it = it;
            return;
        }
    }
    if (mode == SPEC_FIRST) {
        const int o = 1 - t;
        const bool want2 = it + 1 < c.max_iters;
        if (want2 && c.lane < na) {
            const double lo = c.v.dbl[h.o_act_lo + c.lane], hi = c.v.dbl[h.o_act_hi + c.lane];
            c.r2[c.lane] = fma(hi - lo, rng_uniform_k(c.rng_k, (uint64_t)(it + 1) * na + c.lane), lo);
        }
        if (c.lane < na) c.nn_q[c.lane] = dstate[c.lane];
        wave_sync();
        if (want2 && c.lane < na) c.nn_q[na + c.lane] = c.r2[c.lane];
        wave_sync();
        int ia, ib;
        const int lane = c.lane; (void)lane;
        { PLAN_T0();
        if (!(want2 ? nn_fast<B, true>(h, c, o, c.nn_q, c.nn_q + na, ia, ib) : nn_fast<B, false>(h, c, o, c.nn_q, c.nn_q, ia, ib))) {
#ifdef MOPA_PLAN_STATS
            if (threadIdx.x == 0) atomicAdd(&g_plan_t[47], 1ull);
#endif
            plan_nearest2(h, c, o, c.nn_q, want2 ? c.nn_q + na : c.nn_q, ia, ib);
        } else if (!want2) ib = ia;
        PLAN_T(22); }
        PLAN_T0();
        c.nn_tree0 = o; c.nn_size0 = tree_n(c, o); c.nn_idx0 = ia;
        c.nn_tree1 = want2 ? o : -1; c.nn_size1 = tree_n(c, o); c.nn_idx1 = ib;
        spec_push_steer(h, c, o, ia, c.nn_q, true);
        if (want2) spec_push_steer(h, c, o, ib, c.nn_q + na, false);
        PLAN_T(23);
    } else if (mode == SPEC_CONNECT && !reach) {
        const int lane = c.lane; (void)lane;
        PLAN_T0();
        // cur = dstate; next = steer(cur -> rs); ...
        const double *cur = dstate;
        for (int k = 0; k < kSpec; k++) {
            const double d = wave_dist_l1(h, c.v, c.lane, c.so2, cur, c.rs);
            double *out = c.spec_q + c.spec_n * na;
            if (!(d > h.range)) break;          // the step after `cur` reaches rs, whose verdict is known
            const double tt = h.range / d;
            double x = 0.0;
            bool same = true;
            if (c.lane < na) {
                x = k3_interp_dim(c.so2, c.lane, cur[c.lane], c.rs[c.lane], tt);
                same = !(fabs(x - cur[c.lane]) > 2.0 * kCcdEps);
            }
            if (__all(same)) break;
            if (c.lane < na) out[c.lane] = x;
            c.spec_n++;
            wave_sync();
            cur = out;
        }
        PLAN_T(38);
    }
}
MOPA_D int nn_known(const SceneHdr &h, const PlanCtx &c, int t, const double *q) {
    if (c.nn_tree0 == t && c.nn_size0 == tree_n(c, t) && plan_same_state(c, h.na, c.nn_q, q)) return c.nn_idx0;
    if (c.nn_tree1 == t && c.nn_size1 == tree_n(c, t) && plan_same_state(c, h.na, c.nn_q + h.na, q)) return c.nn_idx1;
    return -1;
}

// a validated state joins tree t behind node nm
MOPA_D void plan_append(const SceneHdr &h, PlanCtx &c, int t, int nm, const double *dstate) {
    if (c.lane < h.na) tree_q(c, t)[(size_t)tree_n(c, t) * h.na + c.lane] = dstate[c.lane];
    if (c.lane == 0) tree_p(c, t)[tree_n(c, t)] = nm;
    nn_mirror_put(h, c, t, tree_n(c, t), dstate);
    __threadfence_block();
    wave_sync();
    c.xmotion = tree_n(c, t);
    if (t) c.n1++; else c.n0++;
}

// OMPL RRTConnect::growTree(tree, tgi, rmotion)
template <class B>
MOPA_D int plan_grow(const SceneHdr &h, K3Ctx<B> &c, int t, bool is_start, int spec_mode, int it, int role /* K3WG: 0 = the iteration's first call, 1 = first call of its connect step, 2 = later ones */) {
    const int lane = c.lane; (void)lane;
    int nm;
    if constexpr (B::kWg) {
        c.sp_pending = false;
        c.cur_role = role;
        if (role <= 1) {
            // the whole call from the table: nearest node unchanged (tree as it was) -> the steering outcome, the state, the segment count
            // of its motion and (if it was evaluated) its verdict are the ones recorded; what is left is the bookkeeping of growTree
            PLAN_T0();
            const double *e = c.ftab + (it & (kFSlots - 1)) * kFStride;
            const int4 e03 = *reinterpret_cast<const int4 *>(e), e47 = *reinterpret_cast<const int4 *>(e + 2);      // the entry's eight ints in one go
            const int fl = wg_rfl(e03.y);
            const int need = role ? (FF_NNC | FF_DS) : FF_NND;
            const int cur = tree_n(c, t), size = wg_rfl(role ? e47.x : e03.z);
            if (wg_rfl(e03.x) == it && (fl & need) == need && size <= cur && cur - size <= 32 && (role == 0 || plan_same_state(c, h.na, e + FO_D, c.rs))) {
                int gs = -1;
                const int idx = wg_rfl(role ? e47.y : e03.w);
                if (size < cur && wg_refine(h, c, t, c.rs, idx, size, cur) != idx) gs = -2;        // another node is nearer now: the general path
                else if (fl & (role ? FF_CTRAP : FF_DTRAP)) gs = GROW_TRAPPED;
                else if (fl & (role ? FF_CS : FF_DS)) {
                    int v = -1;
                    if (role == 0) { if (fl & FF_D) v = (fl & FF_DOK) ? 1 : 0; }
                    else if (fl & FF_CREACH) v = 1;        // (the state the first call has just added)
                    else if (fl & FF_C) v = (fl & FF_COK) ? 1 : 0;
                    const int nd = wg_rfl(role ? e47.w : e47.z);
                    const int iv = nd < 2 ? 1 : ((nd == 2 && (fl & (role ? FF_CI : FF_DI))) ? ((fl & (role ? FF_CIOK : FF_DIOK)) ? 1 : 0) : -1);
                    if (cur >= c.cap) gs = GROW_TRAPPED;
                    else if (v == 0) { c.n_checks++; gs = GROW_TRAPPED; }
                    else if (v == 1 && iv >= 0) {
                        c.n_checks += (is_start ? 1 : 2) + (nd < 2 ? 0 : 1);      // the new state [, the tree node behind it], the interior state
                        if (!iv) gs = GROW_TRAPPED;
                        else {
                            const double *ds = e + (role ? FO_C : FO_D);
                            const bool rch = (fl & (role ? FF_CREACH : FF_DREACH)) != 0;
                            if (!rch && lane < h.na) c.xs[lane] = ds[lane];
                            plan_append(h, c, t, idx, ds);
                            gs = rch ? GROW_REACHED : GROW_ADVANCED;
                        }
                    }
                }
                if (gs >= 0) {
#ifdef MOPA_PLAN_STATS
                    c.st_fast++;
#endif
                    PLAN_T(39);
                    return gs;
                }
            }
            PLAN_T(39);
        }
    }
    {
        PLAN_T0();
        if constexpr (B::kWg) nm = wg_nn_lookup(h, c, t, it, role, c.rs);
        else nm = nn_known(h, c, t, c.rs);
        if (nm < 0) {
            int dummy;
            if (!nn_fast<B, false>(h, c, t, c.rs, c.rs, nm, dummy)) {
#ifdef MOPA_PLAN_STATS
                if (threadIdx.x == 0) atomicAdd(&g_plan_t[47], 1ull);
#endif
                nm = plan_nearest(h, c, t, c.rs);
            }
        }
        PLAN_T(6);
    }
    PLAN_T0();
    if (c.lane < h.na) c.ns[c.lane] = tree_q(c, t)[(size_t)nm * h.na + c.lane];
    wave_sync();
    bool reach = true;
    const double *dstate = c.rs;
    double d = wave_dist_l1(h, c.v, c.lane, c.so2, c.ns, c.rs);
    if (d > h.range) {
        double tt = h.range / d;
        if (c.lane < h.na) c.xs[c.lane] = k3_interp_dim(c.so2, c.lane, c.ns[c.lane], c.rs[c.lane], tt);
        wave_sync();
        bool differs = false;
        for (int a = c.lane; a < h.na; a += 64) differs |= fabs(c.xs[a] - c.ns[a]) > 2.0 * kCcdEps;   // StateSpace::equalStates
        if (!__any(differs)) return GROW_TRAPPED;
        dstate = c.xs;
        reach = false;
    }
    PLAN_T(48);
    if (tree_n(c, t) >= c.cap) return GROW_TRAPPED;   // node budget: a full tree takes no new state, so nothing is validated for it
    int lead_v;
    {   // no pass will run if the new state is already known to be invalid: nothing to ride along with
        PLAN_T0();
        const int lead_k = memo_find(h, c, dstate);
        lead_v = lead_k >= 0 ? (int)((c.memo_ok >> lead_k) & 1u) : -1;
        if constexpr (B::kWg) {
            if (lead_v < 0) lead_v = wg_memo_lookup(h, c, it, role, dstate);
        }
        if (lead_v != 0) plan_speculate<B>(h, c, spec_mode, t, dstate, reach, it);
        else c.spec_n = 0;
        PLAN_T(7);
    }
    // (one call site: growing the start tree checks ns -> dstate, the goal tree dstate -> ns after dstate itself)
#ifdef MOPA_PLAN_STATS
    const unsigned long long tcm0_ = wall_clock64();
#endif
    const bool ok = plan_check_motion<B>(h, c, is_start ? c.ns : dstate, is_start ? dstate : c.ns, is_start ? nullptr : dstate, lead_v);
#ifdef MOPA_PLAN_STATS
    if (threadIdx.x == 0) atomicAdd(&g_plan_t[49], wall_clock64() - tcm0_);
    const unsigned long long tap0_ = wall_clock64();
#endif
    if (!ok) return GROW_TRAPPED;
    plan_append(h, c, t, nm, dstate);
#ifdef MOPA_PLAN_STATS
    if (threadIdx.x == 0) atomicAdd(&g_plan_t[50], wall_clock64() - tap0_);
#endif
    return reach ? GROW_REACHED : GROW_ADVANCED;
}

// A solution's rows into the caller's path (k_rrt_connect; k_race_pick for the race's winner): the start tree's chain from node sm backwards
// into rows n1-1 .. 0, the goal tree's from node gm forwards into rows n1 ...  Per row the env row first, then -- behind a fence -- the
// active entries: their columns may alias columns of the env row.  GUARDED (k_race_pick, which walks what another kernel recorded): a node
// index outside the tree, or a row outside the solution's `total` rows or the path's max_path, ends the walk; the unguarded form takes no guards.
template <bool GUARDED>
MOPA_D void plan_write_rows(int lane, int na, int nq, const int *act_adr, const double *row, double *pe, const double *tq0, const int32_t *tp0,
                            const double *tq1, const int32_t *tp1, int sm, int gm, int n1, int max_nodes = 0, int total = 0, int max_path = 0 /* the guards */) {
    auto put = [&](int k, const double *node) {
        double *rowo = pe + (size_t)k * nq;
        for (int i = lane; i < nq; i += 64) rowo[i] = row[i];
        __threadfence_block();
        wave_sync();
        if (lane < na) rowo[act_adr[lane]] = node[lane];
    };
    int k = n1 - 1;
    for (int m = sm; m != -1 && (!GUARDED || (m >= 0 && m < max_nodes && k >= 0)); m = tp0[m], k--) put(k, tq0 + (size_t)m * na);
    k = n1;
    for (int m = gm; m != -1 && (!GUARDED || (m >= 0 && m < max_nodes && k < total && k < max_path)); m = tp1[m], k++) put(k, tq1 + (size_t)m * na);
}

// Two waves per SIMD (256 registers): the planner is latency-bound per wave -- one env, one dependency chain -- so a second
// wave on the SIMD is nearly free throughput (a stream of batches through the ladder: 360 -> 438 k plans/s).  What made that
// possible: wave-uniform indices through readfirstlane (22 pointers had lived in vector registers: 310 -> 264 registers) and
// the single inlined validity call site (no ABI register saves around every pass).  A lone launch is capped to one workgroup
// per CU by default (mopa_plan_batch): two budget-exhausting queries that share a SIMD both finish late (47 vs 54 ms).
template <class B>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(B::kWaves, B::kWaves))) void k_rrt_connect(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                        const double *__restrict__ start, const double *__restrict__ goal, long long E,
                                                        MopaPlanParams prm, PlanWs ws, double *__restrict__ path,
                                                        int32_t *__restrict__ path_len, int32_t *__restrict__ status,
                                                        long long *__restrict__ n_checks, int plan_lds_off, unsigned long long *__restrict__ env_ctr, int nn_cap,
                                                        std::conditional_t<B::kRace, RaceArgs, K3NoArgs> ra) {
    // The planner's own name for the dynamic LDS (every such array starts at the same address).  Sharing the other kernels' `smem`
    // ties the compiler's treatment of their address arithmetic to this kernel's: with it K3W2 had 36 VGPR spills instead of 33 and
    // k_contact_rows one more SGPR spill (profiles/r20).
    extern __shared__ __attribute__((aligned(16))) unsigned char k3_smem[];
    unsigned char *const smem = k3_smem;
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int na = h.na;
    const int vec_bytes = B::kWg ? plan_vec_bytes_wg(na) : plan_vec_bytes(na);
    const int wave_plan_bytes = vec_bytes + ms_bytes_per_wave(h.nmg, na, h.n_pq, ms_sc_doubles(h.nmj, h.nmb), h.npair);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + plan_lds_off + kWavesPerBlock * wave_plan_bytes);
    {
        const int *src = reinterpret_cast<const int *>(&h);
        int *dst = reinterpret_cast<int *>(lh);
        for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    // Persistent waves: a wave takes the next env from a global counter when it has finished one.  With one env per wave
    // of a fixed grid, a workgroup holding one query that runs out its budget kept its other three waves' slots (and
    // its LDS) idle for the whole batch while later workgroups waited for a free CU.
    // The first query of a wave is fixed by its place -- wave w of workgroup b takes query b + w x (workgroups) --, so that a launch of few
    // queries (a retry launch: budget-exhausting queries only) puts ONE on every workgroup before any gets a second: four such queries
    // on one CU run 12 % slower each (40.6 vs 35.6 ms) than one alone.
    // (one-wave-per-SIMD builds only: the 256-register build spills more with this one flag alive -- ladder 478 -> 425 k plans/s;
    //  there it is the constant `false` and the first branch below is gone)
    bool first_query = B::kWaves == 1;
    // what lies behind the header's copy: the FP32 mirrors of the workgroup's four queries, or -- one query per workgroup -- the pass
    // mailbox, the two query-index words and the workgroup's one mirror
    unsigned char *wg_sh = smem + plan_lds_off + kWavesPerBlock * wave_plan_bytes + (((int)sizeof(SceneHdr) + 15) & ~15);
    // one query per workgroup: the first by the workgroup's place, later ones from the counter, fetched by wave 0 and handed to the
    // others through LDS (two words in turn: a wave cannot be two fetches ahead of another, each fetch has a barrier)
    long long *sh_e = reinterpret_cast<long long *>(wg_sh + 2 * kWavesPerBlock * kMbStride * 8);
    int fetch_par = 0;
    for (;;) {
    long long e = 0;
    if (first_query) {
        first_query = false;
        e = (long long)blockIdx.x + (B::kWg ? 0ll : (long long)gridDim.x * wave);
    } else if constexpr (B::kWg) {
        if (wave == 0 && lane == 0) sh_e[fetch_par] = (long long)(atomicAdd(env_ctr, 1ull) + (unsigned long long)gridDim.x);
        __syncthreads();
        const long long t = sh_e[fetch_par];
        e = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) |
                        (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)t));
        fetch_par ^= 1;
    } else {
        unsigned long long t = 0;
        if (lane == 0) t = atomicAdd(env_ctr, 1ull) + ((B::kWaves == 1) ? (unsigned long long)gridDim.x * kWavesPerBlock : 0ull);
        // scalar registers for the env index (and so for the tree / row pointers derived from it)
        e = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) |
                        (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)t));
    }
    if (e >= E) { tile_ctr_release(env_ctr, lane); return; }       // (the last wave out leaves the counter at zero for the next launch)
    // the race: e is the launch SLOT (trees, record); start, goal, env row, stream id and seed are query eq's -- no K-fold copy of
    // the inputs.  Every other build: the slot is the query.
    int member = 0;
    long long eq = e;
    if constexpr (B::kRace) {
        member = (int)(e / ra.Eq);
        eq = e - (long long)member * ra.Eq;
    }
#ifdef MOPA_PLAN_STATS
    const unsigned long long tq0_ = wall_clock64();
#endif
    // (continuation of a launch's whole query list: the queries that launch already settled are skipped, outputs untouched)
    if (prm.resume_state && prm.resume_state[4 * e] == -2) continue;
    // planner vectors live behind the validity slabs of all waves
    unsigned char *pbase = smem + plan_lds_off + wave * wave_plan_bytes;
    K3Ctx<B> c;
    c.v = v; c.lane = lane; c.lh = lh;
    c.row = start + eq * h.nq;
    c.rs = reinterpret_cast<double *>(pbase); c.xs = c.rs + na; c.ns = c.xs + na; c.ts = c.ns + na; c.r2 = c.ts + na;
    c.memo_q = c.r2 + na; c.spec_q = c.memo_q + kMemo * na; c.nn_q = c.spec_q + kSpec * na;
    c.queue = reinterpret_cast<short *>(c.nn_q + 2 * na);
    c.memo_ok = 0; c.memo_cnt = 0; c.spec_n = 0;
    c.nn_tree0 = c.nn_tree1 = -1; c.nn_size0 = c.nn_size1 = 0; c.nn_idx0 = c.nn_idx1 = 0;
    if constexpr (B::kWg) {
        // ONE mirror for the workgroup (nn_cap = all of it): every wave appends the same values in the same order and only sweeps what it
        // has itself appended
        c.nn_f = reinterpret_cast<float *>(wg_sh + plan_wg_shared_bytes());
        c.wave = wave;
        c.ftab = reinterpret_cast<double *>(pbase + plan_vec_bytes(na));
        c.f0 = c.ftab + kFSlots * kFStride; c.f1 = c.f0 + 8; c.f2 = c.f1 + 8;
        c.mbox = reinterpret_cast<double *>(wg_sh);
        c.pass_par = 0; c.sp_pending = false; c.sp_it = 0; c.cur_it = 0; c.cur_role = 0;
        if (lane < kFSlots) {
            int *ei = reinterpret_cast<int *>(c.ftab + lane * kFStride);
            ei[0] = -1; ei[1] = 0;
        }
    } else c.nn_f = reinterpret_cast<float *>(wg_sh) + (size_t)wave * nn_cap * na;
    c.nn_cap = nn_cap; c.nn_cnt0 = c.nn_cnt1 = 0; c.nn_eps2 = (float)(2.0 * h.nn_eps);
    c.ms.grec = reinterpret_cast<double *>(pbase + vec_bytes);
    c.ms.qbuf = c.ms.grec + kMS * h.nmg * kGeomStride;
    c.ms.qs = c.ms.qbuf + kMS * (na + h.n_pq + ms_sc_doubles(h.nmj, h.nmb));
    c.ms.wl = reinterpret_cast<unsigned *>(c.ms.qs + kMS * na);
    ms_fill_passive(h, v.ints, c.ms.qbuf, lane, c.row);
    c.cap = prm.max_nodes;
    // trees: the launch's scratch, or -- when the caller wants to continue unsolved queries later (keep_state) -- its buffers
    c.tq0 = (prm.tree_q_dev ? prm.tree_q_dev : ws.tree_q) + ((size_t)e * 2) * (size_t)prm.max_nodes * na;
    c.tq1 = c.tq0 + (size_t)prm.max_nodes * na;
    c.tp0 = (prm.tree_p_dev ? prm.tree_p_dev : ws.tree_parent) + ((size_t)e * 2) * (size_t)prm.max_nodes;
    c.tp1 = c.tp0 + prm.max_nodes;
    c.n0 = c.n1 = 1;
    c.n_checks = 0; c.xmotion = -1; c.overflow = false;
    // Continuation (resume_*): query e goes on from the trees, iteration count and consumed-check count an earlier launch with
    // a smaller budget left behind (state row: iterations done | -1 = that outcome is final, n0, n1, consumed checks).  A
    // query's outcome is a function of its endpoints and sample stream only and a budget merely ends the loop, so the
    // continued run IS the full run; what is not carried over (verdict memo, nearest-neighbour cache) only saves work.
    int it0 = 0;
    bool resumed = false, final_no_exact = false;
    if (prm.resume_state) {
        const int64_t *rs = prm.resume_state + 4 * e;
        resumed = true;
        const long long itd = rs[0];
        c.n0 = (int)rs[1]; c.n1 = (int)rs[2]; c.n_checks = rs[3];
        if (itd < 0) final_no_exact = true;
        else {
            it0 = (int)itd;
            const double *sq = prm.resume_tree_q + ((size_t)e * 2) * (size_t)prm.max_nodes * na;
            const int32_t *sp = prm.resume_tree_p + ((size_t)e * 2) * (size_t)prm.max_nodes;
            for (int i = lane; i < c.n0 * na; i += 64) c.tq0[i] = sq[i];
            for (int i = lane; i < c.n1 * na; i += 64) c.tq1[i] = sq[(size_t)prm.max_nodes * na + i];
            for (int i = lane; i < c.n0; i += 64) c.tp0[i] = sp[i];
            for (int i = lane; i < c.n1; i += 64) c.tp1[i] = sp[prm.max_nodes + i];
            __threadfence_block();
            wave_sync();
        }
    }
    const uint64_t stream_id = prm.env_ids_dev ? prm.env_ids_dev[eq] : prm.env_id_base + (uint64_t)eq;
    uint64_t seed_q = prm.seeds_dev ? prm.seeds_dev[eq] : prm.seed;
    if constexpr (B::kRace) seed_q += (uint64_t)member * kRaceSeedStep;
    c.seed = seed_q; c.stream = stream_id; c.rng_k = rng_key(seed_q, stream_id); c.max_iters = prm.max_iters;
    c.so2 = __ballot(lane < na && v.ints[h.o_act_so2 + (lane < na ? lane : 0)] != 0);
    const int *I = v.ints;
    const double *D = v.dbl;
    const double *grow_ = goal + eq * h.nq;
    // roots
    if (!resumed) {
        if (lane < na) {
            int adr = I[h.o_act_adr + lane];
            tree_q(c, 0)[lane] = c.row[adr];
            tree_q(c, 1)[lane] = grow_[adr];
        }
        if (lane == 0) { tree_p(c, 0)[0] = -1; tree_p(c, 1)[0] = -1; }
        __threadfence_block();
        wave_sync();
    }
    // mirror what the trees hold now: the roots, or the nodes a continued query starts from (tree 1 first gets at most half)
    for (int t = 1; t >= 0; t--) {
        const int n = tree_n(c, t);
        int room = c.nn_cap - c.nn_cnt0 - c.nn_cnt1;
        if (t == 1 && room > c.nn_cap / 2) room = c.nn_cap / 2;
        const int take = n < room ? n : room;
        const double *tq = tree_q(c, t);
        for (int idx = lane; idx < take * na; idx += 64) {
            const int i = idx / na, j = idx - i * na;
            c.nn_f[j * c.nn_cap + (t ? c.nn_cap - 1 - i : i)] = (float)tq[idx];
        }
        if (t) c.nn_cnt1 = take; else c.nn_cnt0 = take;
    }
    wave_sync();
    int st = MOPA_PLAN_OK;
    int plen = 0;
    bool keep_final = false;       // keep_state: this NO_EXACT does not depend on the budget (invalid start, path too long)
    // goal must be valid (KinematicPlanner.cpp:181-184)
    if (!resumed) c.n_checks++;
    auto root_valid = [&](const double *qa) -> bool {      // validity of a tree root through the multi-state routine (one state)
        if (lane < na) c.ms.qs[lane] = qa[lane];
        wave_sync();
        return (plan_states_valid_ms_k3<B>(c.lh, c.v.dbl, c.v.ints, c.ms.grec, c.ms.qbuf, c.ms.wl, c.ms.qs, lane, 1, c.row) & 1u) != 0u;
    };
    if (!resumed && !root_valid(tree_q(c, 1))) st = MOPA_PLAN_INVALID_GOAL;
    int it_end = 0;
    int race_sm = -1, race_gm = -1;      // the race: the solution's two motions, for k_race_pick
    bool race_cut = false;
    if (st == MOPA_PLAN_OK) {
        int max_iters = prm.max_iters;
        if (!resumed) {
            c.n_checks++;
            if (!root_valid(tree_q(c, 0))) { max_iters = 0; keep_final = true; }   // OMPL: "Invalid start" -> no exact solution
        } else if (final_no_exact) { max_iters = 0; keep_final = true; }
        bool start_tree = (it0 & 1) == 0, solved = false;      // the trees alternate from iteration 0 on
        int start_motion = -1, goal_motion = -1;
        int it = it0;
        for (; it < max_iters && !solved; it++) {
            if constexpr (B::kRace) {
                // the race word holds the smallest key = consumed checks * K + member of the members that have solved.  Consumed checks only
                // grow, so a member whose key so far is already larger can no longer win: it stops.  (An atomic load by one lane, never
                // a plain or scalar one; a stale value only delays the cut.)
                if (!ra.no_abort) {
                    unsigned long long w = 0ull;
                    if (lane == 0) w = __hip_atomic_load(ra.word + eq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w);
                    if ((unsigned long long)c.n_checks * (unsigned long long)ra.K + (unsigned long long)member > w) { race_cut = true; break; }
                }
            }
            int tree = start_tree ? 0 : 1;
            bool tgi_start = start_tree;
            start_tree = !start_tree;
            int other = start_tree ? 0 : 1;
            if (lane < na) {
                double lo = D[h.o_act_lo + lane], hi = D[h.o_act_hi + lane];
                c.rs[lane] = fma(hi - lo, rng_uniform_k(c.rng_k, (uint64_t)it * na + lane), lo);
            }
            wave_sync();
            int role = 0;
            if constexpr (B::kWg) c.cur_it = it;
            // growTree(tree, sample), then -- unless trapped -- growTree(other, new state) while it advances: the same
            // sequence of calls as OMPL's loop, issued from ONE site (a two-phase trip) so that everything below it,
            // the validity pass included, is inlined exactly once
            bool extend = true;
            int added = -1;
            for (;;) {
#ifdef MOPA_PLAN_STATS
                const unsigned long long tg0_ = wall_clock64();
#endif
                const int gs = plan_grow<B>(h, c, extend ? tree : other, extend ? tgi_start : start_tree, extend ? SPEC_FIRST : SPEC_CONNECT, it, role);
#ifdef MOPA_PLAN_STATS
                if (threadIdx.x == 0) { atomicAdd(&g_plan_t[45], wall_clock64() - tg0_); atomicAdd(&g_plan_t[46], 1ull); }
#endif
                if (extend) {
                    if (gs == GROW_TRAPPED) break;
                    added = c.xmotion;
                    if (gs != GROW_REACHED) {
                        if (lane < na) c.rs[lane] = c.xs[lane];
                        wave_sync();
                    }
                    extend = false;
                    role = 1;
                    continue;
                }
                role = 2;
                if (gs == GROW_ADVANCED) continue;
                if (gs == GROW_REACHED) {
                                    start_motion = start_tree ? c.xmotion : added;
                    goal_motion = start_tree ? added : c.xmotion;
                    if (tree_p(c, 0)[start_motion] != -1) start_motion = tree_p(c, 0)[start_motion];
                    else goal_motion = tree_p(c, 1)[goal_motion];
                    solved = true;
                }
                break;
            }
        }
            if (solved) {
            int n1 = 0, n2 = 0;
            for (int m = start_motion; m != -1; m = tree_p(c, 0)[m]) n1++;
            for (int m = goal_motion; m != -1; m = tree_p(c, 1)[m]) n2++;
            if (n1 + n2 > prm.max_path) { st = MOPA_PLAN_NO_EXACT; keep_final = true; }
            else {
                if constexpr (B::kRace) {
                    // no path rows: the trees stay in the launch's scratch and k_race_pick traces the winner's
                    race_sm = start_motion; race_gm = goal_motion;
                    if (lane == 0) (void)__hip_atomic_fetch_min(ra.word + eq, (unsigned long long)c.n_checks * (unsigned long long)ra.K + (unsigned long long)member,
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (!B::kWg || wave == 0)
                    plan_write_rows<false>(lane, na, h.nq, I + h.o_act_adr, c.row, path + (size_t)e * prm.max_path * h.nq, c.tq0, c.tp0, c.tq1, c.tp1,
                                           start_motion, goal_motion, n1);
                plen = n1 + n2;
            }
        } else st = MOPA_PLAN_NO_EXACT;
        if constexpr (B::kRace) {
            if (race_cut) st = kRaceCut;
        }
        it_end = it;
    }
    if (!B::kWg || wave == 0) {
    if (lane == 0 && prm.state_dev) {
        int64_t *so = prm.state_dev + 4 * e;
        so[0] = (st != MOPA_PLAN_NO_EXACT) ? -2ll : (keep_final ? -1ll : (long long)it_end);     // -2: settled (solved / invalid goal)
        so[1] = c.n0; so[2] = c.n1; so[3] = c.n_checks;
    }
#ifdef MOPA_PLAN_STATS
    if (threadIdx.x == 0) atomicAdd(&g_plan_t[44], wall_clock64() - tq0_);
#endif
    if constexpr (B::kRace) {
        if (lane == 0) {       // the member's record (slot order) instead of the query's outputs: k_race_pick writes those
            long long *r = ra.rec + (size_t)kRaceRec * (size_t)e;
            r[0] = st; r[1] = c.n_checks; r[2] = it_end; r[3] = race_sm; r[4] = race_gm; r[5] = plen;
        }
    } else if (lane == 0) {
        status[e] = st;
        path_len[e] = plen;
        if (n_checks) n_checks[e] = c.n_checks;
#ifdef MOPA_PLAN_STATS   // debug builds only: passes / evaluated states / tree sizes packed above the count
        if (n_checks) n_checks[e] = (c.n_checks & 0xffff) | (c.st_pass << 16) | (c.st_states << 30) | ((long long)tree_n(c, 0) << 44) | ((long long)tree_n(c, 1) << 54);
#endif
    }
    }
#ifdef MOPA_PLAN_STATS
    if constexpr (B::kWg) {
        if (lane == 0) {    // table hits and pass causes (wave 0's counts = every wave's), states posed per wave
            if (wave == 0) {
                atomicAdd(&g_plan_t[51], (unsigned long long)c.st_fnn); atomicAdd(&g_plan_t[52], (unsigned long long)c.st_fmemo);
                atomicAdd(&g_plan_t[57], (unsigned long long)c.st_fast);
                atomicAdd(&g_plan_t[58], (unsigned long long)c.st_c0); atomicAdd(&g_plan_t[59], (unsigned long long)c.st_c1);
                atomicAdd(&g_plan_t[60], (unsigned long long)c.st_c2); atomicAdd(&g_plan_t[61], (unsigned long long)c.st_c3);
            }
            atomicAdd(&g_plan_t[53 + wave], (unsigned long long)c.st_fstates);
        }
    }
#endif
    wave_sync();
    }
}

