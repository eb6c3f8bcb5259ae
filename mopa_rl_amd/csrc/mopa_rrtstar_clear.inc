// mopa_rrtstar_clear.inc -- K3b under the maximize-min-clearance objective, band-limited: k_rrt_star_clear, one wave per query.
// (included by mopa_hip.hip behind mopa_rrtstar.inc, whose StarArgs, slab / LDS layout, star_ld / star_ldi and host staging it shares)
//
// RRT* whose cost is the quantity the clearance report measures (DESIGN.md section 4, "K3b under the clearance objective").  The
// sequential form of tests/star_clearance_ref.py is the definition; paths, clearance, length and counters are required identical to
// it.  A chain's key is (C, L): C = min(the band-saturated clearance of the root state, the motion clearances of its edges), L = its
// L1 length; better((C1, L1), (C2, L2)) = C1 > C2 or (C1 == C2 and L1 < L2).  Draws, nearest, steering, the full-tree rule, k(n),
// the goal rule and the goal-bias rule are k_rrt_star's, expression for expression, so the node set of a query is the one
// path-length RRT* grows.  What differs:
//   * a motion is EVALUATED, not checked: mc(a -> b) = the smallest band-saturated state clearance over s_1 .. s_c, c = max(nd, 1),
//     s_k = interp_dim(a, qa[a], qb[a], (double)k / (double)c) for k < c and s_c = qb's bits -- mopa_motion_clearance.inc's
//     expressions, k ascending, one state per pass through wave_state_clearance (k_clearance_states' sweep).  Valid iff mc > thr.  An
//     evaluation stops as soon as its running minimum is <= thr: the value is then unused.
//   * the parent walk is an exact branch and bound over ub[s] = (C[nbh[s]], L[nbh[s]] + ninc[s]), best first, ties to lower s: it
//     stops at the first bound that is not better than the best parent found, starting from the nearest node's own evaluation.
//   * a rewire is pre-tested on (C[n], L[n] + ninc[s]) without an evaluation, evaluated in the chain's direction x -> Q[i] (nothing
//     of the parent walk is reused), and refreshes C and L of every descendant from `edge` and `inc` by k_rrt_star's stamped sweeps.
// The tree slab holds per node: na doubles, C, L, inc, edge, the distance to the new state, parent, stamp, goal flag (8 na + 52
// bytes).  Decisions come from wave-uniform values, reads at wave-uniform indices are volatile, stores are vector stores, no
// atomics -- mopa_rrtstar.inc's rules.

struct StarClearArgs {
    StarArgs s;                         // s.cost: length [E] nullable; s.info: [E, 11] nullable
    double band;
    double *clearance;                  // [E]
    const int32_t *pair_model;          // [npair]: wave_state_clearance's pair names (its second output is not used here)
};

constexpr int kStarClearInfoCols = 11;
static int star_clear_node_bytes(int na) { return 8 * na + 40 + 12; }

// wave_state_clearance behind a call, as plan_state_valid_impl puts the validity sweep behind one: the planner body keeps its registers.
// `qa` (the wave's spare [na] doubles) and every pointer but `row` / `pair_model` are LDS.  Returns the saturated clearance on every lane.
__device__ __noinline__ double plan_state_clearance_impl(const SceneHdr *hp, const double *dbl, const int *ints, double *grec, double *qbuf,
                                                         unsigned short *wl, int lane, const double *qa, const double *row,
                                                         const int32_t *pair_model, double band) {
    MOPA_ASSUME_LDS(hp); MOPA_ASSUME_LDS(dbl); MOPA_ASSUME_LDS(ints); MOPA_ASSUME_LDS(grec); MOPA_ASSUME_LDS(qbuf); MOPA_ASSUME_LDS(wl);
    const SceneHdr &h = *hp;
    LdsView v;
    v.dbl = dbl; v.ints = ints; v.grec = grec; v.qbuf = qbuf; v.sc = qbuf + h.na + h.n_pq + h.na; v.wl = wl;
    double d;
    int p;
    // one copy of each instantiation; the branch is wave-uniform (scenes with a collidable mesh: Lift's can)
    if (h.has_mesh) wave_state_clearance<true>(h, v, lane, qa, row, pair_model, band, d, p);
    else wave_state_clearance<false>(h, v, lane, qa, row, pair_model, band, d, p);
    wave_sync();   // worklist / geom slab are about to be reused
    return d;
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_rrt_star_clear(SceneHdr h, const double *__restrict__ g_dbl,
                                                                                                     const int32_t *__restrict__ g_int, StarClearArgs ca) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const StarArgs &a = ca.s;
    LdsView v = make_view(h, smem);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + a.hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int na = h.na, nq = h.nq, max_nodes = a.max_nodes;
    const double band = ca.band, thr = h.thr;
    double *ends = reinterpret_cast<double *>(smem + a.list_lds_off + wave * a.list_bytes);      // [2][na]
    double *rs = ends + 2 * na, *xs = rs + na, *qg = xs + na;                                     // [na] each
    double *tst = v.qbuf + na + h.n_pq;                                                         // spare [na] doubles behind the joint-value buffer
    const int *adr = v.ints + h.o_act_adr;
    unsigned char *tb = a.tree + (size_t)((long long)blockIdx.x * kWavesPerBlock + wave) * (size_t)a.tree_bytes;
    double *Q = reinterpret_cast<double *>(tb);                     // [max_nodes][na]
    double *Cn = Q + (size_t)max_nodes * na;                        // [max_nodes]: the clearance of the node's chain
    double *Ln = Cn + max_nodes;                                    // [max_nodes]: its L1 length
    double *inc = Ln + max_nodes;                                   // [max_nodes]: distance to the parent
    double *edge = inc + max_nodes;                                 // [max_nodes]: mc(parent -> node)
    double *dtmp = edge + max_nodes;                                // [max_nodes]: distance to the new state of this iteration
    int *parent = reinterpret_cast<int *>(dtmp + max_nodes);        // [max_nodes]
    int *stamp = parent + max_nodes;                                // [max_nodes]: the rewire that last refreshed the node's key
    int *flags = stamp + max_nodes;                                 // [max_nodes]: 1 = goal node
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long e = (long long)blockIdx.x * kWavesPerBlock + wave; e < a.E; e += stride) {
        const double *row = a.start + (size_t)e * nq, *grow_ = a.goal + (size_t)e * nq;
        double *pe = a.path + (size_t)e * a.max_path * nq;
        const unsigned long long key = rng_key(a.seeds ? a.seeds[e] : a.seed, a.env_ids ? a.env_ids[e] : a.env_id_base + (unsigned long long)e);
        long long n_evals = 0, n_par = 0, n_rew = 0, n_raise = 0, n_rewire = 0, n_desc = 0, n_full = 0, n_goal = 0, first_goal = -1, its = 0;
        int n = 0, st = MOPA_PLAN_OK, plen = 0;
        double best_c = -__builtin_inf(), best_l = __builtin_inf();

        auto uni = [&](bool b) -> bool { return __builtin_amdgcn_readfirstlane((int)b) != 0; };
        auto better = [](double c1, double l1, double c2, double l2) -> bool { return c1 > c2 || (c1 == c2 && l1 < l2); };
        auto state_ok = [&](const double *q) -> bool {
            for (int i = lane; i < na; i += 64) tst[i] = q[i];
            wave_sync();
            const bool ok = uni(plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row));
            wave_sync();
            return ok;
        };
        // sc(tst), wave-uniform
        auto state_clear = [&]() -> double {
            return wave_bcast_f64(plan_state_clearance_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row, ca.pair_model, band), 0);
        };
        // mc from ends[0..na) to ends[na..2 na); at or below thr the value is only known to be that
        auto eval_ends = [&]() -> double {
            n_evals++;
            wave_sync();
            const int nd = __builtin_amdgcn_readfirstlane(valid_segment_count(h, v, ends, ends + na));
            const int c = nd > 1 ? nd : 1;
            double m = __builtin_inf();
            for (int k = 1; k <= c; k++) {
                const double t = (double)k / (double)c;
                for (int i = lane; i < na; i += 64) tst[i] = (k == c) ? ends[na + i] : interp_dim(h, v, i, ends[i], ends[na + i], t);
                wave_sync();
                const double d = state_clear();
                if (d < m) m = d;
                if (!(m > thr)) break;
            }
            wave_sync();
            return m;
        };
        // the smallest (distance, index) pair of the wave, on every lane
        auto reduce_min = [&](double &bd, int &bi) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double od = __shfl_xor(bd, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            bi = __builtin_amdgcn_readfirstlane(bi);
            bd = wave_bcast_f64(bd, 0);
        };
        // dist(Q[i], p) with p in LDS: the adds in ascending coordinate order, from 0.0
        auto node_dist = [&](int i, const double *p) -> double {
            double d = 0.0;
            for (int c = 0; c < na; c++) d += dist_dim(h, v, c, Q[(size_t)i * na + c], p[c]);
            return d;
        };
        auto node_dist_uniform = [&](int i, const double *p) -> double {
            double d = 0.0;
            for (int c = 0; c < na; c++) d += dist_dim(h, v, c, star_ld(Q + (size_t)i * na + c), p[c]);
            return d;
        };

        for (int i = lane; i < na; i += 64) { qg[i] = grow_[adr[i]]; rs[i] = row[adr[i]]; }
        wave_sync();
        if (!state_ok(qg)) st = MOPA_PLAN_INVALID_GOAL;
        else if (!state_ok(rs)) st = MOPA_PLAN_NO_EXACT;
        if (st == MOPA_PLAN_OK) {
            // the root: vertex 0 is counted, as path_clearance counts it
            for (int i = lane; i < na; i += 64) { Q[i] = rs[i]; tst[i] = rs[i]; }
            wave_sync();
            const double c_root = state_clear();
            if (lane == 0) { parent[0] = -1; inc[0] = 0.0; edge[0] = __builtin_inf(); Cn[0] = c_root; Ln[0] = 0.0; stamp[0] = 0; flags[0] = 0; }
            wave_sync();
            n = 1;
            int cur_stamp = 0;
            for (int it = 0; it < a.max_iters; it++) {
                // 1. draws
                const unsigned long long c0 = (unsigned long long)it * (unsigned long long)(na + 1);
                const bool to_goal = n_goal == 0 && rng_uniform_k(key, c0) < a.goal_bias;
                for (int i = lane; i < na; i += 64) {
                    const double lo = v.dbl[h.o_act_lo + i], hi = v.dbl[h.o_act_hi + i];
                    rs[i] = to_goal ? qg[i] : fma(hi - lo, rng_uniform_k(key, c0 + 1ull + (unsigned long long)i), lo);
                }
                wave_sync();
                // 2. nearest node, the new state
                double d = __builtin_inf();
                int nm = 0x7fffffff;
                for (int i = lane; i < n; i += 64) {
                    const double di = node_dist(i, rs);
                    if (di < d) { d = di; nm = i; }
                }
                reduce_min(d, nm);
                {
                    const bool steer = d > h.range;
                    const double t = steer ? h.range / d : 1.0;
                    for (int i = lane; i < na; i += 64) xs[i] = steer ? interp_dim(h, v, i, Q[(size_t)nm * na + i], rs[i], t) : rs[i];
                }
                wave_sync();
                // 3. full tree
                if (n >= max_nodes) { n_full++; continue; }
                // 4. the first evaluation: the motion check and nm's edge value
                for (int i = lane; i < na; i += 64) { ends[i] = Q[(size_t)nm * na + i]; ends[na + i] = xs[i]; }
                const double m_nm = eval_ends();
                if (!(m_nm > thr)) continue;
                // 5. neighbours: lane s holds the s-th nearest node of the new state and its bound ub[s] = (my_c, my_l)
                for (int i = lane; i < n; i += 64) dtmp[i] = node_dist(i, xs);
                wave_sync();
                const int kt = star_ldi(a.ktab + (n - 1));
                const int kk = kt < n ? kt : n;
                double my_inc = 0.0, my_c = -__builtin_inf(), my_l = __builtin_inf();
                int my_idx = -1;
                {
                    double last_d = -1.0;
                    int last_i = -1;
                    for (int s = 0; s < kk; s++) {
                        double bd = __builtin_inf();
                        int bi = 0x7fffffff;
                        for (int i = lane; i < n; i += 64) {
                            const double di = dtmp[i];
                            if ((di > last_d || (di == last_d && i > last_i)) && di < bd) { bd = di; bi = i; }
                        }
                        reduce_min(bd, bi);
                        last_d = bd; last_i = bi;
                        if (lane == s) { my_inc = bd; my_idx = bi; }
                    }
                }
                if (lane < kk) { my_c = Cn[my_idx]; my_l = Ln[my_idx] + my_inc; }
                // 6. parent: branch and bound over the bounds, best first, ties to lower s
                int rank = 0;
                for (int t = 0; t < kk; t++) {
                    const double ct = wave_bcast_f64(my_c, t), lt = wave_bcast_f64(my_l, t);
                    if (ct > my_c || (ct == my_c && (lt < my_l || (lt == my_l && t < lane)))) rank++;
                }
                int par = nm;
                double pinc = node_dist_uniform(nm, xs), pedge = m_nm;
                double bc, bl = star_ld(Ln + nm) + pinc;
                {
                    const double cnm = star_ld(Cn + nm);
                    bc = m_nm < cnm ? m_nm : cnm;
                }
                for (int r = 0; r < kk; r++) {
                    const unsigned long long mk = __ballot(lane < kk && rank == r);
                    const int s = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)mk) - 1);
                    const int idx = __builtin_amdgcn_readlane(my_idx, s);
                    if (idx == nm) continue;
                    const double uc = wave_bcast_f64(my_c, s), ul = wave_bcast_f64(my_l, s);
                    if (!better(uc, ul, bc, bl)) break;          // every later bound is no better
                    n_par++;
                    for (int i = lane; i < na; i += 64) { ends[i] = Q[(size_t)idx * na + i]; ends[na + i] = xs[i]; }
                    const double m = eval_ends();
                    if (!(m > thr)) continue;
                    const double nc = m < uc ? m : uc;
                    if (better(nc, ul, bc, bl)) { bc = nc; bl = ul; par = idx; pedge = m; pinc = wave_bcast_f64(my_inc, s); }
                }
                // 7. append
                for (int i = lane; i < na; i += 64) Q[(size_t)n * na + i] = xs[i];
                if (lane == 0) { parent[n] = par; inc[n] = pinc; edge[n] = pedge; Cn[n] = bc; Ln[n] = bl; stamp[n] = 0; flags[n] = 0; }
                wave_sync();
                // 8. rewire
                for (int s = 0; s < kk; s++) {
                    const int i = __builtin_amdgcn_readlane(my_idx, s);
                    if (i == par) continue;
                    const double inc_s = wave_bcast_f64(my_inc, s);
                    const double nl = bl + inc_s;
                    const double ci = star_ld(Cn + i), li = star_ld(Ln + i);
                    if (!better(bc, nl, ci, li)) continue;       // the new chain's clearance cannot exceed C[n]
                    n_rew++;
                    for (int c = lane; c < na; c += 64) { ends[c] = xs[c]; ends[na + c] = Q[(size_t)i * na + c]; }
                    const double m = eval_ends();
                    if (!(m > thr)) continue;
                    const double nc = m < bc ? m : bc;
                    if (!better(nc, nl, ci, li)) continue;
                    if (nc > ci) n_raise++;
                    n_rewire++;
                    cur_stamp++;
                    if (lane == 0) { parent[i] = n; inc[i] = inc_s; edge[i] = m; Cn[i] = nc; Ln[i] = nl; stamp[i] = cur_stamp; }
                    wave_sync();
                    // every descendant of i, top down: a node is refreshed once its parent carries this rewire's stamp
                    bool changed = true;
                    while (changed) {
                        changed = false;
                        for (int base = 0; base <= n; base += 64) {
                            const int j = base + lane;
                            bool upd = false;
                            double nvc = 0.0, nvl = 0.0;
                            if (j <= n && stamp[j] != cur_stamp) {
                                const int p = parent[j];
                                if (p >= 0 && stamp[p] == cur_stamp) {
                                    upd = true;
                                    const double cp = Cn[p], ej = edge[j];
                                    nvc = ej < cp ? ej : cp;
                                    nvl = Ln[p] + inc[j];
                                }
                            }
                            wave_sync();
                            if (upd) { Cn[j] = nvc; Ln[j] = nvl; stamp[j] = cur_stamp; }
                            wave_sync();
                            const unsigned long long um = __ballot(upd);
                            n_desc += __popcll(um);
                            changed = changed || um != 0ull;
                        }
                    }
                }
                // 9. goal
                {
                    double dg = 0.0;
                    for (int c = 0; c < na; c++) dg += dist_dim(h, v, c, xs[c], qg[c]);
                    if (uni(dg <= a.goal_threshold)) {
                        if (lane == 0) flags[n] = 1;
                        if (n_goal == 0) first_goal = it;
                        n_goal++;
                    }
                }
                n++;
                wave_sync();
            }
            its = a.max_iters;
            // the goal node of the best key (the earliest among equals), its chain to the root
            st = MOPA_PLAN_NO_EXACT;
            if (n_goal > 0) {
                double gc = -__builtin_inf(), gl = __builtin_inf();
                int bg = 0x7fffffff;
                for (int j = lane; j < n; j += 64) {
                    const double cj = Cn[j], lj = Ln[j];
                    if (flags[j] != 0 && better(cj, lj, gc, gl)) { gc = cj; gl = lj; bg = j; }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double oc = __shfl_xor(gc, off, 64), ol = __shfl_xor(gl, off, 64);
                    const int oj = __shfl_xor(bg, off, 64);
                    if (better(oc, ol, gc, gl) || (oc == gc && ol == gl && oj < bg)) { gc = oc; gl = ol; bg = oj; }
                }
                bg = __builtin_amdgcn_readfirstlane(bg);
                gc = wave_bcast_f64(gc, 0);
                gl = wave_bcast_f64(gl, 0);
                int len = 0;
                for (int t = bg; t >= 0 && len <= n; t = star_ldi(parent + t)) len++;
                if (len <= a.max_path) {
                    int t = bg;
                    for (int pos = len - 1; pos >= 0; pos--) {
                        for (int i = lane; i < nq; i += 64) {
                            double val = row[i];
                            for (int c = 0; c < na; c++)
                                if (adr[c] == i) val = Q[(size_t)t * na + c];
                            pe[(size_t)pos * nq + i] = val;
                        }
                        t = star_ldi(parent + t);
                    }
                    st = MOPA_PLAN_OK;
                    plen = len;
                    best_c = gc;
                    best_l = gl;
                }
            }
        }
        if (lane == 0) {
            a.path_len[e] = plen;
            a.status[e] = st;
            ca.clearance[e] = best_c;
            if (a.cost) a.cost[e] = best_l;
            if (a.info) {
                long long *o = a.info + kStarClearInfoCols * e;
                o[0] = its; o[1] = n; o[2] = n_evals; o[3] = n_rewire; o[4] = n_goal; o[5] = first_goal; o[6] = n_desc; o[7] = n_full;
                o[8] = n_par; o[9] = n_rew; o[10] = n_raise;
            }
        }
        wave_sync();
    }
}

static const LdsKernels kStarClearLds({(const void *)k_rrt_star_clear});

extern "C" int mopa_plan_star_clearance_batch(MopaScene *S, const double *start, const double *goal, int64_t E, const MopaStarParams *params, double band,
                                              double *path, int32_t *path_len, int32_t *status, double *clearance, double *length, int64_t *info,
                                              void *stream) {
    if (!S || !params || (E > 0 && (!start || !goal || !path || !path_len || !status || !clearance))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const int node_bytes = star_clear_node_bytes(S->na);
    if (const int rc = star_rules(S, *params, E, "RRT* under the clearance objective (mopa_plan_star_clearance)", node_bytes)) return rc;
    if (const int rc = band_rule(band)) return rc;
    if (!(band > S->hdr.thr)) return fail(MOPA_ERR_INVALID_ARG, "band must be above the scene's contact_threshold: no motion is valid at or below it");
    if (S->pruned) return refuse_pruned("RRT* under the clearance objective needs");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    StarClearArgs ca;
    int64_t nblk;
    // two workgroups per CU are resident (two waves per SIMD, no VGPR spills: tools/kernel_resources.py)
    if (const int rc = star_stage(S, *params, start, goal, E, path, path_len, status, node_bytes, 2, (hipStream_t)stream, ca.s, nblk)) return rc;
    ca.s.cost = length;
    ca.s.info = reinterpret_cast<long long *>(info);
    ca.band = band;
    ca.clearance = clearance;
    ca.pair_model = (const int32_t *)S->d_pair_model;
    hipLaunchKernelGGL(k_rrt_star_clear, dim3((unsigned)nblk), dim3(kBlock), star_lds_bytes(S), (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, ca);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// the single-query host form (mopa_plan_star's shape): stream id = env_id_base, the default stream, synchronous
extern "C" int mopa_plan_star_clearance(MopaScene *S, const double *start_host, const double *goal_host, const MopaStarParams *params, double band,
                                        double *path_host, int32_t *path_len_out, int32_t *status_out, double *clearance_out, double *length_out,
                                        int64_t *info_out) {
    if (!S || !start_host || !goal_host || !params || !path_host || !path_len_out || !status_out || !clearance_out)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (params->max_path < 2) return fail(MOPA_ERR_INVALID_ARG, "max_path < 2");
    MOPA_REFUSE_GLUED(S, "RRT* under the clearance objective (mopa_plan_star_clearance)");
    MopaStarParams one = *params;
    one.env_ids_dev = nullptr;
    one.seeds_dev = nullptr;
    // further outputs: clearance | length | info[kStarClearInfoCols]
    return plan_single(S, start_host, goal_host, params->max_path, path_host, path_len_out, status_out, 8 * (2 + kStarClearInfoCols),
        [&](const double *s, const double *g, double *p, int32_t *len, int32_t *st, void *x) {
            return mopa_plan_star_clearance_batch(S, s, g, 1, &one, band, p, len, st, static_cast<double *>(x), static_cast<double *>(x) + 1,
                                                  static_cast<int64_t *>(x) + 2, nullptr);
        },
        [&](const void *x) {
            hipError_t e = hipMemcpy(clearance_out, x, 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess && length_out) e = hipMemcpy(length_out, static_cast<const double *>(x) + 1, 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess && info_out) e = hipMemcpy(info_out, static_cast<const int64_t *>(x) + 2, 8 * kStarClearInfoCols, hipMemcpyDeviceToHost);
            return e;
        });
}
