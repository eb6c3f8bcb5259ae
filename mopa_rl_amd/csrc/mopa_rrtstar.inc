// mopa_rrtstar.inc -- K3b: RRT* (the reference's planner_type "rrt"), one wave per query, persistent waves.
// (included by mopa_hip.hip behind mopa_k9.inc: the kernel has the shape of the K9 kernels)
//
// OMPL's geometric::RRTstar restated as the reference configures it -- k-nearest neighbourhoods, path-length objective, no cost
// threshold -- with an iteration budget in place of the wall clock (DESIGN.md "K3b RRT*").  The sequential form of
// tests/rrtstar_ref.py is the definition: path rows, cost and counters are required identical to it, hence every floating-point
// operation is the one named there (adds in ascending coordinate order, one division range / d, interp_dim's fma, the sample's
// fma).  A single tree that chooses parents by cost and rewires its neighbours; it always runs its whole budget.
//
// The tree of the query a wave is working on lives in the library's scratch, one slab per RESIDENT wave (not per query):
// [max_nodes] x (na doubles, cost, increment, distance to the new state, parent, stamp, goal flag).  Nearest and k-nearest come from
// (distance, index) wave reductions over the node array, k rounds of extraction; neighbour s then lives on lane s (k <= 64, the
// table k(n) is computed on the host: the device never evaluates a logarithm).  The parent walk ranks 64 keys (cost, s) across
// lanes.  A rewire refreshes the costs below the rewired node by stamped sweeps over the node array: a node is refreshed once its
// parent carries the current stamp, until a sweep changes nothing (rewiring breaks parent < child, so one ascending sweep is not
// enough).  Every decision is taken from wave-uniform values, the counters are scalars.  No atomics; all stores are vector
// stores.  A motion check is motion_valid_ends, k_check_motion's loop, with the start row as the env row.

struct StarArgs {
    const double *start, *goal;         // [E, nq]
    long long E;
    double *path;                       // [E, max_path, nq]
    int32_t *path_len, *status;         // [E]
    double *cost;                       // [E] nullable
    long long *info;                    // [E, 8] nullable
    int max_iters, max_nodes, max_path;
    unsigned long long seed, env_id_base;
    const unsigned long long *env_ids, *seeds;      // nullable, as in MopaPlanParams
    double goal_bias, goal_threshold;
    const int32_t *ktab;                // [max_nodes]: ktab[n - 1] = k(n)
    unsigned char *tree;                // one slab of tree_bytes per wave of the launch
    long long tree_bytes;
    int hdr_lds_off, list_lds_off, list_bytes;      // LDS: SceneHdr copy, the waves' vectors, bytes of one wave's vectors
};

constexpr int kStarInfoCols = 8, kStarMaxK = 64;
constexpr long long kStarMaxTreeBytes = 1ll << 30;        // all slabs of a launch

// per wave behind the header copy: [2 * na doubles: the endpoints of the check][na: the sample][na: the new state][na: the goal]
static int star_list_bytes(int na) { return (8 * 5 * na + 15) & ~15; }
static int star_lds_bytes(const MopaScene *S) {
    return ((S->lds_bytes + 15) & ~15) + (((int)sizeof(SceneHdr) + 15) & ~15) + kWavesPerBlock * star_list_bytes(S->na);
}
static int star_node_bytes(int na) { return 8 * na + 24 + 12; }       // one node of k_rrt_star's slab
static long long star_tree_bytes(int max_nodes, int node_bytes) { return ((long long)max_nodes * node_bytes + 15) & ~15ll; }

// reads of the tree at a wave-uniform index: what this wave's vector stores wrote must come back through the vector memory path
MOPA_D double star_ld(const double *p) { return *reinterpret_cast<const volatile double *>(p); }
MOPA_D int star_ldi(const int *p) { return *reinterpret_cast<const volatile int *>(p); }

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_rrt_star(SceneHdr h, const double *__restrict__ g_dbl,
                                                                                               const int32_t *__restrict__ g_int, StarArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + a.hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int na = h.na, nq = h.nq, max_nodes = a.max_nodes;
    double *ends = reinterpret_cast<double *>(smem + a.list_lds_off + wave * a.list_bytes);      // [2][na]
    double *rs = ends + 2 * na, *xs = rs + na, *qg = xs + na;                                     // [na] each
    double *tst = v.qbuf + na + h.n_pq;                                                         // spare [na] doubles behind the joint-value buffer
    const int *adr = v.ints + h.o_act_adr;
    unsigned char *tb = a.tree + (size_t)((long long)blockIdx.x * kWavesPerBlock + wave) * (size_t)a.tree_bytes;
    double *Q = reinterpret_cast<double *>(tb);                     // [max_nodes][na]
    double *cost = Q + (size_t)max_nodes * na;                      // [max_nodes]
    double *inc = cost + max_nodes;                                 // [max_nodes]: distance to the parent
    double *dtmp = inc + max_nodes;                                 // [max_nodes]: distance to the new state of this iteration
    int *parent = reinterpret_cast<int *>(dtmp + max_nodes);        // [max_nodes]
    int *stamp = parent + max_nodes;                                // [max_nodes]: the rewire that last refreshed the node's cost
    int *flags = stamp + max_nodes;                                 // [max_nodes]: 1 = goal node
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long e = (long long)blockIdx.x * kWavesPerBlock + wave; e < a.E; e += stride) {
        const double *row = a.start + (size_t)e * nq, *grow_ = a.goal + (size_t)e * nq;
        double *pe = a.path + (size_t)e * a.max_path * nq;
        const unsigned long long key = rng_key(a.seeds ? a.seeds[e] : a.seed, a.env_ids ? a.env_ids[e] : a.env_id_base + (unsigned long long)e);
        long long n_checks = 0, n_rewire = 0, n_desc = 0, n_full = 0, n_goal = 0, first_goal = -1, its = 0;
        int n = 0, st = MOPA_PLAN_OK, plen = 0;
        double best_cost = __builtin_inf();

        auto uni = [&](bool b) -> bool { return __builtin_amdgcn_readfirstlane((int)b) != 0; };
        auto state_ok = [&](const double *q) -> bool {
            for (int i = lane; i < na; i += 64) tst[i] = q[i];
            wave_sync();
            const bool ok = uni(plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row));
            wave_sync();
            return ok;
        };
        // K2's rule from ends[0..na) to ends[na..2 na)
        auto check_ends = [&]() -> bool {
            n_checks++;
            return motion_valid_ends(h, v, lh, lane, ends, tst, row);
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
            for (int i = lane; i < na; i += 64) Q[i] = rs[i];
            if (lane == 0) { parent[0] = -1; inc[0] = 0.0; cost[0] = 0.0; stamp[0] = 0; flags[0] = 0; }
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
                // 4. first check
                for (int i = lane; i < na; i += 64) { ends[i] = Q[(size_t)nm * na + i]; ends[na + i] = xs[i]; }
                if (!check_ends()) continue;
                // 5. neighbours: lane s holds the s-th nearest node of the new state
                for (int i = lane; i < n; i += 64) dtmp[i] = node_dist(i, xs);
                wave_sync();
                const int kt = star_ldi(a.ktab + (n - 1));
                const int kk = kt < n ? kt : n;
                double my_inc = 0.0, my_c = __builtin_inf();
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
                if (lane < kk) my_c = cost[my_idx] + my_inc;
                // 6. parent: the neighbours in ascending (c, s) order
                int rank = 0;
                for (int t = 0; t < kk; t++) {
                    const double ct = wave_bcast_f64(my_c, t);
                    if (ct < my_c || (ct == my_c && t < lane)) rank++;
                }
                int par = nm, verdict = 0;
                double pinc = node_dist_uniform(nm, xs);
                double pcost = star_ld(cost + nm) + pinc;
                for (int r = 0; r < kk; r++) {
                    const unsigned long long m = __ballot(lane < kk && rank == r);
                    const int s = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1);
                    const int idx = __builtin_amdgcn_readlane(my_idx, s);
                    bool ok = true;
                    if (idx != nm) {
                        for (int i = lane; i < na; i += 64) { ends[i] = Q[(size_t)idx * na + i]; ends[na + i] = xs[i]; }
                        ok = check_ends();
                    }
                    if (lane == s) verdict = ok ? 1 : -1;
                    if (ok) {
                        par = idx;
                        pinc = wave_bcast_f64(my_inc, s);
                        pcost = wave_bcast_f64(my_c, s);
                        break;
                    }
                }
                // 7. append
                for (int i = lane; i < na; i += 64) Q[(size_t)n * na + i] = xs[i];
                if (lane == 0) { parent[n] = par; inc[n] = pinc; cost[n] = pcost; stamp[n] = 0; flags[n] = 0; }
                wave_sync();
                // 8. rewire
                for (int s = 0; s < kk; s++) {
                    const int i = __builtin_amdgcn_readlane(my_idx, s);
                    if (i == par) continue;
                    const double inc_s = wave_bcast_f64(my_inc, s);
                    const double nc = pcost + inc_s;
                    if (!(nc < star_ld(cost + i))) continue;
                    const int vs = __builtin_amdgcn_readlane(verdict, s);
                    bool ok = vs > 0;
                    if (vs == 0) {
                        for (int c = lane; c < na; c += 64) { ends[c] = xs[c]; ends[na + c] = Q[(size_t)i * na + c]; }
                        ok = check_ends();
                    }
                    if (!ok) continue;
                    n_rewire++;
                    cur_stamp++;
                    if (lane == 0) { parent[i] = n; inc[i] = inc_s; cost[i] = nc; stamp[i] = cur_stamp; }
                    wave_sync();
                    // every descendant of i, top down: a node is refreshed once its parent carries this rewire's stamp
                    bool changed = true;
                    while (changed) {
                        changed = false;
                        for (int base = 0; base <= n; base += 64) {
                            const int j = base + lane;
                            bool upd = false;
                            double nv = 0.0;
                            if (j <= n && stamp[j] != cur_stamp) {
                                const int p = parent[j];
                                if (p >= 0 && stamp[p] == cur_stamp) { upd = true; nv = cost[p] + inc[j]; }
                            }
                            wave_sync();
                            if (upd) { cost[j] = nv; stamp[j] = cur_stamp; }
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
            // the goal node of lowest cost (the earliest among equals), its chain to the root
            st = MOPA_PLAN_NO_EXACT;
            if (n_goal > 0) {
                double bc = __builtin_inf();
                int bg = 0x7fffffff;
                for (int j = lane; j < n; j += 64) {
                    const double cj = cost[j];
                    if (flags[j] != 0 && cj < bc) { bc = cj; bg = j; }
                }
                reduce_min(bc, bg);
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
                    best_cost = bc;
                }
            }
        }
        if (lane == 0) {
            a.path_len[e] = plen;
            a.status[e] = st;
            if (a.cost) a.cost[e] = best_cost;
            if (a.info) {
                long long *o = a.info + kStarInfoCols * e;
                o[0] = its; o[1] = n; o[2] = n_checks; o[3] = n_rewire; o[4] = n_goal; o[5] = first_goal; o[6] = n_desc; o[7] = n_full;
            }
        }
        wave_sync();
    }
}

static const LdsKernels kStarLds({(const void *)k_rrt_star});

extern "C" int mopa_star_params_size(void) { return (int)sizeof(MopaStarParams); }

extern "C" int mopa_plan_star_k(int32_t na, int64_t n, double rewire_factor) {
    if (na < 1 || n < 1) return -1;
    const double e = 2.718281828459045;
    const double k_rrt = rewire_factor * (e + e / (double)na);
    const double k = std::ceil(k_rrt * std::log((double)(n + 1)));
    return k > 2147483647.0 ? 2147483647 : (int)k;
}

// What every RRT* entry refuses before a launch (`what`: the entry, `node_bytes`: one node of its tree slab), in this order.
static int star_rules(MopaScene *S, const MopaStarParams &p, int64_t E, const char *what, int node_bytes) {
    if (S->glue_b >= 0) return fail(MOPA_ERR_UNSUPPORTED, std::string(what) + " is not built for a glued scene (glue_bodies)");
    if (E < 0 || p.max_iters < 0 || p.max_nodes < 2 || p.max_path < 2 || !(p.goal_bias >= 0.0 && p.goal_bias <= 1.0) || !(p.goal_threshold >= 0.0) ||
        !(p.rewire_factor > 0.0) || !std::isfinite(p.rewire_factor))
        return fail(MOPA_ERR_INVALID_ARG, "bad RRT* parameters (E < 0, max_iters < 0, max_nodes < 2, max_path < 2, goal_bias outside [0, 1], "
                                          "goal_threshold < 0 or rewire_factor <= 0)");
    if (mopa_plan_star_k(S->na, p.max_nodes, p.rewire_factor) > kStarMaxK)
        return fail(MOPA_ERR_UNSUPPORTED, "RRT*: k(max_nodes) = " + std::to_string(mopa_plan_star_k(S->na, p.max_nodes, p.rewire_factor)) +
                                              " neighbours, the kernel holds one per lane (64)");
    if (star_tree_bytes(p.max_nodes, node_bytes) * kWavesPerBlock > kStarMaxTreeBytes)
        return fail(MOPA_ERR_UNSUPPORTED, "RRT*: the trees of one workgroup (max_nodes = " + std::to_string(p.max_nodes) + ") do not fit the scratch");
    if (star_lds_bytes(S) > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "RRT* LDS does not fit");
    return MOPA_OK;
}

// The launch of an accepted call with E > 0, on the scene's device: the number of persistent workgroups (`per_cu` resident per CU),
// the tree slabs and the table k(n) in the stream's scratch, and the kernel arguments all RRT* kernels share (cost / info: the caller's).
static int star_stage(MopaScene *S, const MopaStarParams &p, const double *start, const double *goal, int64_t E, double *path, int32_t *path_len,
                      int32_t *status, int node_bytes, int per_cu, hipStream_t stream, StarArgs &a, int64_t &nblk) {
    const long long tree_bytes = star_tree_bytes(p.max_nodes, node_bytes);
    // persistent workgroups: `per_cu` per CU are resident; max_workgroups > 0 caps them; fewer where the trees ask for it
    nblk = std::min<int64_t>((E + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)S->n_cu * per_cu);
    if (p.max_workgroups > 0) nblk = std::min<int64_t>(nblk, p.max_workgroups);
    nblk = std::max<int64_t>(1, std::min<int64_t>(nblk, kStarMaxTreeBytes / (tree_bytes * kWavesPerBlock)));
    StreamScratch &sc = scratch_for(S, stream);
    HIP_TRY(grow(S, sc.star_tree, (size_t)nblk * kWavesPerBlock * (size_t)tree_bytes));
    // the table k(n), n = 1 .. max_nodes: a prefix of every longer table of the same rewire_factor, so it is uploaded when it grows
    // or the factor changes (synchronously, into a buffer of its own: launches in flight keep reading the one they were given)
    if (sc.star_k_n < p.max_nodes || sc.star_k_rf != p.rewire_factor) {
        const int cnt = std::max(p.max_nodes, 4096);
        std::vector<int32_t> tab((size_t)cnt);
        for (int n = 1; n <= cnt; n++) tab[(size_t)n - 1] = mopa_plan_star_k(S->na, n, p.rewire_factor);
        DevBuf nb;
        HIP_TRY(grow(S, nb, sizeof(int32_t) * (size_t)cnt));
        HIP_TRY(hipMemcpy(nb.p, tab.data(), sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice));
        if (sc.star_k.p) {
            std::lock_guard<std::mutex> lock(S->mu);
            S->retired.push_back(sc.star_k.p);
        }
        sc.star_k = nb;
        sc.star_k_n = cnt;
        sc.star_k_rf = p.rewire_factor;
    }
    a.start = start; a.goal = goal; a.E = (long long)E; a.path = path; a.path_len = path_len; a.status = status; a.cost = nullptr; a.info = nullptr;
    a.max_iters = p.max_iters; a.max_nodes = p.max_nodes; a.max_path = p.max_path; a.seed = p.seed; a.env_id_base = p.env_id_base;
    a.env_ids = reinterpret_cast<const unsigned long long *>(p.env_ids_dev); a.seeds = reinterpret_cast<const unsigned long long *>(p.seeds_dev);
    a.goal_bias = p.goal_bias; a.goal_threshold = p.goal_threshold;
    a.ktab = sc.star_k.as<int32_t>(); a.tree = sc.star_tree.as<unsigned char>(); a.tree_bytes = tree_bytes;
    a.hdr_lds_off = (S->lds_bytes + 15) & ~15;
    a.list_lds_off = a.hdr_lds_off + (((int)sizeof(SceneHdr) + 15) & ~15);
    a.list_bytes = star_list_bytes(S->na);
    return MOPA_OK;
}

extern "C" int mopa_plan_star_batch(MopaScene *S, const double *start, const double *goal, int64_t E, const MopaStarParams *params, double *path,
                                    int32_t *path_len, int32_t *status, double *cost, int64_t *info, void *stream) {
    if (!S || !params || (E > 0 && (!start || !goal || !path || !path_len || !status))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const int node_bytes = star_node_bytes(S->na);
    if (const int rc = star_rules(S, *params, E, "RRT* (mopa_plan_star)", node_bytes)) return rc;
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    StarArgs a;
    int64_t nblk;
    // two workgroups per CU are resident (two waves per SIMD)
    if (const int rc = star_stage(S, *params, start, goal, E, path, path_len, status, node_bytes, 2, (hipStream_t)stream, a, nblk)) return rc;
    a.cost = cost;
    a.info = reinterpret_cast<long long *>(info);
    hipLaunchKernelGGL(k_rrt_star, dim3((unsigned)nblk), dim3(kBlock), star_lds_bytes(S), (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, a);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// the single-query host form (mopa_plan's shape): stream id = env_id_base, the default stream, synchronous
extern "C" int mopa_plan_star(MopaScene *S, const double *start_host, const double *goal_host, const MopaStarParams *params, double *path_host,
                              int32_t *path_len_out, int32_t *status_out, double *cost_out, int64_t *info_out) {
    if (!S || !start_host || !goal_host || !params || !path_host || !path_len_out || !status_out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (params->max_path < 2) return fail(MOPA_ERR_INVALID_ARG, "max_path < 2");
    MOPA_REFUSE_GLUED(S, "RRT* (mopa_plan_star)");
    MopaStarParams one = *params;
    one.env_ids_dev = nullptr;
    one.seeds_dev = nullptr;
    // further outputs: cost | info[kStarInfoCols]
    return plan_single(S, start_host, goal_host, params->max_path, path_host, path_len_out, status_out, 8 * (1 + kStarInfoCols),
        [&](const double *s, const double *g, double *p, int32_t *len, int32_t *st, void *x) {
            return mopa_plan_star_batch(S, s, g, 1, &one, p, len, st, static_cast<double *>(x), static_cast<int64_t *>(x) + 1, nullptr);
        },
        [&](const void *x) {
            hipError_t e = cost_out ? hipMemcpy(cost_out, x, 8, hipMemcpyDeviceToHost) : hipSuccess;
            if (e == hipSuccess && info_out) e = hipMemcpy(info_out, static_cast<const int64_t *>(x) + 1, 8 * kStarInfoCols, hipMemcpyDeviceToHost);
            return e;
        });
}
