// mopa_race.inc -- K3 race: every query is run by `portfolio` = K RRT-Connect members that share start, goal, env row and stream id and
// differ in their seed only (member m: seed + m * kRaceSeedStep; member 0 is the query mopa_plan_batch runs).  The result of a query is
// that of ONE member -- the solved one with the smallest (consumed checks, m) -- whatever the timing:
//   * k_rrt_connect<K3Race> (the race build of mopa_planner_k3.inc, on the one-wave-per-SIMD settings of K3W1): launch slot v
//     is member v / E of query v % E, so every query gets its first member before any query gets a second.  A member writes no path
//     rows; it leaves a record (status, consumed checks, iterations, the two motions of its solution, their row count) and its trees
//     in the launch's scratch.
//   * the race word: one uint64 per query, all-ones before every launch.  A member that solves does an atomic min of
//     key = consumed checks * K + m; at the top of every iteration a member compares its count so far * K + m with the word and stops
//     ("cut") when that is larger.  Consumed checks only grow, so a member is cut only when it could no longer win, and the member
//     with the smallest final key can never be cut: the winner is the sequential form's (tests/race_ref.py) whatever the dispatch
//     order.  A stale read only delays a cut.  No member waits for another.
//   * k_race_pick, behind it on the stream, one wave per query: arg-min of the keys of the solved members, the winner's two trees traced
//     into the caller's path rows by k_rrt_connect's row writer (plan_write_rows), the outputs.  No atomics, no read-back.
// (included by mopa_planner.inc behind the planner body and mopa_plan_batch; RaceArgs and the race's constants, which the body names,
//  are defined in mopa_planner.inc in front of the body)

__global__ __launch_bounds__(kBlock) void k_race_pick(int na, int nq, int o_act_adr, const int32_t *__restrict__ g_int, const double *__restrict__ start,
                                                      long long E, int K, int max_nodes, int max_path, unsigned long long seed,
                                                      const uint64_t *__restrict__ seeds_dev, PlanWs ws, const long long *__restrict__ rec,
                                                      double *__restrict__ path, int32_t *__restrict__ path_len, int32_t *__restrict__ status,
                                                      long long *__restrict__ n_checks, int32_t *__restrict__ winner,
                                                      unsigned long long *__restrict__ win_seed, long long *__restrict__ info) {
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * kWavesPerBlock;
    for (long long g = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < E; g += nw) {
        unsigned long long best = ~0ull;
        long long spent = 0;
        int cut = 0;
        for (int m = lane; m < K; m += 64) {
            const long long *r = rec + (size_t)kRaceRec * (size_t)((long long)m * E + g);
            const long long st = r[0], chk = r[1];
            spent += chk;
            cut += st == kRaceCut ? 1 : 0;
            if (st == MOPA_PLAN_OK) {
                const unsigned long long key = (unsigned long long)chk * (unsigned long long)K + (unsigned long long)m;
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long ob = __shfl_xor(best, off, 64);
            best = ob < best ? ob : best;
            spent += __shfl_xor(spent, off, 64);
            cut += __shfl_xor(cut, off, 64);
        }
        const int w = best == ~0ull ? -1 : (int)(best % (unsigned long long)K);
        const long long *r0 = rec + (size_t)kRaceRec * (size_t)g;                                          // member 0
        const long long *rw = rec + (size_t)kRaceRec * (size_t)((long long)(w < 0 ? 0 : w) * E + g);       // the winner (none: member 0)
        int plen = 0;
        if (w >= 0) {
            const size_t slot = (size_t)((long long)w * E + g);
            const double *tq0 = ws.tree_q + slot * 2 * (size_t)max_nodes * na, *tq1 = tq0 + (size_t)max_nodes * na;
            const int32_t *tp0 = ws.tree_parent + slot * 2 * (size_t)max_nodes, *tp1 = tp0 + max_nodes;
            const double *row = start + g * nq;
            double *pe = path + (size_t)g * max_path * nq;
            const int sm = (int)rw[3], gm = (int)rw[4];
            const int total = (int)rw[5];          // n1 + n2 <= max_path: checked by the member before it reported "solved"
            int n1 = 0;
            for (int m = sm; m >= 0 && m < max_nodes && n1 < total; m = tp0[m]) n1++;
            // (a row index outside the path never is written)
            plan_write_rows<true>(lane, na, nq, g_int + o_act_adr, row, pe, tq0, tp0, tq1, tp1, sm, gm, n1, max_nodes, total, max_path);
            plen = total;
        }
        if (lane == 0) {
            const unsigned long long seed_g = seeds_dev ? seeds_dev[g] : seed;
            path_len[g] = plen;
            status[g] = w >= 0 ? MOPA_PLAN_OK : (r0[0] == MOPA_PLAN_INVALID_GOAL ? MOPA_PLAN_INVALID_GOAL : MOPA_PLAN_NO_EXACT);
            n_checks[g] = rw[1];
            winner[g] = w;
            win_seed[g] = seed_g + (unsigned long long)(w < 0 ? 0 : w) * kRaceSeedStep;
            if (info) {
                info[3 * g] = cut;
                info[3 * g + 1] = spent;
                info[3 * g + 2] = w >= 0 ? rw[2] : -1ll;
            }
        }
        wave_sync();
    }
}

extern "C" int mopa_race_params_size(void) { return (int)sizeof(MopaRaceParams); }

extern "C" int mopa_plan_race_batch(MopaScene *S, const double *start, const double *goal, int64_t E, const MopaRaceParams *params, double *path,
                                    int32_t *path_len, int32_t *status, int64_t *n_checks, int32_t *winner, uint64_t *win_seed, int64_t *info,
                                    void *stream) {
    if (!S || !params || (E > 0 && (!start || !goal || !path || !path_len || !status || !n_checks || !winner || !win_seed)))
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E < 0 || params->max_nodes < 2 || params->max_path < 2 || params->max_iters < 0)
        return fail(MOPA_ERR_INVALID_ARG, "bad plan parameters");
    if (params->portfolio < 1 || params->portfolio > 256) return fail(MOPA_ERR_INVALID_ARG, "portfolio must be 1 .. 256");
    MOPA_REFUSE_GLUED(S, "the K3 race (mopa_plan_race)");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    const int K = params->portfolio;
    const int64_t slots = E * (int64_t)K;
    // trees of every member: E * K * 2 * max_nodes * na doubles (+ pad: nn_node8 reads 8 doubles per node) plus parents
    const double need_q = (double)slots * 2.0 * (double)params->max_nodes * S->na * 8.0 + 64.0, need_p = (double)slots * 2.0 * (double)params->max_nodes * 4.0;
    {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (need_q + need_p > (double)total_b) {
            char msg[160];
            snprintf(msg, sizeof msg, "race tree scratch of %.0f bytes (E * portfolio * 2 * max_nodes trees) exceeds the device's %zu bytes", need_q + need_p, total_b);
            return fail(MOPA_ERR_LIMIT, msg);
        }
    }
    StreamScratch &sc = scratch_for(S, st);
    if (grow(S, sc.plan_q, (size_t)need_q) != hipSuccess || grow(S, sc.plan_p, (size_t)need_p) != hipSuccess) {
        (void)hipGetLastError();
        char msg[160];
        snprintf(msg, sizeof msg, "race tree scratch of %.0f bytes (E * portfolio * 2 * max_nodes trees) could not be allocated", need_q + need_p);
        return fail(MOPA_ERR_LIMIT, msg);
    }
    HIP_TRY(grow(S, sc.race_rec, (size_t)slots * kRaceRec * sizeof(long long)));
    HIP_TRY(grow(S, sc.race_word, (size_t)E * sizeof(unsigned long long)));
    PlanWs ws{sc.plan_q.as<double>(), sc.plan_p.as<int32_t>()};
    // mopa_plan_batch's policy over the E * K slots.  The build holds one wave per SIMD, so a CU holds one workgroup at a time: the
    // launch always asks for more than half a CU's LDS and the rest of the CU's LDS holds the FP32 tree mirrors of its four members
    PlanGeom g;
    if (const int rc = plan_geometry(S, sc, slots, params->max_workgroups, params->max_nodes, true, 0, g)) return rc;
    if (std::getenv("MOPA_DEBUG")) fprintf(stderr, "[mopa] race launch: %lld queries x %d members, %lld workgroups, mirror %d nodes/member, LDS %d bytes\n", (long long)E, K, (long long)g.nblk, g.nn_cap, g.lds_launch);
    MopaPlanParams prm{};
    prm.max_iters = params->max_iters; prm.max_nodes = params->max_nodes; prm.max_path = params->max_path;
    prm.seed = params->seed; prm.env_id_base = params->env_id_base; prm.env_ids_dev = params->env_ids_dev; prm.seeds_dev = params->seeds_dev;
    RaceArgs ra{(long long)E, K, params->no_abort ? 1 : 0, sc.race_word.as<unsigned long long>(), sc.race_rec.as<long long>()};
    // all-ones in front of EVERY launch: the kernel never relies on what an earlier launch left in the word
    HIP_TRY(hipMemsetAsync(sc.race_word.p, 0xff, (size_t)E * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_rrt_connect<K3Race>, dim3((unsigned)g.nblk), dim3(kBlock), g.lds_launch, st, S->hdr, S->d_dbl, S->d_int, start, goal, (long long)slots, prm, ws,
                       (double *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (long long *)nullptr, g.scene_bytes, g.ctr, g.nn_cap, ra);
    HIP_TRY(hipGetLastError());
    const int64_t pick_blocks = std::max<int64_t>(1, std::min<int64_t>((E + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)S->n_cu * 8));
    hipLaunchKernelGGL(k_race_pick, dim3((unsigned)pick_blocks), dim3(kBlock), 0, st, S->na, S->nq, S->hdr.o_act_adr, S->d_int, start, (long long)E, K, params->max_nodes,
                       params->max_path, (unsigned long long)params->seed, params->seeds_dev, ws, sc.race_rec.as<long long>(), path, path_len, status,
                       (long long *)n_checks, winner, (unsigned long long *)win_seed, (long long *)info);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_plan_race(MopaScene *S, const double *start_host, const double *goal_host, const MopaRaceParams *params, double *path_host,
                              int32_t *path_len_out, int32_t *status_out, int64_t *n_checks_out, int32_t *winner_out, uint64_t *win_seed_out,
                              int64_t *info_out) {
    if (!S || !start_host || !goal_host || !params || !path_host || !path_len_out || !status_out)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (params->max_path < 2) return fail(MOPA_ERR_INVALID_ARG, "bad plan parameters");
    MOPA_REFUSE_GLUED(S, "the K3 race (mopa_plan_race)");
    MopaRaceParams one = *params;
    one.env_ids_dev = nullptr;   // single query: the stream id is env_id_base
    one.seeds_dev = nullptr;
    one.max_workgroups = 0;
    long long out[6];            // [0] checks [1] win_seed [2..4] info [5] winner
    const int rc = plan_single(S, start_host, goal_host, params->max_path, path_host, path_len_out, status_out, sizeof out,
        [&](const double *s, const double *g, double *p, int32_t *len, int32_t *st, void *x) {
            long long *o = static_cast<long long *>(x);
            return mopa_plan_race_batch(S, s, g, 1, &one, p, len, st, (int64_t *)o, reinterpret_cast<int32_t *>(o + 5), reinterpret_cast<uint64_t *>(o + 1), (int64_t *)(o + 2), nullptr);
        },
        [&](const void *x) { return hipMemcpy(out, x, sizeof out, hipMemcpyDeviceToHost); });
    if (rc == MOPA_OK) {
        int32_t win;
        std::memcpy(&win, out + 5, 4);
        if (n_checks_out) *n_checks_out = out[0];
        if (winner_out) *winner_out = win;
        if (win_seed_out) *win_seed_out = (uint64_t)out[1];
        if (info_out) { info_out[0] = out[2]; info_out[1] = out[3]; info_out[2] = out[4]; }
    }
    return rc;
}
