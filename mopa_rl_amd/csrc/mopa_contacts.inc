// mopa_contacts.inc -- batched contact report: which candidate pairs of a state lie at or below a (negative) cutoff, and how deep.
// What the reference reads off d->contact[i].geom1 / geom2 / dist (mujoco_ompl_interface.cpp:917-978), for N states at once.
//
// Two stages (DESIGN.md section 4, "Contact report"):
//   1. the min-depth launch of mopa_is_valid_batch: a state has a record iff its deepest penetration is <= cutoff.  Exact for
//      cutoff < 0 (the broad phase culls at zero margin: it only ever drops separated pairs).
//   2. k_contact_rows (here): persistent waves pull chunks of states from a counter; rows of states without a record are filled with
//      the "unused" pattern, every other state gets one wave: the FK and pair sweep of the wave-per-state validity routine
//      (wave_load_state / wave_fk / wave_broad_phase over pair_culled / geom_dist -- what k_is_valid, k_debug_state and
//      plan_state_valid_impl are made of) with NO verdict early-out and NO deep-overlap shortcut (wave_each_survivor), so a
//      distance carries the bits mopa_debug_pair_dist reports.
// Order: every distance lands in a per-wave LDS array indexed by the pair's position in the MopaSceneDesc pair list; the wave then
// emits records in that order with a ballot and a prefix popcount -- ascending pair index and "the lowest K are kept" without atomics,
// so two runs write the same bytes.

template <bool MESH>
__global__ __launch_bounds__(kBlock) void k_contact_rows(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                         const int32_t *__restrict__ pair_model /*[h.npair] device pair -> index in the desc's pair list*/,
                                                         int npair_model, const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                         long long N, long long samples_per_env, const double *__restrict__ min_dist /*[N] stage 1*/,
                                                         double cutoff, int K, int chunk /*1..64 states per pull*/, unsigned long long *__restrict__ ctr,
                                                         int32_t *__restrict__ count, int32_t *__restrict__ pair, double *__restrict__ dist,
                                                         int pd_off /*byte offset of the per-wave distance arrays in LDS*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double *pd = reinterpret_cast<double *>(smem + pd_off) + wave * npair_model;   // [npair_model] distance by pair index, kFar = no record
    const int *I = v.ints;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (;;) {
        const long long s0 = wave_pull64(ctr, lane) * chunk;
        if (s0 >= N) break;
        const int n = (int)((N - s0 < (long long)chunk) ? (N - s0) : (long long)chunk);
        const bool kept = lane < n && min_dist[s0 + lane] <= cutoff;
        unsigned long long km = __ballot(kept);
        // states without a record: count 0, the whole row unused
        for (long long e = lane; e < (long long)n * K; e += 64) {
            const int ls = (int)(e / K);
            if (!((km >> ls) & 1ull)) {
                pair[s0 * K + e] = -1;
                dist[s0 * K + e] = kFar;
            }
        }
        if (lane < n && !kept) count[s0 + lane] = 0;
        while (km) {
            const int ls = __ffsll((long long)km) - 1;
            km &= km - 1ull;
            const long long s = s0 + ls;
            wave_load_state(h, v, lane, q_active + s * h.na, qpos_env + (s / samples_per_env) * h.nq);
            wave_fk(h, v, lane);
            for (int i = lane; i < npair_model; i += 64) pd[i] = kFar;
            const int wl_count = wave_broad_phase(h, v, lane, CullZeroMargin{});
            // narrow phase over every survivor, full refinement
            wave_each_survivor(h, v, lane, wl_count, [&](int p, int g1, int g2, int code) {
                pd[pair_model[p]] = geom_dist<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl);
            });
            wave_sync();
            // records in pair-index order; the count runs on past K
            int cnt = 0;
            for (int base = 0; base < npair_model; base += 64) {
                const int p = base + lane;
                const double d = (p < npair_model) ? pd[p] : kFar;
                const bool hit = d <= cutoff;
                const unsigned long long mask = __ballot(hit);
                const int idx = cnt + __popcll(mask & lt);
                if (hit && idx < K) {
                    pair[s * K + idx] = p;
                    dist[s * K + idx] = d;
                }
                cnt += __popcll(mask);
            }
            row_fill_unused(pair, dist, s, K, cnt, lane);
            if (lane == 0) count[s] = cnt;
            wave_sync();   // pd / worklist / geom slab are about to be reused
        }
    }
    tile_ctr_release(ctr, lane);
}

static const LdsKernels kContactsLds({(const void *)k_contact_rows<false>, (const void *)k_contact_rows<true>});

extern "C" int mopa_contacts_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                   double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist, void *stream) {
    if (!S || !count || !pair || !dist || (N > 0 && (!q_active || !qpos_env))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contacts_batch)");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    if (!std::isfinite(cutoff) || !(cutoff < 0.0)) return fail(MOPA_ERR_INVALID_ARG, "cutoff must be finite and < 0 (the broad phase culls at zero margin)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1");
    if (S->pruned && cutoff > S->hdr.thr) return refuse_pruned("cutoff > contact_threshold needs");
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    int pd_off;
    size_t lds;
    int rc = pair_dist_lds(S, "contact report", &pd_off, &lds);
    if (rc != MOPA_OK) return rc;
    StreamScratch &sc = scratch_for(S, st);
    HIP_TRY(grow(S, sc.ct_valid, (size_t)N));
    HIP_TRY(grow(S, sc.ct_md, (size_t)N * sizeof(double)));
    rc = ensure_report_ctr(S, sc);
    if (rc != MOPA_OK) return rc;
    // stage 1: deepest penetration of every state
    rc = launch_is_valid(S, q_active, qpos_env, N, samples_per_env, nullptr, sc.ct_valid.as<uint8_t>(), sc.ct_md.as<double>(), stream);
    if (rc != MOPA_OK) return rc;
    // stage 2: persistent waves (189 / 191 VGPRs); small batches are handed out state by state, large ones in chunks of up to 64
    const int64_t blocks = report_blocks(S, N);
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(64, N / (blocks * kWavesPerBlock * 8)));
    hipLaunchKernelGGL(S->hdr.has_mesh ? k_contact_rows<true> : k_contact_rows<false>, dim3((unsigned)blocks), dim3(kBlock), lds, st, S->hdr, S->d_dbl, S->d_int,
                       (const int32_t *)S->d_pair_model, S->npair_model, q_active, qpos_env, (long long)N, (long long)samples_per_env,
                       (const double *)sc.ct_md.as<double>(), cutoff, (int)K, chunk, sc.ct_ctr.as<unsigned long long>(), count, pair, dist, pd_off);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_contacts_state(MopaScene *S, const double *qpos_host, double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist) {
    if (!S || !qpos_host || !count || !pair || !dist) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contacts_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    Staging g;
    const auto f_dist = g.dbl(K);
    const auto f_pair = g.i32(K), f_count = g.i32(1);
    HIP_TRY(g.alloc());
    rc = mopa_contacts_batch(S, S->d_q + S->nq, S->d_q, 1, 1, cutoff, K, g.dev(f_count), g.dev(f_pair), g.dev(f_dist), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_dist, dist); g.out(f_pair, pair); g.out(f_count, count);
    return MOPA_OK;
}
