// mopa_proximity.inc -- batched proximity report: how far from collision a state is, and which pairs are nearest, inside a band.
// What a user of a collision-checked planner asks besides the verdict; the reference's maximize_min_clearance objective reads it.
//
// One launch (DESIGN.md section 4, "Proximity report"): persistent waves pull states from the reports' counter (wave_pull64), one
// state per pull, and EVERY state gets a wave -- there is no stage-1 gate, a separated state has a clearance too.  Per state: the
// wave-per-state validity routine's wave_load_state / wave_fk, the shared pair sweep (wave_broad_phase / wave_each_survivor,
// mopa_hip.hip) with a MARGIN cull (pair_culled_band: every bound of pair_culled widened by the band, so no pair at distance
// <= band is dropped) and geom_sep (mopa_sep.hpp) for the survivors, then the selection.
// Every distance lands in a per-wave LDS array indexed by the pair's position in the MopaSceneDesc pair list (kFar = out of band);
// the count is a ballot over it, the K nearest come out of min(K, count) rounds of a wave-wide minimum over (distance, pair index)
// (wave_argmin) -- ties to the lower index, no atomics, one writer per output word: two runs write the same bytes.
// EXACT = true (the *_exact entry points): the same kernel with geom_sep's exact route (gjk_distance) in the lambda; nothing else changes.

template <bool MESH, bool EXACT = false>
__global__ __launch_bounds__(kBlock) void k_proximity_rows(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                           const int32_t *__restrict__ pair_model /*[h.npair] device pair -> index in the desc's pair list*/,
                                                           int npair_model, const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                           long long N, long long samples_per_env, double band, int K,
                                                           unsigned long long *__restrict__ ctr, double *__restrict__ clearance,
                                                           int32_t *__restrict__ count, int32_t *__restrict__ pair, double *__restrict__ dist,
                                                           int pd_off /*byte offset of the per-wave distance arrays in LDS*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double *pd = reinterpret_cast<double *>(smem + pd_off) + wave * npair_model;   // [npair_model] distance by pair index, kFar = out of band
    const int *I = v.ints;
    for (;;) {
        const long long s = wave_pull64(ctr, lane);
        if (s >= N) break;
        wave_load_state(h, v, lane, q_active + s * h.na, qpos_env + (s / samples_per_env) * h.nq);
        wave_fk(h, v, lane);
        for (int i = lane; i < npair_model; i += 64) pd[i] = kFar;
        // margin broad phase
        const int wl_count = wave_broad_phase(h, v, lane, CullBand{band});
        wave_each_survivor(h, v, lane, wl_count, [&](int p, int g1, int g2, int code) {
            pd[pair_model[p]] = geom_sep<MESH, 1, EXACT>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], band, v.dbl);
        });
        wave_sync();
        int cnt = 0;
        for (int base = 0; base < npair_model; base += 64) {
            const int p = base + lane;
            const double d = (p < npair_model) ? pd[p] : kFar;
            cnt += __popcll(__ballot(d <= band && d < kFar));
        }
        // the K nearest, ascending by (distance, pair index): one wave-wide minimum per record
        const int nrec = cnt < K ? cnt : K;
        for (int r = 0; r < nrec; r++) {
            double bd = kFar;
            int bi = 0x7fffffff;
            for (int p = lane; p < npair_model; p += 64) {
                const double d = pd[p];
                if (d < bd) { bd = d; bi = p; }      // (ascending p within a lane: the first minimum is the lowest index)
            }
            wave_argmin(bd, bi);
            if (lane == 0) {
                pair[s * K + r] = bi;
                dist[s * K + r] = bd;
                if (r == 0) clearance[s] = bd;
            }
            if (bi < npair_model && (bi & 63) == lane) pd[bi] = kFar;      // (cnt counted it: bi names an entry below kFar)
            wave_sync();
        }
        row_fill_unused(pair, dist, s, K, nrec, lane);
        if (lane == 0) {
            count[s] = cnt;
            if (cnt == 0) clearance[s] = band;
        }
        wave_sync();   // pd / worklist / geom slab are about to be reused
    }
    tile_ctr_release(ctr, lane);
}

// pair level: one lane per posed pair; a mesh (type 7) as the second geom reads the hull at mesh_verts
__global__ __launch_bounds__(256) void k_geom_sep(long long M, const int32_t *__restrict__ types /*[M,2]*/, const double *__restrict__ recs /*[M,2,15]*/,
                                                  const double *__restrict__ mesh_verts /*[nvert,3] or null*/, int nvert, double band,
                                                  double *__restrict__ out /*[M]*/) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    out[i] = geom_sep_rec(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, mesh_verts, nvert, band);
}
// ... with geom_sep's exact route
__global__ __launch_bounds__(256) void k_geom_sep_exact(long long M, const int32_t *__restrict__ types /*[M,2]*/, const double *__restrict__ recs /*[M,2,15]*/,
                                                        const double *__restrict__ mesh_verts /*[nvert,3] or null*/, int nvert, double band,
                                                        double *__restrict__ out /*[M]*/) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    out[i] = geom_sep_rec<true>(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, mesh_verts, nvert, band);
}

static const LdsKernels kProximityLds({(const void *)k_proximity_rows<false>, (const void *)k_proximity_rows<true>,
                                       (const void *)k_proximity_rows<false, true>, (const void *)k_proximity_rows<true, true>});

// the band of the proximity and clearance reports and of geom_sep
static int band_rule(double band) {
    if (!std::isfinite(band) || !(band >= 0.0)) return fail(MOPA_ERR_INVALID_ARG, "band must be finite and >= 0");
    return MOPA_OK;
}

static int proximity_batch(bool exact, MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env, double band,
                           int32_t K, double *clearance, int32_t *count, int32_t *pair, double *dist, void *stream) {
    if (!S || !clearance || !count || !pair || !dist || (N > 0 && (!q_active || !qpos_env))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the proximity report (mopa_proximity_batch)");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    if (const int rc = band_rule(band)) return rc;
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_pairs must be >= 1");
    if (S->pruned) return refuse_pruned("the proximity report needs");
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    int pd_off;
    size_t lds;
    int rc = pair_dist_lds(S, "proximity report", &pd_off, &lds);
    if (rc != MOPA_OK) return rc;
    StreamScratch &sc = scratch_for(S, st);
    rc = ensure_report_ctr(S, sc);
    if (rc != MOPA_OK) return rc;
    const auto kern = exact ? (S->hdr.has_mesh ? k_proximity_rows<true, true> : k_proximity_rows<false, true>)
                            : (S->hdr.has_mesh ? k_proximity_rows<true> : k_proximity_rows<false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)report_blocks(S, N)), dim3(kBlock), lds, st, S->hdr, S->d_dbl, S->d_int,
                       (const int32_t *)S->d_pair_model, S->npair_model, q_active, qpos_env, (long long)N, (long long)samples_per_env, band, (int)K,
                       sc.ct_ctr.as<unsigned long long>(), clearance, count, pair, dist, pd_off);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
extern "C" int mopa_proximity_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env, double band,
                                    int32_t K, double *clearance, int32_t *count, int32_t *pair, double *dist, void *stream) {
    return proximity_batch(false, S, q_active, qpos_env, N, samples_per_env, band, K, clearance, count, pair, dist, stream);
}
extern "C" int mopa_proximity_exact_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env, double band,
                                          int32_t K, double *clearance, int32_t *count, int32_t *pair, double *dist, void *stream) {
    return proximity_batch(true, S, q_active, qpos_env, N, samples_per_env, band, K, clearance, count, pair, dist, stream);
}

static int proximity_state(bool exact, MopaScene *S, const double *qpos_host, double band, int32_t K, double *clearance, int32_t *count, int32_t *pair,
                           double *dist) {
    if (!S || !qpos_host || !clearance || !count || !pair || !dist) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the proximity report (mopa_proximity_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_pairs must be >= 1");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    Staging g;
    const auto f_dist = g.dbl(K), f_clear = g.dbl(1);
    const auto f_pair = g.i32(K), f_count = g.i32(1);
    HIP_TRY(g.alloc());
    rc = proximity_batch(exact, S, S->d_q + S->nq, S->d_q, 1, 1, band, K, g.dev(f_clear), g.dev(f_count), g.dev(f_pair), g.dev(f_dist), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_dist, dist); g.out(f_clear, clearance); g.out(f_pair, pair); g.out(f_count, count);
    return MOPA_OK;
}
extern "C" int mopa_proximity_state(MopaScene *S, const double *qpos_host, double band, int32_t K, double *clearance, int32_t *count, int32_t *pair,
                                    double *dist) {
    return proximity_state(false, S, qpos_host, band, K, clearance, count, pair, dist);
}
extern "C" int mopa_proximity_exact_state(MopaScene *S, const double *qpos_host, double band, int32_t K, double *clearance, int32_t *count, int32_t *pair,
                                          double *dist) {
    return proximity_state(true, S, qpos_host, band, K, clearance, count, pair, dist);
}

static int geom_sep_batch(bool exact, int32_t device, int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band,
                          double *out, void *stream) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr, mesh_verts, nvert)) return rc;
    if (const int rc = band_rule(band)) return rc;
    return pair_launch(device, exact ? k_geom_sep_exact : k_geom_sep, M, stream, types, recs, mesh_verts, (int)nvert, band, out);
}
extern "C" int mopa_geom_sep_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band,
                                   double *out, void *stream) {
    return geom_sep_batch(false, device, M, types, recs, mesh_verts, nvert, band, out, stream);
}
extern "C" int mopa_geom_sep_exact_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert,
                                         double band, double *out, void *stream) {
    return geom_sep_batch(true, device, M, types, recs, mesh_verts, nvert, band, out, stream);
}

// The host compile of the same functions: the sequential form the kernels must match bit for bit.  No GPU, no HIP call.
template <bool EXACT>
static int geom_sep_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band, double *out, int32_t *iters_out) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr, mesh_verts, nvert)) return rc;
    if (const int rc = band_rule(band)) return rc;
    for (int64_t i = 0; i < M; i++) {
        int it = 0;
        out[i] = geom_sep_rec<EXACT>(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, mesh_verts, nvert, band, &it);
        if (iters_out) iters_out[i] = it;
    }
    return MOPA_OK;
}
extern "C" int mopa_geom_sep_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band, double *out) {
    return geom_sep_host<false>(M, types, recs, mesh_verts, nvert, band, out, nullptr);
}
// iters_out [M] (nullable): the exact route's number of support evaluations, 0 where it was not taken, negative where its cap ended it
extern "C" int mopa_geom_sep_exact_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band, double *out,
                                        int32_t *iters_out) {
    return geom_sep_host<true>(M, types, recs, mesh_verts, nvert, band, out, iters_out);
}
