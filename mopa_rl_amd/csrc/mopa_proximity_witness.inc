// mopa_proximity_witness.inc -- witness points of the batched proximity report: for every record of mopa_proximity_exact_batch the
// two closest points of the pair and the unit direction between them (mopa_witness.hpp: geom_witness).
//
// A kernel of its own BEHIND k_proximity_rows<MESH, true>, reading the rows that one wrote, as k_contact_frames does behind
// k_contact_rows: without witnesses the report's launch, its registers and its bytes are what they are (DESIGN.md section 4,
// "Witness points", has the resource rows behind the choice: the GJK walk with a support point of A per simplex vertex does not fit
// k_proximity_rows' budget).  Mapping as there, a wave per state with a record: the wave poses the state (wave_load_state / wave_fk),
// then the lanes that own a record with slot < min(count, K) run geom_witness on their pair and store n / p1 / p2; every other slot
// is written 0.0.  Each output word has exactly one writer: two runs write the same bytes.

template <bool MESH>
__global__ __launch_bounds__(kBlock) void k_proximity_witness(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                              const int32_t *__restrict__ pair_slot /*[npair_model] model pair -> device pair or -1*/,
                                                              int npair_model, const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                              long long N, long long samples_per_env, double band, int K,
                                                              const int32_t *__restrict__ count /*[N]*/, const int32_t *__restrict__ pair /*[N,K]*/,
                                                              double *__restrict__ normal /*[N,K,3]*/, double *__restrict__ p1o /*[N,K,3]*/,
                                                              double *__restrict__ p2o /*[N,K,3]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int *I = v.ints;
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long s = (long long)blockIdx.x * kWavesPerBlock + wave; s < N; s += stride) {
        const int cnt = __builtin_amdgcn_readfirstlane(count[s]);
        const int nrec = cnt < K ? cnt : K;
        if (nrec > 0) {
            wave_load_state(h, v, lane, q_active + s * h.na, qpos_env + (s / samples_per_env) * h.nq);
            wave_fk(h, v, lane);
        }
        for (int slot = lane; slot < K; slot += 64) {
            V3 n{0.0, 0.0, 0.0}, a{0.0, 0.0, 0.0}, b{0.0, 0.0, 0.0};
            if (slot < nrec) {
                const int p = pair[s * K + slot];
                const int dp = (p >= 0 && p < npair_model) ? pair_slot[p] : -1;
                if (dp >= 0 && dp < h.npair) {
                    const int pk = I[h.o_pairs + dp];
                    const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
                    // (the scene's pairs are in the narrow phase's order already, as in k_contact_frames: p1 lies on pair_geom's first geom)
                    (void)geom_witness<MESH, 1>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], band, v.dbl, n, a, b);
                }
            }
            const long long o = (s * K + slot) * 3;
            normal[o] = n.x; normal[o + 1] = n.y; normal[o + 2] = n.z;
            p1o[o] = a.x; p1o[o + 1] = a.y; p1o[o + 2] = a.z;
            p2o[o] = b.x; p2o[o + 1] = b.y; p2o[o + 2] = b.z;
        }
        if (nrec > 0) wave_sync();   // the geom slab is about to be reused
    }
}

// pair level: one lane per posed pair; a mesh (type 7) reads the hull at mesh_verts, as in k_geom_sep_exact
__global__ __launch_bounds__(256) void k_geom_witness(long long M, const int32_t *__restrict__ types /*[M,2]*/, const double *__restrict__ recs /*[M,2,15]*/,
                                                      const double *__restrict__ mesh_verts /*[nvert,3] or null*/, int nvert, double band,
                                                      double *__restrict__ out /*[M,10]*/) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double o[10];
    geom_witness_rec(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, mesh_verts, nvert, band, o);
#pragma unroll
    for (int k = 0; k < 10; k++) out[i * 10 + k] = o[k];
}

static const LdsKernels kProximityWitnessLds({(const void *)k_proximity_witness<false>, (const void *)k_proximity_witness<true>});

extern "C" int mopa_proximity_witness_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env, double band,
                                            int32_t K, double *clearance, int32_t *count, int32_t *pair, double *dist, double *normal, double *p1, double *p2,
                                            void *stream) {
    if (!S || !normal || !p1 || !p2) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    // (argument rules, refusals and status codes: mopa_proximity_exact_batch's, all of them in front of its launch)
    const int rc = mopa_proximity_exact_batch(S, q_active, qpos_env, N, samples_per_env, band, K, clearance, count, pair, dist, stream);
    if (rc != MOPA_OK || N == 0) return rc;
    return contact_tail_launch(S, "proximity witness", S->hdr.has_mesh ? k_proximity_witness<true> : k_proximity_witness<false>, N, stream, q_active, qpos_env,
                               (long long)N, (long long)samples_per_env, band, (int)K, (const int32_t *)count, (const int32_t *)pair, normal, p1, p2);
}

extern "C" int mopa_proximity_witness_state(MopaScene *S, const double *qpos_host, double band, int32_t K, double *clearance, int32_t *count, int32_t *pair,
                                            double *dist, double *normal, double *p1, double *p2) {
    if (!S || !qpos_host || !clearance || !count || !pair || !dist || !normal || !p1 || !p2) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the proximity report (mopa_proximity_witness_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_pairs must be >= 1");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    Staging g;
    const auto f_dist = g.dbl(K), f_clear = g.dbl(1), f_normal = g.dbl(3 * (size_t)K), f_p1 = g.dbl(3 * (size_t)K), f_p2 = g.dbl(3 * (size_t)K);
    const auto f_pair = g.i32(K), f_count = g.i32(1);
    HIP_TRY(g.alloc());
    rc = mopa_proximity_witness_batch(S, S->d_q + S->nq, S->d_q, 1, 1, band, K, g.dev(f_clear), g.dev(f_count), g.dev(f_pair), g.dev(f_dist), g.dev(f_normal),
                                      g.dev(f_p1), g.dev(f_p2), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_dist, dist); g.out(f_clear, clearance); g.out(f_pair, pair); g.out(f_count, count);
    g.out(f_normal, normal); g.out(f_p1, p1); g.out(f_p2, p2);
    return MOPA_OK;
}

extern "C" int mopa_geom_witness_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band,
                                       double *out, void *stream) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr, mesh_verts, nvert)) return rc;
    if (const int rc = band_rule(band)) return rc;
    return pair_launch(device, k_geom_witness, M, stream, types, recs, mesh_verts, (int)nvert, band, out);
}

// The host compile of the same functions: the sequential form the kernels must match bit for bit.  No GPU, no HIP call.
// iters_out [M] (nullable): as mopa_geom_sep_exact_host's
extern "C" int mopa_geom_witness_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double band, double *out,
                                      int32_t *iters_out) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr, mesh_verts, nvert)) return rc;
    if (const int rc = band_rule(band)) return rc;
    for (int64_t i = 0; i < M; i++) {
        int it = 0;
        geom_witness_rec(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, mesh_verts, nvert, band, out + i * 10, &it);
        if (iters_out) iters_out[i] = it;
    }
    return MOPA_OK;
}
