// mopa_contact_manifold.inc -- contact manifolds of the batched contact report: for every record of mopa_contacts_batch the frame's
// normal and up to P contact points (mopa_manifold.hpp: geom_manifold), what the reference reads off d->contact[i].pos / frame /
// dist per CONTACT where MuJoCo emits several for a pair (util/contact_info.py).  [3P] restated, PARITY UNPINNED.
//
// A kernel of its own BEHIND k_contact_rows, reading the rows that one wrote, as k_contact_frames does: with manifolds off not one
// launch, byte or register of the report or of the frames changes.  Mapping as there -- a wave per state with a record poses the
// state (wave_load_state / wave_fk), then ONE LANE PER RECORD runs geom_manifold on its pair.  A state has few records (K = 16 is
// the usual cap) and most of them are single-point classes, so a lane group per record would idle as many lanes as it frees; the
// clip tables of the box-box rule live in scratch (DESIGN.md section 4, "Contact manifolds", has the resource table).  Every word
// of normal / npoint / point_dist / point_pos has exactly one writer and is written by a plain store, unused slots and states
// without a record included: two runs write the same bytes.

template <bool MESH>
__global__ __launch_bounds__(kBlock) void k_contact_manifolds(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                              const int32_t *__restrict__ pair_slot /*[npair_model] model pair -> device pair or -1*/,
                                                              int npair_model, const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                              long long N, long long samples_per_env, int K, int P, double point_cutoff,
                                                              const int32_t *__restrict__ count /*[N]*/, const int32_t *__restrict__ pair /*[N,K]*/,
                                                              double *__restrict__ normal /*[N,K,3]*/, int32_t *__restrict__ npoint /*[N,K]*/,
                                                              double *__restrict__ point_dist /*[N,K,P]*/, double *__restrict__ point_pos /*[N,K,P,3]*/) {
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
            V3 n{0.0, 0.0, 0.0};
            int np = 0;
            double pd[kManifoldMax], pp[3 * kManifoldMax];
            bool have = false;
            if (slot < nrec) {
                const int p = pair[s * K + slot];
                const int dp = (p >= 0 && p < npair_model) ? pair_slot[p] : -1;
                if (dp >= 0 && dp < h.npair) {
                    const int pk = I[h.o_pairs + dp];
                    const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
                    // (the scene's pairs are in the narrow phase's order already, as in k_contact_frames)
                    (void)geom_manifold<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl, point_cutoff, P, n, np, pd,
                                              pp);
                    have = true;
                }
            }
            const long long rec = s * K + slot;
            double *no = normal + rec * 3, *dd = point_dist + rec * P, *po = point_pos + rec * P * 3;
            no[0] = n.x; no[1] = n.y; no[2] = n.z;
            npoint[rec] = np;
            for (int i = 0; i < P; i++) {
                dd[i] = have ? pd[i] : kFar;
                po[3 * i] = have ? pp[3 * i] : 0.0;
                po[3 * i + 1] = have ? pp[3 * i + 1] : 0.0;
                po[3 * i + 2] = have ? pp[3 * i + 2] : 0.0;
            }
        }
        if (nrec > 0) wave_sync();   // the geom slab is about to be reused
    }
}

// pair level: one lane per posed primitive pair
__global__ __launch_bounds__(256) void k_geom_manifolds(long long M, const int32_t *__restrict__ types /*[M,2]*/, const double *__restrict__ recs /*[M,2,15]*/,
                                                        double point_cutoff, int P, double *__restrict__ normal_dist /*[M,4]*/, int32_t *__restrict__ npoint /*[M]*/,
                                                        double *__restrict__ points /*[M,P,4]*/) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    int np;
    geom_manifold_pair<false>(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, nullptr, point_cutoff, P, normal_dist + i * 4, &np, points + i * P * 4);
    npoint[i] = np;
}

static const LdsKernels kContactManifoldsLds({(const void *)k_contact_manifolds<false>, (const void *)k_contact_manifolds<true>});

static int manifold_args_ok(int32_t P, double point_cutoff) {
    if (P < 1 || P > kManifoldMax) return fail(MOPA_ERR_INVALID_ARG, "max_points must be 1 .. 8");
    if (!std::isfinite(point_cutoff)) return fail(MOPA_ERR_INVALID_ARG, "point_cutoff must be finite");
    return MOPA_OK;
}

extern "C" int mopa_contact_manifolds_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env, double cutoff,
                                            double point_cutoff, int32_t K, int32_t P, int32_t *count, int32_t *pair, double *dist, double *normal, int32_t *npoint,
                                            double *point_dist, double *point_pos, void *stream) {
    if (!S || !normal || !npoint || !point_dist || !point_pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_manifolds_batch)");
    int rc = manifold_args_ok(P, point_cutoff);
    if (rc != MOPA_OK) return rc;
    if (!(point_cutoff >= cutoff)) return fail(MOPA_ERR_INVALID_ARG, "point_cutoff must be >= cutoff (the deepest point of a reported pair lies at or below cutoff)");
    // (argument rules and status codes: mopa_contacts_batch's)
    rc = mopa_contacts_batch(S, q_active, qpos_env, N, samples_per_env, cutoff, K, count, pair, dist, stream);
    if (rc != MOPA_OK || N == 0) return rc;
    return contact_tail_launch(S, "contact manifolds", S->hdr.has_mesh ? k_contact_manifolds<true> : k_contact_manifolds<false>, N, stream, q_active, qpos_env,
                               (long long)N, (long long)samples_per_env, (int)K, (int)P, point_cutoff, (const int32_t *)count, (const int32_t *)pair, normal, npoint,
                               point_dist, point_pos);
}

extern "C" int mopa_contact_manifolds_state(MopaScene *S, const double *qpos_host, double cutoff, double point_cutoff, int32_t K, int32_t P, int32_t *count,
                                            int32_t *pair, double *dist, double *normal, int32_t *npoint, double *point_dist, double *point_pos) {
    if (!S || !qpos_host || !count || !pair || !dist || !normal || !npoint || !point_dist || !point_pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_manifolds_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1");
    int rc = manifold_args_ok(P, point_cutoff);
    if (rc != MOPA_OK) return rc;
    ON_DEVICE(S->device);
    rc = upload_state(S, qpos_host);
    if (rc) return rc;
    const size_t nK = (size_t)K, nP = (size_t)P;
    Staging g;
    const auto f_dist = g.dbl(nK), f_normal = g.dbl(3 * nK), f_pd = g.dbl(nK * nP), f_pp = g.dbl(3 * nK * nP);
    const auto f_pair = g.i32(nK), f_np = g.i32(nK), f_count = g.i32(1);
    HIP_TRY(g.alloc());
    rc = mopa_contact_manifolds_batch(S, S->d_q + S->nq, S->d_q, 1, 1, cutoff, point_cutoff, K, P, g.dev(f_count), g.dev(f_pair), g.dev(f_dist), g.dev(f_normal),
                                      g.dev(f_np), g.dev(f_pd), g.dev(f_pp), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_dist, dist); g.out(f_normal, normal); g.out(f_pd, point_dist); g.out(f_pp, point_pos);
    g.out(f_pair, pair); g.out(f_np, npoint); g.out(f_count, count);
    return MOPA_OK;
}

extern "C" int mopa_geom_manifolds_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, double point_cutoff, int32_t P, double *normal_dist,
                                         int32_t *npoint, double *points, void *stream) {
    if (const int rc = pair_batch_rule(M, types, recs, normal_dist && npoint && points)) return rc;
    if (const int rc = manifold_args_ok(P, point_cutoff)) return rc;
    return pair_launch(device, k_geom_manifolds, M, stream, types, recs, point_cutoff, (int)P, normal_dist, npoint, points);
}

// The host compile of the same functions: the sequential form the kernels must match bit for bit.  No GPU, no HIP call.
extern "C" int mopa_geom_manifolds_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double point_cutoff, int32_t P,
                                        double *normal_dist, int32_t *npoint, double *points) {
    if (const int rc = pair_batch_rule(M, types, recs, normal_dist && npoint && points, mesh_verts, nvert)) return rc;
    if (const int rc = manifold_args_ok(P, point_cutoff)) return rc;
    for (int64_t i = 0; i < M; i++) {
        const int t1 = types[2 * i], t2 = types[2 * i + 1];
        const double *r1 = recs + i * 30, *r2 = r1 + 15;
        int np = 0;
        if (t2 == G_MESH && nvert > 0) {
            // a mesh as the second geom: its record's size slots are replaced by where the hull lives, as in mopa_geom_frames_host
            double rm[15];
            pair_mesh_rec(r2, nvert, rm);
            geom_manifold_pair<true>(t1, r1, t2, rm, mesh_verts, point_cutoff, P, normal_dist + i * 4, &np, points + i * P * 4);
        } else {
            geom_manifold_pair<false>(t1, r1, t2, r2, nullptr, point_cutoff, P, normal_dist + i * 4, &np, points + i * P * 4);
        }
        npoint[i] = np;
    }
    return MOPA_OK;
}
