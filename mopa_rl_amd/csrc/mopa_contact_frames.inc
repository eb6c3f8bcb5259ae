// mopa_contact_frames.inc -- contact frames of the batched contact report: for every record of mopa_contacts_batch the contact
// normal and point (mopa_frames.hpp: geom_frame), what the reference reads off d->contact[i].frame / pos (util/contact_info.py).
//
// A kernel of its own BEHIND k_contact_rows, reading the rows that one wrote: the report's two launches, their registers and
// their bytes are what they are without frames (DESIGN.md section 4, "Contact frames", has the resource table behind the
// choice: the MPR walk with its six extra vectors per portal vertex does not fit k_contact_rows' budget).  Mapping as there, a
// wave per state with a record: the wave poses the state (wave_load_state / wave_fk, the validity routine's), then the lanes
// that own a record with slot < K run geom_frame on their pair and store normal / pos; every other slot is written 0.0.  Each
// output word has exactly one writer: two runs write the same bytes.

template <bool MESH>
__global__ __launch_bounds__(kBlock) void k_contact_frames(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                           const int32_t *__restrict__ pair_slot /*[npair_model] model pair -> device pair or -1*/,
                                                           int npair_model, const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                           long long N, long long samples_per_env, int K, const int32_t *__restrict__ count /*[N]*/,
                                                           const int32_t *__restrict__ pair /*[N,K]*/, double *__restrict__ normal /*[N,K,3]*/,
                                                           double *__restrict__ pos /*[N,K,3]*/) {
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
            V3 n{0.0, 0.0, 0.0}, c{0.0, 0.0, 0.0};
            if (slot < nrec) {
                const int p = pair[s * K + slot];
                const int dp = (p >= 0 && p < npair_model) ? pair_slot[p] : -1;
                if (dp >= 0 && dp < h.npair) {
                    const int pk = I[h.o_pairs + dp];
                    const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
                    // (the scene's pairs are in the narrow phase's order already -- type1 <= type2, mopa_scene_create refuses any other --
                    //  so the normal points from pair_geom's first geom towards its second as it comes out)
                    (void)geom_frame<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], v.dbl, n, c);
                }
            }
            double *no = normal + (s * K + slot) * 3, *po = pos + (s * K + slot) * 3;
            no[0] = n.x; no[1] = n.y; no[2] = n.z;
            po[0] = c.x; po[1] = c.y; po[2] = c.z;
        }
        if (nrec > 0) wave_sync();   // the geom slab is about to be reused
    }
}

// pair level: one lane per posed primitive pair
__global__ __launch_bounds__(256) void k_geom_frames(long long M, const int32_t *__restrict__ types /*[M,2]*/, const double *__restrict__ recs /*[M,2,15]*/,
                                                     double *__restrict__ out /*[M,7]*/) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    geom_frame_pair<false>(types[2 * i], recs + i * 30, types[2 * i + 1], recs + i * 30 + 15, nullptr, out + i * 7);
}

static void contact_frames_register_lds() {
    for (const void *k : {(const void *)k_contact_frames<false>, (const void *)k_contact_frames<true>})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
}

extern "C" int mopa_contact_frames_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                         double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist, double *normal, double *pos, void *stream) {
    if (!S || !normal || !pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_frames_batch)");
    // (argument rules and status codes: mopa_contacts_batch's)
    const int rc = mopa_contacts_batch(S, q_active, qpos_env, N, samples_per_env, cutoff, K, count, pair, dist, stream);
    if (rc != MOPA_OK || N == 0) return rc;
    ON_DEVICE(S->device);
    if (S->lds_bytes > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "contact frames: the scene does not fit LDS");
    hipLaunchKernelGGL(S->hdr.has_mesh ? k_contact_frames<true> : k_contact_frames<false>, dim3(grid_for(S, N)), dim3(kBlock), S->lds_bytes, (hipStream_t)stream,
                       S->hdr, S->d_dbl, S->d_int, (const int32_t *)S->d_pair_slot, S->npair_model, q_active, qpos_env, (long long)N, (long long)samples_per_env,
                       (int)K, (const int32_t *)count, (const int32_t *)pair, normal, pos);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_contact_frames_state(MopaScene *S, const double *qpos_host, double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist,
                                         double *normal, double *pos) {
    if (!S || !qpos_host || !count || !pair || !dist || !normal || !pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_frames_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    void *buf = nullptr;
    const size_t nK = (size_t)K;
    const size_t off_dist = 0, off_normal = nK * sizeof(double), off_pos = off_normal + 3 * nK * sizeof(double), off_pair = off_pos + 3 * nK * sizeof(double),
                 off_count = off_pair + nK * sizeof(int32_t);
    HIP_TRY(hipMalloc(&buf, off_count + sizeof(int32_t)));
    unsigned char *b = static_cast<unsigned char *>(buf);
    rc = mopa_contact_frames_batch(S, S->d_q + S->nq, S->d_q, 1, 1, cutoff, K, reinterpret_cast<int32_t *>(b + off_count), reinterpret_cast<int32_t *>(b + off_pair),
                                   reinterpret_cast<double *>(b + off_dist), reinterpret_cast<double *>(b + off_normal), reinterpret_cast<double *>(b + off_pos), nullptr);
    hipError_t e = hipSuccess;
    if (rc == MOPA_OK) {
        e = hipMemcpy(dist, b + off_dist, nK * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(normal, b + off_normal, 3 * nK * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pos, b + off_pos, 3 * nK * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pair, b + off_pair, nK * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(count, b + off_count, sizeof(int32_t), hipMemcpyDeviceToHost);
    }
    (void)hipFree(buf);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(e);
    return MOPA_OK;
}

extern "C" int mopa_geom_frames_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, double *out, void *stream) {
    if (M < 0 || (M > 0 && (!types || !recs || !out))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
    if (device < 0 || device >= mopa_device_count()) return fail(MOPA_ERR_INVALID_ARG, "device ordinal out of range");
    if (M == 0) return MOPA_OK;
    ON_DEVICE(device);
    hipLaunchKernelGGL(k_geom_frames, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)M, types, recs, out);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// The host compile of the same functions: the sequential form the kernels must match bit for bit.  No GPU, no HIP call.
extern "C" int mopa_geom_frames_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double *out) {
    if (M < 0 || (M > 0 && (!types || !recs || !out)) || nvert < 0 || (nvert > 0 && !mesh_verts)) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
    for (int64_t i = 0; i < M; i++) {
        const int t1 = types[2 * i], t2 = types[2 * i + 1];
        const double *r1 = recs + i * 30, *r2 = r1 + 15;
        if (t2 == G_MESH && nvert > 0) {
            // a mesh as the second geom: its record's size slots are replaced by where the hull lives (offset 0 of mesh_verts, nvert vertices)
            double rm[15];
            std::memcpy(rm, r2, sizeof(rm));
            rm[GO_SIZE] = 0.0; rm[GO_SIZE + 1] = (double)nvert; rm[GO_SIZE + 2] = 0.0;
            geom_frame_pair<true>(t1, r1, t2, rm, mesh_verts, out + i * 7);
        } else {
            geom_frame_pair<false>(t1, r1, t2, r2, nullptr, out + i * 7);
        }
    }
    return MOPA_OK;
}
