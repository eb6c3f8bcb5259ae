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

static const LdsKernels kContactFramesLds({(const void *)k_contact_frames<false>, (const void *)k_contact_frames<true>});

// The launch of a kernel behind k_contact_rows (k_contact_frames, k_contact_manifolds): a wave per state, the scene's own LDS;
// `args`: the kernel's arguments from q_active on.
template <class Kern, class... Args>
static int contact_tail_launch(MopaScene *S, const char *what, Kern kern, int64_t N, void *stream, Args... args) {
    ON_DEVICE(S->device);
    if (S->lds_bytes > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, std::string(what) + ": the scene does not fit LDS");
    hipLaunchKernelGGL(kern, dim3(grid_for(S, N)), dim3(kBlock), S->lds_bytes, (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, (const int32_t *)S->d_pair_slot,
                       S->npair_model, args...);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// The pair-level entry points (mopa_geom_{frames,sep,manifolds}_{batch,host}): M posed pairs as types [M,2] and recs [M,2,15], `outs_ok`:
// every output buffer is there; a hull as nvert vertices at mesh_verts (none: 0, null).
static int pair_batch_rule(int64_t M, const int32_t *types, const double *recs, bool outs_ok, const double *mesh_verts = nullptr, int32_t nvert = 0) {
    if (M < 0 || (M > 0 && (!types || !recs || !outs_ok)) || nvert < 0 || (nvert > 0 && !mesh_verts)) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
    return MOPA_OK;
}
// ... the device rule of a _batch form and its launch: one lane per pair, 256 lanes per workgroup; `args`: the kernel's arguments behind M
template <class Kern, class... Args>
static int pair_launch(int32_t device, Kern kern, int64_t M, void *stream, Args... args) {
    if (device < 0 || device >= mopa_device_count()) return fail(MOPA_ERR_INVALID_ARG, "device ordinal out of range");
    if (M == 0) return MOPA_OK;
    ON_DEVICE(device);
    hipLaunchKernelGGL(kern, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)M, args...);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
// ... and in the _host forms a mesh as the second geom: rm = its record r2 with the size slots replaced by where the hull lives
// (offset 0 of mesh_verts, nvert vertices)
static void pair_mesh_rec(const double *r2, int32_t nvert, double *rm /*[15]*/) {
    std::memcpy(rm, r2, 15 * sizeof(double));
    rm[GO_SIZE] = 0.0; rm[GO_SIZE + 1] = (double)nvert; rm[GO_SIZE + 2] = 0.0;
}

extern "C" int mopa_contact_frames_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                         double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist, double *normal, double *pos, void *stream) {
    if (!S || !normal || !pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_frames_batch)");
    // (argument rules and status codes: mopa_contacts_batch's)
    const int rc = mopa_contacts_batch(S, q_active, qpos_env, N, samples_per_env, cutoff, K, count, pair, dist, stream);
    if (rc != MOPA_OK || N == 0) return rc;
    return contact_tail_launch(S, "contact frames", S->hdr.has_mesh ? k_contact_frames<true> : k_contact_frames<false>, N, stream, q_active, qpos_env, (long long)N,
                               (long long)samples_per_env, (int)K, (const int32_t *)count, (const int32_t *)pair, normal, pos);
}

extern "C" int mopa_contact_frames_state(MopaScene *S, const double *qpos_host, double cutoff, int32_t K, int32_t *count, int32_t *pair, double *dist,
                                         double *normal, double *pos) {
    if (!S || !qpos_host || !count || !pair || !dist || !normal || !pos) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the contact report (mopa_contact_frames_state)");
    if (K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    Staging g;
    const auto f_dist = g.dbl(K), f_normal = g.dbl(3 * (size_t)K), f_pos = g.dbl(3 * (size_t)K);
    const auto f_pair = g.i32(K), f_count = g.i32(1);
    HIP_TRY(g.alloc());
    rc = mopa_contact_frames_batch(S, S->d_q + S->nq, S->d_q, 1, 1, cutoff, K, g.dev(f_count), g.dev(f_pair), g.dev(f_dist), g.dev(f_normal), g.dev(f_pos), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_dist, dist); g.out(f_normal, normal); g.out(f_pos, pos); g.out(f_pair, pair); g.out(f_count, count);
    return MOPA_OK;
}

extern "C" int mopa_geom_frames_batch(int32_t device, int64_t M, const int32_t *types, const double *recs, double *out, void *stream) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr)) return rc;
    return pair_launch(device, k_geom_frames, M, stream, types, recs, out);
}

// The host compile of the same functions: the sequential form the kernels must match bit for bit.  No GPU, no HIP call.
extern "C" int mopa_geom_frames_host(int64_t M, const int32_t *types, const double *recs, const double *mesh_verts, int32_t nvert, double *out) {
    if (const int rc = pair_batch_rule(M, types, recs, out != nullptr, mesh_verts, nvert)) return rc;
    for (int64_t i = 0; i < M; i++) {
        const int t1 = types[2 * i], t2 = types[2 * i + 1];
        const double *r1 = recs + i * 30, *r2 = r1 + 15;
        if (t2 == G_MESH && nvert > 0) {
            double rm[15];
            pair_mesh_rec(r2, nvert, rm);
            geom_frame_pair<true>(t1, r1, t2, rm, mesh_verts, out + i * 7);
        } else {
            geom_frame_pair<false>(t1, r1, t2, r2, nullptr, out + i * 7);
        }
    }
    return MOPA_OK;
}
