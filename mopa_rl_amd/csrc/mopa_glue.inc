// mopa_glue.inc -- glue_bodies: the manipulated object attached to the gripper (included by mopa_hip.hip behind mopa_scene_create).
//
// A glued scene (mopa_scene_create_glued(desc, body_a, body_b)) poses body_b -- a body with one free joint -- as a jointless child of
// body_a, a body the active joints move.  Its local pose under body_a, the OFFSET (t, rq), is not a scene constant: it is read from the 7
// free-joint slots of the state (J_GLUE in the FK walks).  A row whose free-joint slots hold the offset is an ATTACHED ROW; k_glue_attach
// makes one out of an ordinary qpos row, and every entry point that serves a glued scene runs it over the caller's rows first (the
// reference: GlueTransformation, motion_planners/src/mujoco_ompl_interface.cpp:810-907, installed by KinematicPlanner::plan /
// isValidState).  k_glue_rows writes the carried body's world pose into the free-joint columns of solved path rows
// (KinematicPlanner.cpp:207-240 fills them from d->qpos after the glued isValid).
//
// This is the WELD form of the reference's write-back form (which writes the world pose into the free joint's qpos and runs FK a
// second time): the same pose up to rounding; on the CPU oracle equal verdicts on every state compared, min_dist equal on all but 0.2 % of them
// (DESIGN.md section 3).

// World pose of moving body `mb` for one state: the walk of fk_one_geom down the body's chain over the same pieces (mopa_fk.hpp), with the
// same arithmetic in the same order (sin / cos of half a hinge angle through apply_joint = mopa_sincos(0.5 * dq), what the sin/cos tables hold).  Value slot s of the
// state is act_row[act_adr[s]] for s < na, else pas_row[pq_adr[s - na]] (both full qpos rows).  Only body_a's chain is walked, and
// body_b is never on it (body_a below body_b is refused by the scene compiler), so there is no J_GLUE step here.
MOPA_D void glue_walk(const SceneHdr &h, const double *D, const int *I, int mb, const double *act_row, const double *pas_row, V3 &pos, Q4 &quat,
                      double *mat) {
    auto slot_ptr = [&](int s) -> const double * { return s < h.na ? act_row + I[h.o_act_adr + s] : pas_row + I[h.o_pq_adr + (s - h.na)]; };
    const int cadr = I[h.o_chain_adr + mb], clen = I[h.o_chain_len + mb];
    pos = V3{0.0, 0.0, 0.0};
    quat = Q4{1.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < clen; k++) {
        const int body = I[h.o_chain_items + cadr + k];
        const int *r = I + h.o_mbr + 8 * body;
        const int jn = r[0], ja = r[1], w7 = r[7];
        const double *bd = D + h.o_mbd + 16 * body;
        const int jt0 = w7 & 0x7f, qsrc0 = w7 >> 8;
        if (jn == 1 && jt0 == J_FREE) {
            const double *qp = slot_ptr(qsrc0);        // (7 contiguous passive slots: checked by the scene compiler)
            fk_free_step(qp, pos, quat);
        } else {
            V3 ppos;
            Q4 pquat;
            if (k == 0) {
                const int sf = r[3];
                sf_frame_ld(h, D, sf, ppos, pquat, mat);
            } else {
                ppos = pos;
                pquat = quat;
            }
            pos = add3(ppos, mat_vec(mat, ld3(bd)));
            quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
            if (jn > 0) apply_joint(jt0, ld3(bd + 7), ld3(bd + 10), (w7 & 0x80) != 0, *slot_ptr(qsrc0) - bd[13], pos, quat);
            for (int j = ja + 1; j < ja + jn; j++) {
                const V3 ax = ld3(D + h.o_mj_axis + 3 * j), jp = ld3(D + h.o_mj_pos + 3 * j);
                apply_joint(I[h.o_mj_type + j], ax, jp, is_zero3(jp), *slot_ptr(I[h.o_mj_qsrc + j]) - D[h.o_mj_ref + j], pos, quat);
            }
            quat = quat_normalize(quat);
        }
        quat2mat(mat, quat);
    }
}

// rows_in [E][nq] -> rows_out [E][nq]: a copy of the row whose 7 free-joint slots (qpos address adr) hold the offset (t, rq) of body_b
// under body_a at the row's own joint values.  One lane per row.  With (p_a, q_a, M_a = quat2mat(q_a)) from glue_walk and
// p_b = row[adr..adr+2], q_b = quat_normalize(row[adr+3..adr+6]) -- the pose FK gives a free body --
//     d  = sub3(p_b, p_a)                                   d.x = p_b.x - p_a.x, ...
//     t  = matT_vec(M_a, d)                                 t.x = fma(M[6], d.z, fma(M[3], d.y, M[0] * d.x)), t.y: M[7], M[4], M[1]; t.z: M[8], M[5], M[2]
//     rq = quat_mul(Q4{q_a.w, -q_a.x, -q_a.y, -q_a.z}, q_b) (quat_mul's own fma order, mopa_device.hpp); not normalised
// (the reference's body_b_a_trans_g and body_b_a_rot).  tests/glue_ref.py restates exactly this.
// STAGE: the scene blobs are staged in LDS as the other kernels do; scenes whose blobs exceed the 64 KiB a launch gets without a
// function attribute (none of this project's: 14-24 KiB) are read from global memory instead.
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_glue_attach(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int, int mb_a, int adr,
                                                        const double *__restrict__ rows_in, double *__restrict__ rows_out, long long E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const double *s_dbl = g_dbl;
    const int *s_int = g_int;
    if (STAGE) {
        double *l_dbl = reinterpret_cast<double *>(smem);
        int *l_int = reinterpret_cast<int *>(l_dbl + h.n_dbl);
        stage_scene(h, g_dbl, g_int, l_dbl, l_int);
        s_dbl = l_dbl;
        s_int = l_int;
    }
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double *row = rows_in + e * h.nq;
    double *out = rows_out + e * h.nq;
    V3 pa;
    Q4 qa;
    double mat[9];
    glue_walk(h, s_dbl, s_int, mb_a, row, row, pa, qa, mat);
    const V3 pb = ld3(row + adr);
    const Q4 qb = quat_normalize(Q4{row[adr + 3], row[adr + 4], row[adr + 5], row[adr + 6]});
    const V3 t = matT_vec(mat, sub3(pb, pa));
    const Q4 rq = quat_mul(Q4{qa.w, -qa.x, -qa.y, -qa.z}, qb);
    for (int i = 0; i < h.nq; i++) out[i] = row[i];
    out[adr] = t.x; out[adr + 1] = t.y; out[adr + 2] = t.z;
    out[adr + 3] = rq.w; out[adr + 4] = rq.x; out[adr + 5] = rq.y; out[adr + 6] = rq.z;
}

// path [E][max_path][nq], in place: in every row r < path_len[e] the 7 free-joint columns get body_b's world pose at that waypoint,
//     p_b' = add3(p_a', mat_vec(M_a', t)),   q_b' = quat_normalize(quat_mul(q_a', rq))
// -- the jointless-body step of the FK walks, so equal bit for bit to what they pose body_b at -- with (p_a', q_a') from the row's
// active columns and the attached row's passive ones, (t, rq) from the attached row of env e.  One lane per (env, row).
template <bool STAGE>
__global__ __launch_bounds__(kBlock) void k_glue_rows(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int, int mb_a, int adr,
                                                      double *__restrict__ path, const int32_t *__restrict__ path_len, const double *__restrict__ attached,
                                                      long long E, int max_path) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const double *s_dbl = g_dbl;
    const int *s_int = g_int;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long e = idx / max_path;
    const int r = (int)(idx - e * max_path);
    bool live = e < E;
    if (live) live = r < (path_len[e] < max_path ? path_len[e] : max_path);
    if (!__syncthreads_or((int)live)) return;       // (most workgroups lie past their paths' ends: they leave before staging the scene)
    if (STAGE) {
        double *l_dbl = reinterpret_cast<double *>(smem);
        int *l_int = reinterpret_cast<int *>(l_dbl + h.n_dbl);
        stage_scene(h, g_dbl, g_int, l_dbl, l_int);
        s_dbl = l_dbl;
        s_int = l_int;
    }
    if (!live) return;
    double *row = path + (e * max_path + r) * h.nq;
    const double *att = attached + e * h.nq;
    V3 pa;
    Q4 qa;
    double mat[9];
    glue_walk(h, s_dbl, s_int, mb_a, row, att, pa, qa, mat);
    const V3 pb = add3(pa, mat_vec(mat, ld3(att + adr)));
    const Q4 qb = quat_normalize(quat_mul(qa, Q4{att[adr + 3], att[adr + 4], att[adr + 5], att[adr + 6]}));
    row[adr] = pb.x; row[adr + 1] = pb.y; row[adr + 2] = pb.z;
    row[adr + 3] = qb.w; row[adr + 4] = qb.x; row[adr + 5] = qb.y; row[adr + 6] = qb.z;
}

// LDS of a launch: the staged blobs, or 0 = not staged (beyond what a launch gets without a function attribute)
static int glue_lds_bytes(const MopaScene *S) {
    const int bytes = S->hdr.n_dbl * 8 + ((S->hdr.n_int + 1) & ~1) * 4;
    return bytes <= 64 * 1024 ? bytes : 0;
}

// what an entry point that does not serve glued scenes returns on one (never a silent unglued run)
#define MOPA_REFUSE_GLUED(S_, what_) \
    do { if ((S_)->glue_b >= 0) return fail(MOPA_ERR_UNSUPPORTED, std::string(what_) + " is not built for a glued scene (glue_bodies)"); } while (0)

static int glue_attach_launch(MopaScene *S, const double *rows, int64_t E, double *out, hipStream_t st) {
    const unsigned grid = (unsigned)((E + kBlock - 1) / kBlock);
    const int lds = glue_lds_bytes(S);
    hipLaunchKernelGGL(lds ? k_glue_attach<true> : k_glue_attach<false>, dim3(grid), dim3(kBlock), lds, st, S->hdr, S->d_dbl, S->d_int, S->glue_mb_a, S->glue_adr, rows, out,
                       (long long)E);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
// the attached rows of a call's E env rows, in the stream's scratch (valid until the next call on the stream that asks for them)
static int glue_attach_scratch(MopaScene *S, const double *rows, int64_t E, hipStream_t st, const double **out) {
    StreamScratch &sc = scratch_for(S, st);
    HIP_TRY(grow(S, sc.glue_rows, (size_t)E * (size_t)S->nq * sizeof(double)));
    *out = sc.glue_rows.as<double>();
    return glue_attach_launch(S, rows, E, sc.glue_rows.as<double>(), st);
}

extern "C" int mopa_scene_glue(const MopaScene *S, int32_t out[2]) {
    if (!S || !out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    out[0] = S->glue_a; out[1] = S->glue_b;
    return MOPA_OK;
}

extern "C" int mopa_glue_attach_batch(MopaScene *S, const double *rows_dev, int64_t E, double *attached_dev, void *stream) {
    if (!S || (E > 0 && (!rows_dev || !attached_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (S->glue_b < 0) return fail(MOPA_ERR_INVALID_ARG, "not a glued scene (mopa_scene_create_glued)");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "E < 0");
    if (E == 0) return MOPA_OK;
    if (rows_dev == attached_dev) return fail(MOPA_ERR_INVALID_ARG, "attach is not done in place");
    ON_DEVICE(S->device);
    return glue_attach_launch(S, rows_dev, E, attached_dev, (hipStream_t)stream);
}

extern "C" int mopa_glue_rows_batch(MopaScene *S, double *path_dev, const int32_t *path_len_dev, const double *attached_dev, int64_t E, int32_t max_path,
                                    void *stream) {
    if (!S || (E > 0 && (!path_dev || !path_len_dev || !attached_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (S->glue_b < 0) return fail(MOPA_ERR_INVALID_ARG, "not a glued scene (mopa_scene_create_glued)");
    if (E < 0 || max_path < 1) return fail(MOPA_ERR_INVALID_ARG, "E < 0 or max_path < 1");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    const long long n = (long long)E * max_path;
    if ((n + kBlock - 1) / kBlock > 0x7fffffffll) return fail(MOPA_ERR_LIMIT, "E * max_path too large for one launch");
    const int lds = glue_lds_bytes(S);
    hipLaunchKernelGGL(lds ? k_glue_rows<true> : k_glue_rows<false>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), lds, (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int,
                       S->glue_mb_a, S->glue_adr, path_dev, path_len_dev, attached_dev, (long long)E, (int)max_path);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
