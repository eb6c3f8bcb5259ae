// mopa_motion_report.inc -- K2, motion report: WHERE a segment is blocked, and by which pairs.
// (included by mopa_hip.hip after mopa_motion.inc and mopa_contacts.inc)
//
// OMPL's DiscreteMotionValidator::checkMotion(s1, s2, lastValid), restated over the pieces mopa_check_motion_batch is made of.
// Segment i, c = max(nd, 1) states s_k, k = 1 .. c: s_c = qb (its bits), s_k = interp_dim(a, qa[a], qb[a], (double)k / (double)c)
// for k < c -- the expressions of k_check_motion / k_motion_expand; qa is not tested.  Per segment:
//   valid         1 iff every s_k is valid (mopa_check_motion_batch's byte)
//   n_states      c
//   first_bad     the smallest k with s_k invalid, 0 for a valid segment
//   last_valid_t  1.0 if valid, else (double)(first_bad - 1) / (double)c
//   last_valid_q  qb if valid, qa's bits if first_bad == 1, else s_{first_bad - 1}: the values that were validated at that index
//   first_bad_q   s_{first_bad}; qb if valid
// Two forms behind check_motion's dispatch rule (mopa_scene_motion_kernel names the form of both calls):
//   small batches  k_motion_report, one wave per segment, k ASCENDING with a stop at the first invalid state.  k_check_motion tests the
//                  end state first, which is right for the verdict and useless for "first blocked": a segment whose end state alone
//                  is invalid costs c passes here and one there, which is why this is an entry point of its own.
//   large batches  the expanded-motion pipeline check_motion runs (mopa_motion.inc: motion_expand_chunk under motion_for_chunks) and
//                  launch_is_valid, then k_motion_report_reduce in place of k_motion_reduce and k_motion_report_rows.  k_motion_expand
//                  stores state k of a segment at slot o + (c - k), so first_bad = c - (largest j with vstate[o + j] == 0); both rows
//                  are copied out of the expanded state buffer: first_bad_q from slot j = c - first_bad, last_valid_q from slot j + 1
//                  (qa when first_bad == 1).  The pipeline's 31-bit chunking applies, and so does its one 4-byte read-back per
//                  chunk: this form synchronises the stream before it returns.
// Every output word has one writer and is a plain vector store; no atomics, so two runs write the same bytes.
// Blockers (max_contacts = K >= 1): mopa_contacts_batch over the rows first_bad_q at the scene's contact_threshold -- no narrow-phase
// code of its own.  A valid segment's first_bad_q is qb, a valid state, whose row is the "unused" pattern.

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_motion_report(
    SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int, const double *__restrict__ qa_all,
    const double *__restrict__ qb_all, const double *__restrict__ qpos_env, long long N, long long samples_per_env,
    unsigned char *__restrict__ valid, int32_t *__restrict__ n_states, int32_t *__restrict__ first_bad, double *__restrict__ last_valid_t,
    double *__restrict__ last_valid_q /*nullable*/, double *__restrict__ first_bad_q /*nullable*/, int hdr_lds_off, int prev_lds_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    // (the header copy in LDS: as in k_check_motion)
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double *tst = v.qbuf + h.na + h.n_pq;                                             // the state under test, [na]
    double *prev = reinterpret_cast<double *>(smem + prev_lds_off) + wave * h.na;     // the last state that passed, [na] per wave
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long s = (long long)blockIdx.x * kWavesPerBlock + wave; s < N; s += stride) {
        const double *qa = qa_all + s * h.na, *qb = qb_all + s * h.na;
        const double *row = qpos_env + (s / samples_per_env) * h.nq;
        const int nd = __builtin_amdgcn_readfirstlane(valid_segment_count(h, v, qa, qb));
        const int c = nd > 0 ? nd : 1;
        // each lane keeps its own entries of `prev` (lane a: entries a, a + 64, ...), so the copies below need no wave_sync
        for (int i = lane; i < h.na; i += 64) prev[i] = qa[i];
        int bad = 0;
        for (int k = 1; k <= c; k++) {          // one call site -> one copy of FK + collision
            const double t = (double)k / (double)c;
            for (int i = lane; i < h.na; i += 64) tst[i] = (k == c) ? qb[i] : interp_dim(h, v, i, qa[i], qb[i], t);
            wave_sync();
            const bool ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row);
            if (__builtin_amdgcn_readfirstlane((int)ok) == 0) { bad = k; break; }
            if (k < c)
                for (int i = lane; i < h.na; i += 64) prev[i] = tst[i];
        }
        // valid: tst holds s_c = qb, which is both rows
        for (int i = lane; i < h.na; i += 64) {
            const double x = tst[i];
            if (first_bad_q) first_bad_q[s * h.na + i] = x;
            if (last_valid_q) last_valid_q[s * h.na + i] = bad ? prev[i] : x;
        }
        if (lane == 0) {
            valid[s] = bad ? 0 : 1;
            n_states[s] = c;
            first_bad[s] = bad;
            last_valid_t[s] = bad ? (double)(bad - 1) / (double)c : 1.0;
        }
        wave_sync();      // tst is rewritten by the next segment
    }
}

// large batches: per segment the ordered reduction over its slots of the expanded verdicts
__global__ __launch_bounds__(256) void k_motion_report_reduce(const int *__restrict__ cnt, const int *__restrict__ off, const int *__restrict__ bsum,
                                                              const unsigned char *__restrict__ vstate, long long N,
                                                              unsigned char *__restrict__ valid, int32_t *__restrict__ n_states,
                                                              int32_t *__restrict__ first_bad, double *__restrict__ last_valid_t) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = cnt[i], o = motion_slot0(off, bsum, i);
    int jmax = -1;                                  // state k sits at slot c - k: the first bad k is the LAST bad slot
    for (int j = 0; j < c; j++)
        if (!vstate[o + j]) jmax = j;
    const int bad = jmax < 0 ? 0 : c - jmax;
    valid[i] = bad ? 0 : 1;
    n_states[i] = c;
    first_bad[i] = bad;
    last_valid_t[i] = bad ? (double)(bad - 1) / (double)c : 1.0;
}

// ... and its two rows, one lane per output double, copied out of the expanded state buffer (first_bad: what the kernel above wrote)
__global__ __launch_bounds__(256) void k_motion_report_rows(int na, const int *__restrict__ cnt, const int *__restrict__ off,
                                                            const int *__restrict__ bsum, const int32_t *__restrict__ first_bad,
                                                            const double *__restrict__ q_states, const double *__restrict__ qa, long long N,
                                                            double *__restrict__ last_valid_q /*nullable*/, double *__restrict__ first_bad_q /*nullable*/) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * na) return;
    const long long i = e / na;
    const int a = (int)(e - i * na);
    const int c = cnt[i], bad = first_bad[i];
    const size_t o = (size_t)motion_slot0(off, bsum, i);
    const int j = bad ? c - bad : 0;                // slot 0 holds s_c = qb
    if (first_bad_q) first_bad_q[e] = q_states[(o + j) * na + a];
    if (last_valid_q) last_valid_q[e] = (bad == 0) ? q_states[o * na + a] : (bad == 1) ? qa[e] : q_states[(o + j + 1) * na + a];
}

// large batches: the expanded-motion pipeline (mopa_motion.inc) and launch_is_valid, then the ordered reduction and the rows
static int motion_report_expanded(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                  uint8_t *valid, int32_t *n_states, int32_t *first_bad, double *last_valid_t, double *last_valid_q,
                                  double *first_bad_q, hipStream_t st) {
    StreamScratch &sc = scratch_for(S, st);
    const size_t na = (size_t)S->na;
    return motion_for_chunks(S, N, [&](int64_t first, int64_t n) {
        MotionExpanded x;
        int rc = motion_expand_chunk(S, sc, "motion report", qa + first * na, qb + first * na, n, samples_per_env, first, st, x);
        if (rc != MOPA_OK) return rc;
        rc = launch_is_valid(S, x.q, qpos_env, x.T, 1, x.env, sc.mv_valid.as<uint8_t>(), nullptr, st);
        if (rc != MOPA_OK) return rc;
        hipLaunchKernelGGL(k_motion_report_reduce, dim3(x.nb), dim3(256), 0, st, x.cnt, x.off, x.bsum, sc.mv_valid.as<uint8_t>(), (long long)n,
                           valid + first, n_states + first, first_bad + first, last_valid_t + first);
        if (last_valid_q || first_bad_q) {
            const unsigned nbr = (unsigned)((n * S->na + 255) / 256);
            hipLaunchKernelGGL(k_motion_report_rows, dim3(nbr), dim3(256), 0, st, S->na, x.cnt, x.off, x.bsum, first_bad + first, x.q, qa + first * na,
                               (long long)n, last_valid_q ? last_valid_q + first * na : nullptr, first_bad_q ? first_bad_q + first * na : nullptr);
        }
        HIP_TRY(hipGetLastError());
        return (int)MOPA_OK;
    });
}

static const LdsKernels kMotionReportLds({(const void *)k_motion_report});

extern "C" int mopa_motion_report_batch(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                        uint8_t *valid, int32_t *n_states, int32_t *first_bad, double *last_valid_t, double *last_valid_q,
                                        double *first_bad_q, int32_t K, int32_t *block_count, int32_t *block_pair, double *block_dist, void *stream) {
    if (!S) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (N > 0 && (!qa || !qb || !qpos_env || !valid || !n_states || !first_bad || !last_valid_t)) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    const bool blockers = K != 0 || block_count || block_pair || block_dist;
    if (blockers && K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1 (0 with null blocker buffers: no blockers)");
    if (blockers && N > 0 && (!block_count || !block_pair || !block_dist)) return fail(MOPA_ERR_INVALID_ARG, "null blocker buffer with max_contacts >= 1");
    MOPA_REFUSE_GLUED(S, "the motion report (mopa_motion_report_batch)");
    // (mopa_contacts_batch's cutoff rule, ahead of the first launch)
    if (blockers && !(std::isfinite(S->hdr.thr) && S->hdr.thr < 0.0))
        return fail(MOPA_ERR_INVALID_ARG, "blockers: cutoff = contact_threshold must be finite and < 0 (the broad phase culls at zero margin)");
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    if (blockers && !first_bad_q) {     // the rows the contact report reads, in library scratch
        StreamScratch &sc = scratch_for(S, st);
        HIP_TRY(grow(S, sc.mr_fbq, sizeof(double) * (size_t)N * (size_t)S->na));
        first_bad_q = sc.mr_fbq.as<double>();
    }
    if (S->k1.use_v2 && N >= k1_motion_expand_min(S)) {
        const int rc = motion_report_expanded(S, qa, qb, qpos_env, N, samples_per_env, valid, n_states, first_bad, last_valid_t, last_valid_q, first_bad_q, st);
        if (rc != MOPA_OK) return rc;
    } else {
        dim3 grid(grid_for(S, N)), block(kBlock);
        const int hdr_off = (S->lds_bytes + 15) & ~15;
        const int prev_off = (hdr_off + (int)sizeof(SceneHdr) + 15) & ~15;
        const int lds = prev_off + kWavesPerBlock * S->na * (int)sizeof(double);
        if (lds > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "motion report LDS does not fit");
        hipLaunchKernelGGL(k_motion_report, grid, block, lds, st, S->hdr, S->d_dbl, S->d_int, qa, qb, qpos_env, (long long)N, (long long)samples_per_env,
                           valid, n_states, first_bad, last_valid_t, last_valid_q, first_bad_q, hdr_off, prev_off);
        HIP_TRY(hipGetLastError());
    }
    if (!blockers) return MOPA_OK;
    return mopa_contacts_batch(S, first_bad_q, qpos_env, N, samples_per_env, S->hdr.thr, K, block_count, block_pair, block_dist, stream);
}

// one segment, host pointers, synchronous: the active entries of qpos_a -> those of qpos_b, the passive entries from qpos_a
extern "C" int mopa_motion_report(MopaScene *S, const double *qpos_a, const double *qpos_b, int32_t *valid_out, int32_t *n_states_out,
                                  int32_t *first_bad_out, double *last_valid_t_out, double *last_valid_q_out, double *first_bad_q_out, int32_t K,
                                  int32_t *block_count, int32_t *block_pair, double *block_dist) {
    if (!S || !qpos_a || !qpos_b || !valid_out || !n_states_out || !first_bad_out || !last_valid_t_out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const bool blockers = K != 0 || block_count || block_pair || block_dist;
    if (blockers && K < 1) return fail(MOPA_ERR_INVALID_ARG, "max_contacts must be >= 1 (0 with null blocker buffers: no blockers)");
    if (blockers && (!block_count || !block_pair || !block_dist)) return fail(MOPA_ERR_INVALID_ARG, "null blocker buffer with max_contacts >= 1");
    MOPA_REFUSE_GLUED(S, "the motion report (mopa_motion_report)");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_a);       // S->d_q: the env row, then a's active entries
    if (rc) return rc;
    const size_t na = (size_t)S->na, Kb = blockers ? (size_t)K : 0;
    Staging g;
    const auto f_qb = g.dbl(na), f_lvq = g.dbl(na), f_fbq = g.dbl(na), f_t = g.dbl(1), f_dist = g.dbl(Kb);
    const auto f_n = g.i32(1), f_bad = g.i32(1), f_count = g.i32(1), f_pair = g.i32(Kb);
    const auto f_valid = g.u8(1);
    HIP_TRY(g.alloc());
    HIP_TRY(g.seed(f_qb, active_of(S, qpos_b).data()));
    rc = mopa_motion_report_batch(S, S->d_q + S->nq, g.dev(f_qb), S->d_q, 1, 1, g.dev(f_valid), g.dev(f_n), g.dev(f_bad), g.dev(f_t), g.dev(f_lvq), g.dev(f_fbq), K,
                                  blockers ? g.dev(f_count) : nullptr, blockers ? g.dev(f_pair) : nullptr, blockers ? g.dev(f_dist) : nullptr, nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    *valid_out = *g.host(f_valid);
    g.out(f_n, n_states_out); g.out(f_bad, first_bad_out); g.out(f_t, last_valid_t_out);
    g.out(f_lvq, last_valid_q_out); g.out(f_fbq, first_bad_q_out);
    if (blockers) {
        g.out(f_count, block_count); g.out(f_pair, block_pair); g.out(f_dist, block_dist);
    }
    return MOPA_OK;
}
