// mopa_motion_clearance.inc -- K2, clearance report: HOW NEAR a motion comes to collision, where along it, and to which pair.
// (included by mopa_hip.hip after mopa_motion_report.inc and mopa_proximity.inc)
//
// OMPL's MinimaxObjective::motionCost(s1, s2) with the state cost of maximize_min_clearance, restated over the pieces the motion
// report and the proximity report are made of (DESIGN.md section 4, "Clearance report").  Segment i, band b >= 0, c = max(nd, 1)
// states s_k, k = 1 .. c, s_c = qb (its bits), s_k = interp_dim(a, qa[a], qb[a], (double)k / (double)c) for k < c -- k_motion_expand's
// expressions; qa is not evaluated.  Per state d_k = min(b, the smallest pair distance) and p_k = the nearest pair in band (index
// into the MopaSceneDesc pair list, ties to the lower index, -1 when nothing is within the band): the bits of
// mopa_proximity_batch's clearance and pair[.,0].  Per segment:
//   clearance      min_k d_k
//   n_states       c
//   n_near         the number of k with p_k >= 0
//   k_min          the smallest k with d_k == clearance and p_k >= 0; 0 when n_near == 0
//   t_min          (double)k_min / (double)c; 0.0 when k_min == 0
//   pair_min       p_{k_min}; -1 when k_min == 0
//   end_clearance  d_c
//   q_min          s_{k_min}; qb's bits when k_min == 0
// One form at every batch size: the expanded-motion pipeline check_motion runs (mopa_motion.inc: motion_expand_chunk under
// motion_for_chunks) -> k_clearance_states, a wave per expanded state -> k_motion_clearance_reduce, a lane per segment ->
// k_motion_clearance_rows.  A segment of 200 states is 200 waves' work, never one wave's serial chain.  The pipeline's 31-bit
// chunking and its one 4-byte read-back per chunk apply: the call synchronises the stream before it returns.
// Every output word has one writer and is a plain vector store; no atomics on outputs, so two runs write the same bytes.

// k_proximity_rows reduced to the per-state minimum: the same pair sweep (wave_broad_phase / wave_each_survivor with the margin
// cull), no per-wave distance array, no K-selection.  Each lane keeps the running minimum (distance, pair index) over the
// survivors it evaluates -- a strictly smaller distance, or an equal one with a lower index -- and the wave reduces with
// wave_argmin, the reduction k_proximity_rows selects its first record with: the same order by construction.  LDS is the
// scene's own (S->lds_bytes).
// One state of that sweep, for k_clearance_states and for RRT* under the clearance objective (mopa_rrtstar_clear.inc): the active
// vector `q_active` on the env row `row` -> on every lane d = min(band, the smallest pair distance) and p = the nearest pair in
// band, -1 when there is none.  The caller synchronises the wave before the worklist / geom slab are reused.
// EXACT = true: geom_sep's exact route (gjk_distance) in the lambda; nothing else changes.
template <bool MESH, bool EXACT = false>
MOPA_D void wave_state_clearance(const SceneHdr &h, const LdsView &v, int lane, const double *q_active, const double *row,
                                 const int32_t *__restrict__ pair_model, double band, double &d_out, int &p_out) {
    const int *I = v.ints;
    wave_load_state(h, v, lane, q_active, row);
    wave_fk(h, v, lane);
    // margin broad phase
    const int wl_count = wave_broad_phase(h, v, lane, CullBand{band});
    double bd = kFar;
    int bi = 0x7fffffff;
    wave_each_survivor(h, v, lane, wl_count, [&](int p, int g1, int g2, int code) {
        const double d = geom_sep<MESH, 1, EXACT>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], band, v.dbl);
        const int pm = pair_model[p];
        if (d < bd || (d == bd && pm < bi)) { bd = d; bi = pm; }
    });
    wave_argmin(bd, bi);
    const bool near = bd <= band && bd < kFar;      // (k_proximity_rows' count rule)
    d_out = near ? bd : band;
    p_out = near ? bi : -1;
}

template <bool MESH, bool EXACT = false>
__global__ __launch_bounds__(kBlock) void k_clearance_states(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                             const int32_t *__restrict__ pair_model /*[h.npair] device pair -> index in the desc's pair list*/,
                                                             const double *__restrict__ q_states /*[T,na]*/, const double *__restrict__ qpos_env,
                                                             const int32_t *__restrict__ env_of_state /*[T]*/, long long T, double band,
                                                             unsigned long long *__restrict__ ctr, double *__restrict__ d_state /*[T]*/,
                                                             int32_t *__restrict__ p_state /*[T]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63;
    for (;;) {
        const long long s = wave_pull64(ctr, lane);
        if (s >= T) break;
        double d;
        int p;
        wave_state_clearance<MESH, EXACT>(h, v, lane, q_states + s * h.na, qpos_env + (long long)env_of_state[s] * h.nq, pair_model, band, d, p);
        if (lane == 0) {
            d_state[s] = d;
            p_state[s] = p;
        }
        wave_sync();   // worklist / geom slab are about to be reused
    }
    tile_ctr_release(ctr, lane);
}

// per segment the ordered reduction over its slots: state k sits at slot c - k, so ascending k is descending slot
__global__ __launch_bounds__(256) void k_motion_clearance_reduce(const int *__restrict__ cnt, const int *__restrict__ off, const int *__restrict__ bsum,
                                                                 const double *__restrict__ d_state, const int32_t *__restrict__ p_state, long long N,
                                                                 double band, double *__restrict__ clearance, int32_t *__restrict__ n_states,
                                                                 int32_t *__restrict__ n_near, int32_t *__restrict__ k_min, double *__restrict__ t_min,
                                                                 int32_t *__restrict__ pair_min, double *__restrict__ end_clearance) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = cnt[i], o = motion_slot0(off, bsum, i);
    double best = band;
    int kb = 0, pb = -1, near = 0;
    for (int k = 1; k <= c; k++) {
        const int p = p_state[o + (c - k)];
        if (p < 0) continue;                          // out of band: d_k == band, never below a state in band
        const double d = d_state[o + (c - k)];
        near++;
        if (kb == 0 || d < best) { best = d; kb = k; pb = p; }      // strictly smaller: the smallest k keeps a tie
    }
    clearance[i] = best;
    n_states[i] = c;
    n_near[i] = near;
    k_min[i] = kb;
    t_min[i] = kb ? (double)kb / (double)c : 0.0;
    pair_min[i] = pb;
    end_clearance[i] = d_state[o];
}

// ... and its row, one lane per output double, copied out of the expanded state buffer (k_min: what the kernel above wrote)
__global__ __launch_bounds__(256) void k_motion_clearance_rows(int na, const int *__restrict__ cnt, const int *__restrict__ off,
                                                               const int *__restrict__ bsum, const int32_t *__restrict__ k_min,
                                                               const double *__restrict__ q_states, long long N, double *__restrict__ q_min) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N * na) return;
    const long long i = e / na;
    const int a = (int)(e - i * na);
    const int c = cnt[i], k = k_min[i];
    const size_t o = (size_t)motion_slot0(off, bsum, i);
    const int j = k ? c - k : 0;                     // slot 0 holds s_c = qb
    q_min[e] = q_states[(o + j) * na + a];
}

static const LdsKernels kMotionClearanceLds({(const void *)k_clearance_states<false>, (const void *)k_clearance_states<true>,
                                              (const void *)k_clearance_states<false, true>, (const void *)k_clearance_states<true, true>});

static int motion_clearance_batch(bool exact, MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                  double band, double *clearance, int32_t *n_states, int32_t *n_near, int32_t *k_min, double *t_min,
                                  int32_t *pair_min, double *end_clearance, double *q_min, void *stream) {
    if (!S || !clearance || !n_states || !n_near || !k_min || !t_min || !pair_min || !end_clearance || (N > 0 && (!qa || !qb || !qpos_env)))
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the clearance report (mopa_motion_clearance_batch)");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    if (const int rc = band_rule(band)) return rc;
    if (S->pruned) return refuse_pruned("the proximity report needs");
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)S->lds_bytes > (size_t)kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "clearance report: the scene does not fit LDS");
    StreamScratch &sc = scratch_for(S, st);
    const int rc0 = ensure_report_ctr(S, sc);
    if (rc0 != MOPA_OK) return rc0;
    const size_t na = (size_t)S->na;
    const auto kern = exact ? (S->hdr.has_mesh ? k_clearance_states<true, true> : k_clearance_states<false, true>)
                            : (S->hdr.has_mesh ? k_clearance_states<true> : k_clearance_states<false>);
    // the expanded-motion pipeline (mopa_motion.inc), then per chunk: a wave per expanded state, a lane per segment, the row
    return motion_for_chunks(S, N, [&](int64_t first, int64_t n) {
        MotionExpanded x;
        const int rc = motion_expand_chunk(S, sc, "clearance report", qa + first * na, qb + first * na, n, samples_per_env, first, st, x);
        if (rc != MOPA_OK) return rc;
        if ((size_t)x.T * sizeof(double) > sc.mc_d.cap) {
            const size_t cap = (size_t)x.T + (size_t)x.T / 4 + 64;
            HIP_TRY(grow(S, sc.mc_d, sizeof(double) * cap));
            HIP_TRY(grow(S, sc.mc_p, sizeof(int32_t) * cap));
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)report_blocks(S, x.T)), dim3(kBlock), (size_t)S->lds_bytes, st,
                           S->hdr, S->d_dbl, S->d_int, (const int32_t *)S->d_pair_model, (const double *)x.q, qpos_env, (const int32_t *)x.env, (long long)x.T,
                           band, sc.ct_ctr.as<unsigned long long>(), sc.mc_d.as<double>(), sc.mc_p.as<int32_t>());
        hipLaunchKernelGGL(k_motion_clearance_reduce, dim3(x.nb), dim3(256), 0, st, x.cnt, x.off, x.bsum, (const double *)sc.mc_d.as<double>(),
                           (const int32_t *)sc.mc_p.as<int32_t>(), (long long)n, band, clearance + first, n_states + first, n_near + first, k_min + first,
                           t_min + first, pair_min + first, end_clearance + first);
        if (q_min) {
            const unsigned nbr = (unsigned)((n * S->na + 255) / 256);
            hipLaunchKernelGGL(k_motion_clearance_rows, dim3(nbr), dim3(256), 0, st, S->na, x.cnt, x.off, x.bsum, (const int32_t *)(k_min + first),
                               (const double *)x.q, (long long)n, q_min + first * na);
        }
        HIP_TRY(hipGetLastError());
        return (int)MOPA_OK;
    });
}
extern "C" int mopa_motion_clearance_batch(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                           double band, double *clearance, int32_t *n_states, int32_t *n_near, int32_t *k_min, double *t_min,
                                           int32_t *pair_min, double *end_clearance, double *q_min, void *stream) {
    return motion_clearance_batch(false, S, qa, qb, qpos_env, N, samples_per_env, band, clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance,
                                  q_min, stream);
}
extern "C" int mopa_motion_clearance_exact_batch(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                                 double band, double *clearance, int32_t *n_states, int32_t *n_near, int32_t *k_min, double *t_min,
                                                 int32_t *pair_min, double *end_clearance, double *q_min, void *stream) {
    return motion_clearance_batch(true, S, qa, qb, qpos_env, N, samples_per_env, band, clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance,
                                  q_min, stream);
}

// one segment, host pointers, synchronous: the active entries of qpos_a -> those of qpos_b, the passive entries from qpos_a
static int motion_clearance_one(bool exact, MopaScene *S, const double *qpos_a, const double *qpos_b, double band, double *clearance_out,
                                int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out, int32_t *pair_min_out,
                                double *end_clearance_out, double *q_min_out) {
    if (!S || !qpos_a || !qpos_b || !clearance_out || !n_states_out || !n_near_out || !k_min_out || !t_min_out || !pair_min_out || !end_clearance_out)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the clearance report (mopa_motion_clearance)");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_a);       // S->d_q: the env row, then a's active entries
    if (rc) return rc;
    const size_t na = (size_t)S->na;
    Staging g;
    const auto f_qb = g.dbl(na), f_qmin = g.dbl(na), f_clear = g.dbl(1), f_t = g.dbl(1), f_end = g.dbl(1);
    const auto f_n = g.i32(1), f_near = g.i32(1), f_k = g.i32(1), f_pair = g.i32(1);
    HIP_TRY(g.alloc());
    HIP_TRY(g.seed(f_qb, active_of(S, qpos_b).data()));
    rc = motion_clearance_batch(exact, S, S->d_q + S->nq, g.dev(f_qb), S->d_q, 1, 1, band, g.dev(f_clear), g.dev(f_n), g.dev(f_near), g.dev(f_k), g.dev(f_t),
                                g.dev(f_pair), g.dev(f_end), g.dev(f_qmin), nullptr);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(g.fetch());
    g.out(f_clear, clearance_out); g.out(f_t, t_min_out); g.out(f_end, end_clearance_out);
    g.out(f_n, n_states_out); g.out(f_near, n_near_out); g.out(f_k, k_min_out); g.out(f_pair, pair_min_out);
    g.out(f_qmin, q_min_out);
    return MOPA_OK;
}
extern "C" int mopa_motion_clearance(MopaScene *S, const double *qpos_a, const double *qpos_b, double band, double *clearance_out,
                                     int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out, int32_t *pair_min_out,
                                     double *end_clearance_out, double *q_min_out) {
    return motion_clearance_one(false, S, qpos_a, qpos_b, band, clearance_out, n_states_out, n_near_out, k_min_out, t_min_out, pair_min_out,
                                end_clearance_out, q_min_out);
}
extern "C" int mopa_motion_clearance_exact(MopaScene *S, const double *qpos_a, const double *qpos_b, double band, double *clearance_out,
                                           int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out, int32_t *pair_min_out,
                                           double *end_clearance_out, double *q_min_out) {
    return motion_clearance_one(true, S, qpos_a, qpos_b, band, clearance_out, n_states_out, n_near_out, k_min_out, t_min_out, pair_min_out,
                                end_clearance_out, q_min_out);
}
