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
// One form at every batch size: k_motion_count -> k_motion_scan_blocks -> k_motion_expand (all unchanged, mopa_motion.inc) ->
// k_clearance_states, a wave per expanded state -> k_motion_clearance_reduce, a lane per segment -> k_motion_clearance_rows.  A
// segment of 200 states is 200 waves' work, never one wave's serial chain.  motion_expanded's 31-bit chunking and its one 8-byte
// read-back per chunk apply: the call synchronises the stream before it returns.
// Every output word has one writer and is a plain vector store; no atomics on outputs, so two runs write the same bytes.

// k_proximity_rows reduced to the per-state minimum: no per-wave distance array, no K-selection.  Each lane keeps the running
// minimum (distance, pair index) over the survivors it evaluates -- a strictly smaller distance, or an equal one with a lower
// index -- and the wave reduces under the same rule, which is the (distance, index) order k_proximity_rows selects its first
// record by.  LDS is the scene's own (S->lds_bytes).
template <bool MESH>
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
    const int *I = v.ints;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (;;) {
        unsigned long long t = 0ull;
        if (lane == 0) t = atomicAdd(ctr, 1ull);
        const unsigned t_lo = __builtin_amdgcn_readfirstlane((unsigned)t), t_hi = __builtin_amdgcn_readfirstlane((unsigned)(t >> 32));
        const long long s = (long long)(((unsigned long long)t_hi << 32) | t_lo);
        if (s >= T) break;
        wave_load_state(h, v, lane, q_states + s * h.na, qpos_env + (long long)env_of_state[s] * h.nq);
        wave_fk(h, v, lane);
        // margin broad phase + ballot compaction (order-preserving: the worklist stays sorted by narrow-phase class)
        int wl_count = 0;
        for (int base = 0; base < h.npair; base += 64) {
            const int p = base + lane;
            bool surv = false;
            if (p < h.npair) {
                const int pk = I[h.o_pairs + p];
                const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff;
                surv = !pair_culled_band(h, v, g1, g2, geom_rec(h, v, g1), geom_rec(h, v, g2), band);
            }
            const unsigned long long mask = __ballot(surv);
            if (surv) v.wl[wl_count + __popcll(mask & lt)] = (unsigned short)p;
            wl_count += __popcll(mask);
        }
        wave_sync();
        double bd = kFar;
        int bi = 0x7fffffff;
        for (int base = 0; base < wl_count; base += 64) {
            const int i = base + lane;
            if (i < wl_count) {
                const int p = v.wl[i];
                const int pk = I[h.o_pairs + p];
                const int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
                const double d = geom_sep<MESH>(code, geom_rec(h, v, g1), I[h.o_g_type + g1], geom_rec(h, v, g2), I[h.o_g_type + g2], band, v.dbl);
                const int pm = pair_model[p];
                if (d < bd || (d == bd && pm < bi)) { bd = d; bi = pm; }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) {
            const bool near = bd <= band && bd < kFar;      // (k_proximity_rows' count rule)
            d_state[s] = near ? bd : band;
            p_state[s] = near ? bi : -1;
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
    const int c = cnt[i], o = off[i] + bsum[i >> 8];
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
    const size_t o = (size_t)(off[i] + bsum[i >> 8]);
    const int j = k ? c - k : 0;                     // slot 0 holds s_c = qb
    q_min[e] = q_states[(o + j) * na + a];
}

// one chunk of segments: motion_report_expanded_chunk's pipeline with the per-state minimum in place of the verdict
static int motion_clearance_chunk(MopaScene *S, StreamScratch &sc, const double *qa, const double *qb, const double *qpos_env, int64_t N,
                                  int64_t samples_per_env, int64_t first, double band, double *clearance, int32_t *n_states, int32_t *n_near,
                                  int32_t *k_min, double *t_min, int32_t *pair_min, double *end_clearance, double *q_min, hipStream_t st) {
    HIP_TRY(grow(S, sc.mv_cnt, sizeof(int32_t) * (size_t)N));
    HIP_TRY(grow(S, sc.mv_off, sizeof(int32_t) * (size_t)N));
    int32_t *cnt = sc.mv_cnt.as<int32_t>(), *off = sc.mv_off.as<int32_t>();
    const unsigned nb = (unsigned)((N + 255) / 256);
    HIP_TRY(grow(S, sc.mv_scan, sizeof(int32_t) * ((size_t)nb + 1)));
    int32_t *bsum = sc.mv_scan.as<int32_t>();
    hipLaunchKernelGGL(k_motion_count, dim3(nb), dim3(256), 0, st, S->hdr, S->d_dbl, S->d_int, qa, qb, (long long)N, cnt, off, bsum);
    hipLaunchKernelGGL(k_motion_scan_blocks, dim3(1), dim3(1024), 0, st, bsum, (int)nb);
    int32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, bsum + nb, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t T = total;
    if (T <= 0 || T > 0x7fffffffLL) return fail(MOPA_ERR_LIMIT, "clearance report: state count of a chunk does not fit 31 bits");
    const size_t cap = (size_t)T + (size_t)T / 4 + 64;
    if ((size_t)T * S->na * sizeof(double) > sc.mv_q.cap) {      // (the three grow together: the validation pipelines size mv_valid by mv_q's capacity)
        HIP_TRY(grow(S, sc.mv_q, sizeof(double) * cap * S->na));
        HIP_TRY(grow(S, sc.mv_env, sizeof(int32_t) * cap));
        HIP_TRY(grow(S, sc.mv_valid, cap));
    }
    if ((size_t)T * sizeof(double) > sc.mc_d.cap) {
        HIP_TRY(grow(S, sc.mc_d, sizeof(double) * cap));
        HIP_TRY(grow(S, sc.mc_p, sizeof(int32_t) * cap));
    }
    hipLaunchKernelGGL(k_motion_expand, dim3(nb), dim3(256), 0, st, S->hdr, S->d_dbl, S->d_int, qa, qb, (long long)N,
                       (long long)samples_per_env, (long long)first, cnt, off, bsum, sc.mv_q.as<double>(), sc.mv_env.as<int32_t>());
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((T + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)S->n_cu * 2));
    hipLaunchKernelGGL(S->hdr.has_mesh ? k_clearance_states<true> : k_clearance_states<false>, dim3((unsigned)blocks), dim3(kBlock), (size_t)S->lds_bytes, st,
                       S->hdr, S->d_dbl, S->d_int, (const int32_t *)S->d_pair_model, (const double *)sc.mv_q.as<double>(), qpos_env,
                       (const int32_t *)sc.mv_env.as<int32_t>(), (long long)T, band, sc.ct_ctr.as<unsigned long long>(), sc.mc_d.as<double>(),
                       sc.mc_p.as<int32_t>());
    hipLaunchKernelGGL(k_motion_clearance_reduce, dim3(nb), dim3(256), 0, st, cnt, off, bsum, (const double *)sc.mc_d.as<double>(),
                       (const int32_t *)sc.mc_p.as<int32_t>(), (long long)N, band, clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance);
    if (q_min) {
        const unsigned nbr = (unsigned)((N * S->na + 255) / 256);
        hipLaunchKernelGGL(k_motion_clearance_rows, dim3(nbr), dim3(256), 0, st, S->na, cnt, off, bsum, (const int32_t *)k_min,
                           (const double *)sc.mv_q.as<double>(), (long long)N, q_min);
    }
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

static void motion_clearance_register_lds() {
    for (const void *k : {(const void *)k_clearance_states<false>, (const void *)k_clearance_states<true>})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
}

extern "C" int mopa_motion_clearance_batch(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                           double band, double *clearance, int32_t *n_states, int32_t *n_near, int32_t *k_min, double *t_min,
                                           int32_t *pair_min, double *end_clearance, double *q_min, void *stream) {
    if (!S || !clearance || !n_states || !n_near || !k_min || !t_min || !pair_min || !end_clearance || (N > 0 && (!qa || !qb || !qpos_env)))
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the clearance report (mopa_motion_clearance_batch)");
    if (N < 0 || samples_per_env <= 0) return fail(MOPA_ERR_INVALID_ARG, "N < 0 or samples_per_env <= 0");
    if (!std::isfinite(band) || !(band >= 0.0)) return fail(MOPA_ERR_INVALID_ARG, "band must be finite and >= 0");
    if (S->pruned)
        return fail(MOPA_ERR_UNSUPPORTED, "a scene with pair_cull_radius is proven down to its contact_threshold only: the proximity report needs the full scene");
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)S->lds_bytes > (size_t)kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "clearance report: the scene does not fit LDS");
    StreamScratch &sc = scratch_for(S, st);
    if (!sc.ct_ctr.p) {      // the contact report's counter: zeroed once, synchronously; the kernel puts it back to zero (tile_ctr_release)
        HIP_TRY(grow(S, sc.ct_ctr, 64));
        HIP_TRY(hipMemset(sc.ct_ctr.p, 0, 64));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    // (the chunk size of motion_expanded: every 32-bit offset of the count -> scan -> expand pipeline stays in range)
    const int64_t per_seg = (int64_t)std::ceil(1.0 / S->hdr.resolution) + 2;
    const int64_t chunk = std::max<int64_t>(1, 0x7fffffffLL / per_seg);
    const size_t na = (size_t)S->na;
    for (int64_t first = 0; first < N; first += chunk) {
        const int64_t n = std::min(chunk, N - first);
        const int rc = motion_clearance_chunk(S, sc, qa + first * na, qb + first * na, qpos_env, n, samples_per_env, first, band, clearance + first,
                                              n_states + first, n_near + first, k_min + first, t_min + first, pair_min + first, end_clearance + first,
                                              q_min ? q_min + first * na : nullptr, st);
        if (rc != MOPA_OK) return rc;
    }
    return MOPA_OK;
}

// one segment, host pointers, synchronous: the active entries of qpos_a -> those of qpos_b, the passive entries from qpos_a
extern "C" int mopa_motion_clearance(MopaScene *S, const double *qpos_a, const double *qpos_b, double band, double *clearance_out,
                                     int32_t *n_states_out, int32_t *n_near_out, int32_t *k_min_out, double *t_min_out, int32_t *pair_min_out,
                                     double *end_clearance_out, double *q_min_out) {
    if (!S || !qpos_a || !qpos_b || !clearance_out || !n_states_out || !n_near_out || !k_min_out || !t_min_out || !pair_min_out || !end_clearance_out)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the clearance report (mopa_motion_clearance)");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_a);       // S->d_q: the env row, then a's active entries
    if (rc) return rc;
    const size_t na = (size_t)S->na;
    // doubles: qb | q_min | clearance, t_min, end_clearance; int32: n_states, n_near, k_min, pair_min
    const size_t n_dbl = 2 * na + 3, n_i32 = 4;
    std::vector<double> hb(na);
    for (size_t a = 0; a < na; a++) hb[a] = qpos_b[S->active_idx[a]];
    void *buf = nullptr;
    HIP_TRY(hipMalloc(&buf, n_dbl * sizeof(double) + n_i32 * sizeof(int32_t)));
    double *d = static_cast<double *>(buf);
    int32_t *w = reinterpret_cast<int32_t *>(d + n_dbl);
    hipError_t e = hipMemcpy(d, hb.data(), na * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = mopa_motion_clearance_batch(S, S->d_q + S->nq, d, S->d_q, 1, 1, band, d + 2 * na, w, w + 1, w + 2, d + 2 * na + 1, w + 3, d + 2 * na + 2,
                                         d + na, nullptr);
        std::vector<double> hd(n_dbl);
        int32_t hw[4] = {0, 0, 0, 0};
        if (rc == MOPA_OK) {
            e = hipMemcpy(hd.data(), d, n_dbl * sizeof(double), hipMemcpyDeviceToHost);      // (synchronises with the null stream's launches)
            if (e == hipSuccess) e = hipMemcpy(hw, w, n_i32 * sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        if (rc == MOPA_OK && e == hipSuccess) {
            *clearance_out = hd[2 * na];
            *t_min_out = hd[2 * na + 1];
            *end_clearance_out = hd[2 * na + 2];
            *n_states_out = hw[0];
            *n_near_out = hw[1];
            *k_min_out = hw[2];
            *pair_min_out = hw[3];
            if (q_min_out) std::memcpy(q_min_out, &hd[na], na * sizeof(double));
        }
    }
    (void)hipFree(buf);
    if (rc != MOPA_OK) return rc;
    HIP_TRY(e);
    return MOPA_OK;
}
