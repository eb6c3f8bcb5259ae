// mopa_paths.inc -- planner paths -> executable trajectories on the device (rollout row of SURVEY 8f, reference
// motion_planners/sampling_based_planner.py:71-99 and rl/sac_agent.py:205-233).  (included at the end of mopa_hip.hip)
//
// What the reference does with the rows `PyKinematicPlanner.plan` returns, per query:
//   * un-wrap (`SamplingBasedPlanner.plan`): tr[0] = the current state, tr[k] = tr[k-1] + (states[k] - states[k-1]) -- a
//     strictly sequential sum; `PlannerAgent.plan` then drops row 0;
//   * densify (`SACAgent.plan`, interpolation): a waypoint further than ac_scale from its predecessor in some arm joint is
//     reached through `simple_interpolate` from the predecessor clipped by `clip_qpos`: int(s) equal steps,
//     s = max(1, max_j diff_j / (+-0.8 ac_scale)), each one validity-checked, then the waypoint itself.
// Three kernels, one wave per query, one lane per qpos coordinate (nq <= 64), with a validity launch (K1) in between:
//   k_paths_unwrap   the un-wrapped rows (in place over the planner's rows), per segment its step count (0 = short), per
//                    query the number of interior states and of output rows
//   k_paths_walk     the interior states of all long segments -> one compact array for K1
//   k_paths_assemble output rows [query][row][nq]; a query with an invalid interior state is flagged instead (the caller
//                    sends it through the fallback planners, rl/sac_agent.py:300-306)
// Every sum, quotient and compare is the reference's, in its order.

struct PathLimits {
    const double *lo_state, *hi_state, *lo_shrunk, *hi_shrunk;     // [nq], +-inf for unlimited coordinates (float32-rounded values)
};
MOPA_D double wave_max_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = (o > v) ? o : v;
    }
    return v;
}
// `clip_qpos` of a full row held one coordinate per lane (lanes >= nq carry 0 and infinite limits)
MOPA_D double clip_state_lane(double q, double lo, double hi, double lo_s, double hi_s) {
    const bool beyond = __any((q < lo) || (q > hi));
    if (!beyond) return q;
    double r = (q > lo_s) ? q : lo_s;          // np.maximum(q, lo_s)
    r = (r < hi_s) ? r : hi_s;                 // np.minimum(., hi_s)
    return r;
}
// step count of the segment start -> end (both one coordinate per lane; arm coordinates are lanes < n_arm) and its scale
MOPA_D long long segment_steps(double start, double end, int lane, int n_arm, double bound, double &scale) {
    double ratio = 0.0;
    if (lane < n_arm) {
        const double diff = end - start;
        if (diff > bound) ratio = diff / bound;
        else if (diff < -bound) ratio = diff / -bound;
    }
    const double m = wave_max_f64(ratio);
    scale = (m > 1.0) ? m : 1.0;
    return (long long)scale;                   // int(): truncation
}

__global__ __launch_bounds__(kBlock) void k_paths_unwrap(int nq, int n_arm, long long M, double *__restrict__ path, int max_path,
                                                         const int32_t *__restrict__ plen, const int32_t *__restrict__ status,
                                                         const double *__restrict__ cur, double ac_scale, double bound, int interpolate,
                                                         PathLimits lim, int32_t *__restrict__ seg_count, int32_t *__restrict__ n_walk,
                                                         int32_t *__restrict__ out_len, unsigned long long seam_mask) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= M) return;
    // coordinates of unlimited joints (`non_limited_idx`): the planner's states live in (-3.14, 3.14) there, and a step that crosses
    // the seam is taken the short way round (sampling_based_planner.py:79-97 -- 3.14, not pi, and these sums in this order)
    const bool seam = (seam_mask >> lane) & 1ull;
    const int pl = plen[q];
    if (status[q] != 0 || pl <= 0) {
        if (lane == 0) { n_walk[q] = 0; out_len[q] = 0; }
        return;
    }
    const bool on = lane < nq;
    const double lo = on ? lim.lo_state[lane] : -INFINITY, hi = on ? lim.hi_state[lane] : INFINITY;
    const double lo_s = on ? lim.lo_shrunk[lane] : -INFINITY, hi_s = on ? lim.hi_shrunk[lane] : INFINITY;
    double *P = path + (size_t)q * max_path * nq;
    double prevP = on ? P[lane] : 0.0;
    double t = on ? cur[q * nq + lane] : 0.0;
    if (on) P[lane] = t;
    int total = 0, nw = 0;
    for (int k = 1; k < pl; k++) {
        const double pk = on ? P[(size_t)k * nq + lane] : 0.0;
        double tn = t + (pk - prevP);
        if (seam && fabs(pk - prevP) > 3.14) {
            if (prevP > 0.0 && pk <= 0.0) tn = t + (((3.14 - prevP) + pk) + 3.14);
            else if (prevP < 0.0 && pk > 0.0) tn = t - (((3.14 - pk) + prevP) + 3.14);
        }
        prevP = pk;
        int cnt = 0;
        if (interpolate) {
            const double step = tn - t;
            const bool far = __any(lane < n_arm && ((step < -ac_scale) || (step > ac_scale)));
            if (far) {
                double scale;
                cnt = (int)segment_steps(clip_state_lane(t, lo, hi, lo_s, hi_s), tn, lane, n_arm, bound, scale);
            }
        }
        if (lane == 0) seg_count[q * max_path + (k - 1)] = cnt;
        total += cnt > 0 ? cnt + 1 : 1;
        nw += cnt;
        if (on) P[(size_t)k * nq + lane] = tn;
        t = tn;
    }
    if (lane == 0) { n_walk[q] = nw; out_len[q] = total; }
}

__global__ __launch_bounds__(kBlock) void k_paths_walk(int nq, int n_arm, long long M, const double *__restrict__ path, int max_path,
                                                       const int32_t *__restrict__ plen, const int32_t *__restrict__ out_len, double bound,
                                                       PathLimits lim, const int32_t *__restrict__ seg_count,
                                                       const long long *__restrict__ walk_off, double *__restrict__ walk) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= M || out_len[q] == 0) return;
    const bool on = lane < nq;
    const double lo = on ? lim.lo_state[lane] : -INFINITY, hi = on ? lim.hi_state[lane] : INFINITY;
    const double lo_s = on ? lim.lo_shrunk[lane] : -INFINITY, hi_s = on ? lim.hi_shrunk[lane] : INFINITY;
    const double *T = path + (size_t)q * max_path * nq;
    double *w = walk + (size_t)walk_off[q] * nq;
    const int pl = plen[q];
    for (int i = 0; i + 1 < pl; i++) {
        const int cnt = seg_count[q * max_path + i];
        if (cnt == 0) continue;
        const double t = on ? T[(size_t)i * nq + lane] : 0.0, tn = on ? T[(size_t)(i + 1) * nq + lane] : 0.0;
        const double s = clip_state_lane(t, lo, hi, lo_s, hi_s);
        double scale;
        (void)segment_steps(s, tn, lane, n_arm, bound, scale);
        const double per_step = (tn - s) / scale;
        double acc = s;
        for (int c = 0; c < cnt; c++) {          // cnt dependent additions, as the scalar rule
            if (lane < n_arm) acc = acc + per_step;
            if (on) w[lane] = acc;
            w += nq;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_paths_assemble(int nq, long long M, const double *__restrict__ path, int max_path,
                                                           const int32_t *__restrict__ plen, const int32_t *__restrict__ out_len,
                                                           const int32_t *__restrict__ seg_count, const long long *__restrict__ walk_off,
                                                           const double *__restrict__ walk, const unsigned char *__restrict__ walk_valid,
                                                           double *__restrict__ out, int out_rows, unsigned char *__restrict__ needs_fallback) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (q >= M) return;
    if (out_len[q] == 0) {
        if (lane == 0) needs_fallback[q] = 0;
        return;
    }
    const bool on = lane < nq;
    const double *T = path + (size_t)q * max_path * nq;
    long long wi = walk_off[q];
    double *o = out + (size_t)q * out_rows * nq;
    const int pl = plen[q];
    bool bad = false;
    for (int i = 0; i + 1 < pl; i++) {
        const int cnt = seg_count[q * max_path + i];
        for (int c = 0; c < cnt; c++) {
            bad = bad || !walk_valid[wi];
            if (on) o[lane] = walk[(size_t)wi * nq + lane];
            o += nq;
            wi++;
        }
        if (on) o[lane] = T[(size_t)(i + 1) * nq + lane];       // every piece ends in its waypoint
        o += nq;
    }
    if (lane == 0) needs_fallback[q] = bad ? 1 : 0;
}

static int paths_args_ok(int64_t M, int nq, int n_arm, int max_path) {
    if (M < 0 || nq <= 0 || nq > 64 || n_arm <= 0 || n_arm > nq || max_path <= 0) return fail(MOPA_ERR_INVALID_ARG, "bad path post-processing sizes (nq <= 64)");
    return MOPA_OK;
}
extern "C" int mopa_paths_unwrap_seam_batch(int device, int64_t M, int32_t nq, int32_t n_arm, double *path_dev, int32_t max_path,
                                            const int32_t *path_len_dev, const int32_t *status_dev, const double *cur_dev, double ac_scale,
                                            int32_t interpolate, const double *lo_state_dev, const double *hi_state_dev,
                                            const double *lo_shrunk_dev, const double *hi_shrunk_dev, int32_t *seg_count_dev,
                                            int32_t *n_walk_dev, int32_t *out_len_dev, uint64_t seam_mask, void *stream) {
    int rc = paths_args_ok(M, nq, n_arm, max_path);
    if (rc != MOPA_OK) return rc;
    if (M == 0) return MOPA_OK;
    if (!path_dev || !path_len_dev || !status_dev || !cur_dev || !lo_state_dev || !hi_state_dev || !lo_shrunk_dev || !hi_shrunk_dev ||
        !seg_count_dev || !n_walk_dev || !out_len_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(device);
    PathLimits lim{lo_state_dev, hi_state_dev, lo_shrunk_dev, hi_shrunk_dev};
    hipLaunchKernelGGL(k_paths_unwrap, dim3((unsigned)((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, (hipStream_t)stream, (int)nq,
                       (int)n_arm, (long long)M, path_dev, (int)max_path, path_len_dev, status_dev, cur_dev, ac_scale, ac_scale * 0.8,
                       (int)interpolate, lim, seg_count_dev, n_walk_dev, out_len_dev, (unsigned long long)seam_mask);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
extern "C" int mopa_paths_unwrap_batch(int device, int64_t M, int32_t nq, int32_t n_arm, double *path_dev, int32_t max_path,
                                       const int32_t *path_len_dev, const int32_t *status_dev, const double *cur_dev, double ac_scale,
                                       int32_t interpolate, const double *lo_state_dev, const double *hi_state_dev,
                                       const double *lo_shrunk_dev, const double *hi_shrunk_dev, int32_t *seg_count_dev,
                                       int32_t *n_walk_dev, int32_t *out_len_dev, void *stream) {
    return mopa_paths_unwrap_seam_batch(device, M, nq, n_arm, path_dev, max_path, path_len_dev, status_dev, cur_dev, ac_scale, interpolate,
                                        lo_state_dev, hi_state_dev, lo_shrunk_dev, hi_shrunk_dev, seg_count_dev, n_walk_dev, out_len_dev, 0ull, stream);
}
extern "C" int mopa_paths_walk_batch(int device, int64_t M, int32_t nq, int32_t n_arm, const double *path_dev, int32_t max_path,
                                     const int32_t *path_len_dev, const int32_t *out_len_dev, double ac_scale,
                                     const double *lo_state_dev, const double *hi_state_dev, const double *lo_shrunk_dev,
                                     const double *hi_shrunk_dev, const int32_t *seg_count_dev, const int64_t *walk_off_dev,
                                     double *walk_dev, void *stream) {
    int rc = paths_args_ok(M, nq, n_arm, max_path);
    if (rc != MOPA_OK) return rc;
    if (M == 0) return MOPA_OK;
    if (!path_dev || !path_len_dev || !out_len_dev || !seg_count_dev || !walk_off_dev || !walk_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(device);
    PathLimits lim{lo_state_dev, hi_state_dev, lo_shrunk_dev, hi_shrunk_dev};
    hipLaunchKernelGGL(k_paths_walk, dim3((unsigned)((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, (hipStream_t)stream, (int)nq,
                       (int)n_arm, (long long)M, path_dev, (int)max_path, path_len_dev, out_len_dev, ac_scale * 0.8, lim, seg_count_dev,
                       (const long long *)walk_off_dev, walk_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
extern "C" int mopa_paths_assemble_batch(int device, int64_t M, int32_t nq, const double *path_dev, int32_t max_path,
                                         const int32_t *path_len_dev, const int32_t *out_len_dev, const int32_t *seg_count_dev,
                                         const int64_t *walk_off_dev, const double *walk_dev, const uint8_t *walk_valid_dev,
                                         double *out_dev, int32_t out_rows, uint8_t *needs_fallback_dev, void *stream) {
    int rc = paths_args_ok(M, nq, 1, max_path);
    if (rc != MOPA_OK) return rc;
    if (M == 0) return MOPA_OK;
    if (!path_dev || !path_len_dev || !out_len_dev || !seg_count_dev || !walk_off_dev || !out_dev || !needs_fallback_dev || out_rows <= 0)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(device);
    hipLaunchKernelGGL(k_paths_assemble, dim3((unsigned)((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, (hipStream_t)stream, (int)nq,
                       (long long)M, path_dev, (int)max_path, path_len_dev, out_len_dev, seg_count_dev, (const long long *)walk_off_dev,
                       walk_dev, walk_valid_dev, out_dev, (int)out_rows, needs_fallback_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// ---- the straight-line pre-check of SACAgent.plan / simple_interpolate (rl/sac_agent.py:198-204, 236-272) for E envs ----
// Same step rule as the densification above: s = max(1, max_j diff_j / (+-0.8 ac_scale)), int(s) equal steps from the
// (already clipped) current state -- each a running sum cur + d + d + ... -- then the exact target.  Two launches around
// one validity launch (K1 on all E x K interior states, env row = the current state):
//   k_interp_walk      per env: step count and the K arm states of the walk (K = the caller's fixed width)
//   k_interp_assemble  per env: the valid prefix (up to the first invalid state among its int(s)), then the target
__global__ void k_interp_walk(int nq, int n_arm, long long E, int K, const double *__restrict__ cur, const double *__restrict__ target,
                              double bound, double *__restrict__ walk /*[E,K,n_arm]*/, int32_t *__restrict__ n_steps) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double *c = cur + e * nq, *t = target + e * nq;
    double m = 0.0;
    for (int j = 0; j < n_arm; j++) {
        const double diff = t[j] - c[j];
        double ratio = 0.0;
        if (diff > bound) ratio = diff / bound;
        else if (diff < -bound) ratio = diff / -bound;
        m = (ratio > m) ? ratio : m;
    }
    const double scale = (m > 1.0) ? m : 1.0;
    n_steps[e] = (int32_t)(long long)scale;          // int(): truncation
    double *w = walk + (size_t)e * K * n_arm;
    for (int j = 0; j < n_arm; j++) {
        const double per_step = (t[j] - c[j]) / scale;
        double acc = c[j];
        for (int k = 0; k < K; k++) {                // K dependent additions (k * d would round differently)
            acc = acc + per_step;
            w[(size_t)k * n_arm + j] = acc;
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_interp_assemble(int nq, int n_arm, long long E, int K, const double *__restrict__ cur,
                                                            const double *__restrict__ target, const double *__restrict__ walk,
                                                            const unsigned char *__restrict__ walk_valid, const int32_t *__restrict__ n_steps,
                                                            double *__restrict__ traj /*[E,K+1,nq]*/, int32_t *__restrict__ traj_len,
                                                            unsigned char *__restrict__ ok) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (e >= E) return;
    const int ns = n_steps[e] < K ? n_steps[e] : K;
    // first invalid state among the ns of the walk
    const unsigned long long badm = __ballot(lane < ns && !walk_valid[e * K + (lane < K ? lane : 0)]);
    const bool blocked = badm != 0ull;
    const int n_keep = blocked ? (int)__builtin_ctzll(badm) : ns;
    double *o = traj + (size_t)e * (K + 1) * nq;
    const double *w = walk + (size_t)e * K * n_arm;
    for (int i = lane; i < nq; i += 64) {
        const double ci = cur[e * nq + i];
        for (int k = 0; k < n_keep; k++) o[(size_t)k * nq + i] = (i < n_arm) ? w[(size_t)k * n_arm + i] : ci;
        o[(size_t)n_keep * nq + i] = target[e * nq + i];          // the exact target right after the kept prefix
    }
    if (lane == 0) {
        traj_len[e] = n_keep + 1;
        ok[e] = blocked ? 0 : 1;
    }
}

extern "C" int mopa_interpolate_batch(MopaScene *S, int64_t E, int32_t n_arm, int32_t K, const double *cur_dev, const double *target_dev,
                                      double ac_scale, double *traj_dev, int32_t *traj_len_dev, uint8_t *ok_dev, int32_t *n_steps_dev,
                                      void *stream) {
    if (!S || (E > 0 && (!cur_dev || !target_dev || !traj_dev || !traj_len_dev || !ok_dev || !n_steps_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, "the straight-line pre-check (mopa_interpolate_batch)");
    if (E < 0 || K <= 0 || K > 64 || n_arm < S->na || n_arm > S->nq) return fail(MOPA_ERR_INVALID_ARG, "bad pre-check sizes (1 <= K <= 64, na <= n_arm <= nq)");
    if (n_arm != S->na) return fail(MOPA_ERR_UNSUPPORTED, "the interpolated joints must be the planner's active joints");
    for (int a = 0; a < S->na; a++)
        if (S->active_idx[a] != a) return fail(MOPA_ERR_UNSUPPORTED, "the interpolated joints must be qpos[:n_arm]");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    StreamScratch &sc = scratch_for(S, st);
    HIP_TRY(grow(S, sc.ip_walk, (size_t)E * K * (n_arm * sizeof(double) + 1) + 16));
    double *walk = sc.ip_walk.as<double>();
    unsigned char *wv = reinterpret_cast<unsigned char *>(walk + (size_t)E * K * n_arm);
    hipLaunchKernelGGL(k_interp_walk, dim3((unsigned)((E + 127) / 128)), dim3(128), 0, st, S->nq, (int)n_arm, (long long)E, (int)K, cur_dev, target_dev,
                       ac_scale * 0.8, walk, n_steps_dev);
    int rc = launch_is_valid(S, walk, cur_dev, E * K, K, nullptr, wv, nullptr, stream);
    if (rc != MOPA_OK) return rc;
    hipLaunchKernelGGL(k_interp_assemble, dim3((unsigned)((E + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, S->nq, (int)n_arm,
                       (long long)E, (int)K, cur_dev, target_dev, walk, wv, n_steps_dev, traj_dev, traj_len_dev, ok_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
