// The `reuse_data` relabelling of a recorded agent step (mopa_rl_amd/rollout.py::reuse_transitions; the reference's loop is
// rl/mopa_rollouts.py:222-300) for E envs on the device: every env that executed more than 3 waypoints turns up to
// min(n_exec, R) random (start, goal) waypoint pairs into extra transitions ob[start] --inverse-displacement action--> ob[goal].
// Three launches, no read-back:
//   k_reuse_mark   one wave per env, lane = draw: the lane's pair (read from the caller's table, or drawn from the counter RNG as
//                  the host loop draws it), duplicates of a lower lane's pair dropped (broadcast of the lower lanes), the relabelled
//                  action's two tests (planner action on the arm entries; every entry inside [-1, 1]); the ballot of the kept
//                  lanes and its popcount go to the work buffer
//   k_reuse_scan   exclusive scan of the per-env counts in place (one workgroup, 1024 at a time with a running carry, as
//                  k_motion_scan_blocks); the total -- the true number kept, also beyond `cap` -- goes to count[0]
//   k_reuse_write  one wave per env again: the env's rows start at its scanned offset and follow the draw index (prefix popcount
//                  of the ballot), so the list is ordered by env, then draw, as the host's -- no atomics, the same bytes in every
//                  run.  Lanes over the entries of a row: the action is recomputed per joint, the two observation rows (the bulk
//                  of the bytes) are copied with consecutive lanes on consecutive doubles.  Rows at or beyond `cap` are not written.
// The arithmetic is agent_planning.displacement_to_action operation by operation (two successive divisions in the far branch, the
// sign taken of the displacement); the library is built with -ffp-contract=off, so the rows equal the host function's bit for bit
// (tests/test_reuse_gpu.py).

struct ReuseArgs {
    long long E;
    int L, D, nq, n_arm, dof, grip, R, normal_space;
    double ac_scale, omega, omega_over_scale, c1, c2, action_range;
    const double *ob, *meta_rew, *waypoint, *inv_disc;
    const unsigned char *done, *env_mask;
    const long long *n_exec;
    const int *ac_type, *pairs;
    unsigned long long seed, stream0;      // drawn mode: env e draws from rng_key(seed, stream0 + e)
    long long cap;
    long long *off;                        // work [E]: kept draws per env, then (after the scan) the env's first row
    unsigned long long *kept;              // work [E]: ballot of the kept lanes
    long long *count;
    int *out_env, *out_start, *out_goal, *out_intra, *out_ac_type;
    double *out_ac, *out_rew, *out_ob, *out_ob_next;
    unsigned char *out_done;
};

// displacement_to_action on one entry
__device__ __forceinline__ double reuse_action(const ReuseArgs &a, double disp) {
    if (a.normal_space) return disp / a.action_range;
    const double mag = fabs(disp);
    const double stretch = (mag - a.ac_scale) / a.c1 / a.c2;
    const double sgn = (disp > 0.0) ? 1.0 : ((disp < 0.0) ? -1.0 : disp);      // np.sign (0 -> 0, nan -> nan)
    return (mag < a.ac_scale) ? disp * a.omega_over_scale : sgn * (stretch + a.omega);
}

// waypoints the env's record holds, 0 for an env that takes no part (masked out, or no more than 3 waypoints executed)
__device__ __forceinline__ int reuse_len(const ReuseArgs &a, long long e) {
    if (a.env_mask && a.env_mask[e] == 0) return 0;
    const long long n = a.n_exec[e];
    if (n <= 3) return 0;
    return (int)(n < a.L ? n : a.L);       // (a record never holds more than its L rows)
}

// draw `lane` of env e: false when the lane has no draw, or the table's entry is (-1, -1) / out of range
__device__ __forceinline__ bool reuse_pair(const ReuseArgs &a, long long e, int lane, int n, int &start, int &goal) {
    start = goal = -1;
    if (lane >= a.R) return false;
    if (a.pairs) {
        start = a.pairs[(e * a.R + lane) * 2];
        goal = a.pairs[(e * a.R + lane) * 2 + 1];
        return 0 <= start && start < goal && goal < n;
    }
    if (lane >= n) return false;
    // randint(low, high) = low + min(int(u * (high - low)), high - low - 1): start in [0, n - 1), goal in [start + 1, n)
    const uint64_t key = rng_key(a.seed, a.stream0 + (uint64_t)e);
    const double u1 = rng_uniform_k(key, 2ull * lane), u2 = rng_uniform_k(key, 2ull * lane + 1ull);
    const long long s = (long long)(u1 * (double)(n - 1));
    start = (int)(s < n - 2 ? s : n - 2);
    const long long g = (long long)(u2 * (double)(n - 1 - start));
    goal = start + 1 + (int)(g < n - 2 - start ? g : n - 2 - start);
    return true;
}

__global__ __launch_bounds__(256) void k_reuse_mark(ReuseArgs a) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= a.E) return;
    const int n = reuse_len(a, e);
    unsigned long long m = 0ull;
    if (n > 0) {                           // (uniform over the wave)
        int start, goal;
        const bool have = reuse_pair(a, e, lane, n, start, goal);
        // `(start, goal) in seen`: a pair some lower lane holds (kept or not) is skipped
        bool dup = false;
        const int nl = a.pairs ? a.R : (n < a.R ? n : a.R);
        for (int j = 0; j + 1 < nl; j++) {
            const int sj = __shfl(start, j, 64), gj = __shfl(goal, j, 64);
            const int hj = __shfl((int)have, j, 64);
            dup |= j < lane && hj && sj == start && gj == goal;
        }
        bool keep = false;
        if (have && !dup) {
            const double *ws = a.waypoint + ((size_t)e * a.L + start) * a.nq, *wg = a.waypoint + ((size_t)e * a.L + goal) * a.nq;
            bool planner = false, in_box = true;
            for (int j = 0; j < a.n_arm; j++) {
                const double v = reuse_action(a, wg[j] - ws[j]);
                planner |= (v < -a.omega) || (v > a.omega);
                in_box &= (v >= -1.0) && (v <= 1.0);
            }
            if (a.grip >= 0) {
                const double v = wg[a.grip] - ws[a.grip];
                in_box &= (v >= -1.0) && (v <= 1.0);
            }
            keep = planner && in_box;
        }
        m = __ballot(keep);
    }
    if (lane == 0) {
        a.kept[e] = m;
        a.off[e] = __popcll(m);
    }
}

__global__ __launch_bounds__(1024) void k_reuse_scan(long long *__restrict__ off, long long E, long long *__restrict__ count) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (long long first = 0; first < E; first += 1024) {
        const long long i = first + threadIdx.x;
        const long long x = i < E ? off[i] : 0;
        long long incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long base = carry_s;
        for (int w = 0; w < wave; w++) base += wsum[w];
        if (i < E) off[i] = base + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = carry_s;
}

__global__ __launch_bounds__(256) void k_reuse_write(ReuseArgs a) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= a.E) return;
    unsigned long long m = a.kept[e];
    if (!m) return;
    long long row = a.off[e];
    int start, goal;
    reuse_pair(a, e, lane, reuse_len(a, e), start, goal);
    const int D = a.D, dof = a.dof;
    for (; m && row < a.cap; m &= m - 1ull, row++) {
        const int k = __builtin_ctzll(m);
        const int s = __shfl(start, k, 64), g = __shfl(goal, k, 64);
        const double *ws = a.waypoint + ((size_t)e * a.L + s) * a.nq, *wg = a.waypoint + ((size_t)e * a.L + g) * a.nq;
        if (lane < a.n_arm) a.out_ac[row * dof + lane] = reuse_action(a, wg[lane] - ws[lane]);
        else if (lane < dof) a.out_ac[row * dof + lane] = wg[a.grip] - ws[a.grip];
        if (lane == 0) {
            a.out_env[row] = (int)e;
            a.out_start[row] = s;
            a.out_goal[row] = g;
            a.out_rew[row] = (a.meta_rew[e * a.L + g] - a.meta_rew[e * a.L + s]) * a.inv_disc[s];
            a.out_done[row] = a.done[e * a.L + g];
            a.out_intra[row] = g - s - 1;
            if (a.out_ac_type) a.out_ac_type[row] = a.ac_type[e];
        }
        const double *os = a.ob + ((size_t)e * a.L + s) * D, *og = a.ob + ((size_t)e * a.L + g) * D;
        for (int i = lane; i < D; i += 64) {
            a.out_ob[row * D + i] = os[i];
            a.out_ob_next[row * D + i] = og[i];
        }
    }
}

extern "C" int mopa_reuse_batch(int64_t E, int32_t L, int32_t D, int32_t nq, int32_t n_arm, int32_t dof, int32_t grip_qpos_idx,
                                const double *ob_dev, const double *meta_rew_dev, const uint8_t *done_dev, const double *waypoint_dev,
                                const int64_t *n_exec_dev, const int32_t *ac_type_dev, const uint8_t *env_mask_dev,
                                double ac_scale, double omega, double omega_over_scale, double c1, double c2, double action_range, int32_t normal_space,
                                const double *inv_disc_dev, int32_t R, const int32_t *pairs_dev, uint64_t seed, int64_t env_id_base, int64_t env_id_total,
                                int64_t cap, int64_t *work_dev, int64_t *count_dev, int32_t *out_env_dev, int32_t *out_start_dev, int32_t *out_goal_dev,
                                double *out_ac_dev, double *out_rew_dev, uint8_t *out_done_dev, int32_t *out_intra_dev, double *out_ob_dev,
                                double *out_ob_next_dev, int32_t *out_ac_type_dev, void *stream) {
    if (R < 1 || R > 64) return fail(MOPA_ERR_INVALID_ARG, "reuse: max_reuse_data (R) outside 1..64");
    if (n_arm > dof) return fail(MOPA_ERR_INVALID_ARG, "reuse: n_arm > dof");
    if (cap < 0) return fail(MOPA_ERR_INVALID_ARG, "reuse: cap < 0");
    if (!ob_dev || !meta_rew_dev || !done_dev || !waypoint_dev || !n_exec_dev || !inv_disc_dev || !work_dev || !count_dev)
        return fail(MOPA_ERR_INVALID_ARG, "reuse: null buffer");
    // (cap == 0 asks for the count alone: no row is written, no column needed)
    if (cap > 0 && (!out_env_dev || !out_start_dev || !out_goal_dev || !out_ac_dev || !out_rew_dev || !out_done_dev || !out_intra_dev || !out_ob_dev ||
                    !out_ob_next_dev || (ac_type_dev && !out_ac_type_dev)))
        return fail(MOPA_ERR_INVALID_ARG, "reuse: null output column");
    if (!ac_type_dev) out_ac_type_dev = nullptr;
    if (E < 0 || E > 0x7fffffffLL || L < 1 || D < 1 || nq < 1 || n_arm < 1 || n_arm > nq || dof > 64 || grip_qpos_idx >= nq ||
        dof != n_arm + (grip_qpos_idx >= 0 ? 1 : 0) || env_id_base < 0 || env_id_total < 0)
        return fail(MOPA_ERR_INVALID_ARG, "reuse: bad sizes (E, L, D, nq >= 1; n_arm <= nq; dof = n_arm [+ 1 with a gripper index < nq] <= 64)");
    ReuseArgs a;
    a.E = E; a.L = L; a.D = D; a.nq = nq; a.n_arm = n_arm; a.dof = dof; a.grip = grip_qpos_idx < 0 ? -1 : grip_qpos_idx; a.R = R;
    a.normal_space = normal_space != 0;
    a.ac_scale = ac_scale; a.omega = omega; a.omega_over_scale = omega_over_scale; a.c1 = c1; a.c2 = c2; a.action_range = action_range;
    a.ob = ob_dev; a.meta_rew = meta_rew_dev; a.waypoint = waypoint_dev; a.inv_disc = inv_disc_dev;
    a.done = done_dev; a.env_mask = env_mask_dev;
    a.n_exec = (const long long *)n_exec_dev;
    a.ac_type = ac_type_dev; a.pairs = pairs_dev;
    a.seed = seed;
    a.stream0 = 3ull * (uint64_t)(env_id_total ? env_id_total : E) + (uint64_t)env_id_base;
    a.cap = cap;
    a.off = (long long *)work_dev;
    a.kept = (unsigned long long *)(work_dev + E);
    a.count = (long long *)count_dev;
    a.out_env = out_env_dev; a.out_start = out_start_dev; a.out_goal = out_goal_dev; a.out_intra = out_intra_dev; a.out_ac_type = out_ac_type_dev;
    a.out_ac = out_ac_dev; a.out_rew = out_rew_dev; a.out_ob = out_ob_dev; a.out_ob_next = out_ob_next_dev;
    a.out_done = out_done_dev;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((E + 3) / 4)), block(256);
    if (E > 0) hipLaunchKernelGGL(k_reuse_mark, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_reuse_scan, dim3(1), dim3(1024), 0, st, a.off, (long long)E, a.count);
    if (E > 0 && cap > 0) hipLaunchKernelGGL(k_reuse_write, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
