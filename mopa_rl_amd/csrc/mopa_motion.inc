// mopa_motion.inc -- K2, large batches: discrete motion validation through the lane-per-state validity kernel.
// (included by mopa_hip.hip right after launch_is_valid)
//
// OMPL's DiscreteMotionValidator accepts a segment iff its end state and the nd-1 interior states
// interpolate(a, b, k/nd) are all valid -- the verdict does not depend on the order they are tested in.  The
// wave-per-segment kernel (k_check_motion) tests them one after the other with the wave-per-state routine
// (~60 M segments/s for planner-length segments); here the states of ALL segments are written out
// (count + block-local scan -> scan of the block sums -> expand), validated in one launch of k_is_valid_v5 / v2 with an explicit env index per state,
// and AND-ed back per segment.  Same nd, same interpolation arithmetic, same validity routine => same verdicts.
// The total number of states is read back once per chunk (4 bytes, stream-synchronising) to size the launch.
// The pipeline up to the expanded states (motion_expand_chunk under motion_for_chunks) is also the front of the motion report
// (mopa_motion_report.inc) and of the clearance report (mopa_motion_clearance.inc); each adds its own tail.

// exclusive prefix sum of one int per thread over a 256-thread block (wave prefix by DPP-free shuffles + the four wave sums
// through LDS); returns the thread's offset inside the block and, through `block_total`, the block's sum
__device__ __forceinline__ int block_exclusive_scan_256(int x, int &block_total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) base += wsum[w];
    }
    block_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + incl - x;
}

// per segment: its state count nd (end state + nd-1 interior states; nd == 0: the end state alone) and its offset inside its
// block of 256 segments; per block: the sum of its counts
__global__ __launch_bounds__(256) void k_motion_count(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                      const double *__restrict__ qa, const double *__restrict__ qb, long long N,
                                                      int *__restrict__ cnt, int *__restrict__ off, int *__restrict__ bsum) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int c = 0;
    if (i < N) {
        const LdsView v = global_view(g_dbl, g_int);
        const int nd = valid_segment_count(h, v, qa + i * h.na, qb + i * h.na);
        c = nd > 0 ? nd : 1;
        cnt[i] = c;
    }
    int total;
    const int o = block_exclusive_scan_256(c, total);
    if (i < N) off[i] = o;
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// exclusive scan of the block sums in place (one workgroup walks them 1024 at a time with a running carry); the grand
// total -- the number of states of the chunk -- goes to bsum[nb]
__global__ __launch_bounds__(1024) void k_motion_scan_blocks(int *__restrict__ bsum, int nb) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int start = 0; start < nb; start += 1024) {
        const int i = start + threadIdx.x;
        const int x = i < nb ? bsum[i] : 0;
        int incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int base = carry_s;
        for (int w = 0; w < wave; w++) base += wsum[w];
        if (i < nb) bsum[i] = base + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry_s;
}

// slot 0 of segment i in the expanded buffers (it holds the segment's END state; state k sits at slot c - k): the segment's offset
// inside its block of 256 segments + the offset of the block
MOPA_D int motion_slot0(const int *__restrict__ off, const int *__restrict__ bsum, long long i) { return off[i] + bsum[i >> 8]; }

__global__ void k_motion_expand(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                const double *__restrict__ qa, const double *__restrict__ qb, long long N, long long samples_per_env,
                                long long first, const int *__restrict__ cnt, const int *__restrict__ off, const int *__restrict__ bsum,
                                double *__restrict__ q_states, int *__restrict__ env_of_state) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const LdsView v = global_view(g_dbl, g_int);
    const double *a = qa + i * h.na, *b = qb + i * h.na;
    const int nd = cnt[i];
    const int env = (int)((first + i) / samples_per_env);     // `first`: index of this chunk's segment 0 in the caller's batch
    const int o = motion_slot0(off, bsum, i);
    double *out = q_states + (size_t)o * h.na;
    for (int k = nd; k >= 1; k--) {          // k == nd: the end state itself
        const double t = (double)k / (double)nd;
        for (int j = 0; j < h.na; j++) out[j] = (k == nd) ? b[j] : interp_dim(h, v, j, a[j], b[j], t);
        env_of_state[o + (nd - k)] = env;
        out += h.na;
    }
}

__global__ void k_motion_reduce(const int *__restrict__ cnt, const int *__restrict__ off, const int *__restrict__ bsum,
                                const unsigned char *__restrict__ vstate, long long N, unsigned char *__restrict__ valid) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned char ok = 1;
    const int o = motion_slot0(off, bsum, i);
    for (int k = 0; k < cnt[i]; k++) ok &= vstate[o + k];
    valid[i] = ok;
}

// The expanded-motion pipeline of one chunk, as its users (check_motion, the motion report, the clearance report) find it: per segment
// its state count and offset inside its block, per block its offset (motion_slot0 puts the two together), and the T expanded
// states with the env row of each.  All of it is the stream's scratch: it holds until the next expansion on the stream.
struct MotionExpanded {
    const int32_t *cnt, *off, *bsum;
    unsigned nb;          // blocks of 256 segments
    int64_t T;            // expanded states, 1 .. INT32_MAX
    double *q;            // [T, na]
    int32_t *env;         // [T]
};

// count -> block-local scan -> scan of the block sums -> expand for segments [first, first + N) of the caller's batch (qa, qb: the
// chunk's own rows).  The number of states is read back once (4 bytes, stream-synchronising) to size what follows; the state
// offsets of a chunk fit an int32 by construction (motion_for_chunks).  `what` opens the MOPA_ERR_LIMIT message.
static int motion_expand_chunk(MopaScene *S, StreamScratch &sc, const char *what, const double *qa, const double *qb, int64_t N,
                               int64_t samples_per_env, int64_t first, hipStream_t st, MotionExpanded &x) {
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
    if (T <= 0 || T > 0x7fffffffLL) return fail(MOPA_ERR_LIMIT, std::string(what) + ": state count of a chunk does not fit 31 bits");
    // mv_q, mv_env and mv_valid grow together, under mv_q's test: the users size the per-state verdicts (mv_valid) by mv_q's capacity
    // and never test it on their own, so a pipeline that grew mv_q alone would leave the next validation a short verdict buffer.
    const size_t cap = (size_t)T + (size_t)T / 4 + 64;
    if ((size_t)T * S->na * sizeof(double) > sc.mv_q.cap) {
        HIP_TRY(grow(S, sc.mv_q, sizeof(double) * cap * S->na));
        HIP_TRY(grow(S, sc.mv_env, sizeof(int32_t) * cap));
        HIP_TRY(grow(S, sc.mv_valid, cap));
    }
    hipLaunchKernelGGL(k_motion_expand, dim3(nb), dim3(256), 0, st, S->hdr, S->d_dbl, S->d_int, qa, qb, (long long)N,
                       (long long)samples_per_env, (long long)first, cnt, off, bsum, sc.mv_q.as<double>(), sc.mv_env.as<int32_t>());
    x = MotionExpanded{cnt, off, bsum, nb, T, sc.mv_q.as<double>(), sc.mv_env.as<int32_t>()};
    return MOPA_OK;
}

// per_chunk(first, n) over the batch in chunks of the scene's motion_chunk segments (K1Policy: few enough that every 32-bit offset
// of the pipeline above stays in range); the first failure ends the walk
template <class F>
static int motion_for_chunks(const MopaScene *S, int64_t N, F per_chunk) {
    const int64_t chunk = S->k1.motion_chunk;
    for (int64_t first = 0; first < N; first += chunk) {
        const int rc = per_chunk(first, std::min(chunk, N - first));
        if (rc != MOPA_OK) return rc;
    }
    return MOPA_OK;
}

// large batches of check_motion: the expanded states through launch_is_valid, AND-ed back per segment
static int motion_expanded(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N, int64_t samples_per_env,
                           uint8_t *valid, hipStream_t st) {
    StreamScratch &sc = scratch_for(S, st);
    const size_t na = (size_t)S->na;
    return motion_for_chunks(S, N, [&](int64_t first, int64_t n) {
        MotionExpanded x;
        int rc = motion_expand_chunk(S, sc, "motion validation", qa + first * na, qb + first * na, n, samples_per_env, first, st, x);
        if (rc != MOPA_OK) return rc;
        rc = launch_is_valid(S, x.q, qpos_env, x.T, 1, x.env, sc.mv_valid.as<uint8_t>(), nullptr, st);
        if (rc != MOPA_OK) return rc;
        hipLaunchKernelGGL(k_motion_reduce, dim3(x.nb), dim3(256), 0, st, x.cnt, x.off, x.bsum, sc.mv_valid.as<uint8_t>(), (long long)n, valid + first);
        HIP_TRY(hipGetLastError());
        return (int)MOPA_OK;
    });
}
