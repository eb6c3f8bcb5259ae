// The replay sink (mopa_rl_amd/replay.py::DeviceReplayBuffer; the reference's rl/dataset.py as the trainer uses it: every stored
// rollout holds one transition, the ring overwrites the oldest, the sampler draws uniformly over what is stored -- DESIGN section 4
// "Replay sink").  One ring [capacity, W] float32, W = 2 * D + A + 4, a row being
//     ob[D] | ac[A] | rew | done | intra_steps | ac_type | ob_next[D]
// and a device state [2] int64: {rows appended since creation, min(that, capacity)}.  Nothing is read back.
//   k_replay_scan     one workgroup.  Masked sources: the exclusive scan of the keep flags, 1024 at a time with a running carry (as
//                     k_reuse_scan; the rank inside a wave is a ballot's prefix popcount) -> work[i] = rank of row i among the kept
//                     rows, or -1.  Every source: the head the call starts from and the number kept go to work[n], work[n + 1], and
//                     the state moves on -- here, in the launch in front of the copy, so that no row of the copy races with it.
//   k_replay_copy     32 lanes per source row, consecutive lanes on consecutive entries of the row (a coalesced read of the f64 columns
//                     or of the packed record, a coalesced 4 * W byte write): the k-th kept row goes to ring row (head + k) % capacity;
//                     of more than `capacity` kept rows the first m - capacity are skipped, so no ring row is written twice.
//   k_replay_sample   32 lanes per drawn row: index min(int(u * size), size - 1) from the counter RNG, the ring row copied as words.
// The order is computed, not raced for: two runs write the same bytes.  Doubles are narrowed with (float)x (round to nearest even).

#define REPLAY_LANES 32     // lanes per row (8 rows per 256-thread workgroup)

struct ReplaySrc {
    long long n;
    int D, A, ac_ld, intra64;
    const unsigned char *mask;             // [n] bytes, or NULL
    const long long *count;                // [1], or NULL
    const double *ob, *ac, *rew, *ob_next;
    const unsigned char *done;
    const void *intra;                     // [n] int64 (intra64) or int32
    const int *ac_type;                    // [n] or NULL (stored as 0)
    const float *packed;                   // [n, W] exchange records (column D + A + 3 is the mask), or NULL: the columns above
};

__global__ __launch_bounds__(1024) void k_replay_scan(ReplaySrc s, long long capacity, long long *__restrict__ state, long long *__restrict__ work) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = s.n;
    long long m;
    if (s.mask || s.packed) {
        const int W = 2 * s.D + s.A + 4, col = s.D + s.A + 3;
        if (threadIdx.x == 0) carry_s = 0;
        __syncthreads();
        for (long long first = 0; first < n; first += 1024) {
            const long long i = first + threadIdx.x;
            bool keep = false;
            if (i < n) keep = s.packed ? (s.packed[i * W + col] != 0.0f) : (s.mask[i] != 0);
            const unsigned long long b = __ballot(keep);
            if (lane == 0) wsum[wave] = __popcll(b);
            __syncthreads();
            long long base = carry_s;
            for (int w = 0; w < wave; w++) base += wsum[w];
            if (i < n) work[i] = keep ? base + __popcll(b & ((1ull << lane) - 1ull)) : -1;
            __syncthreads();
            if (threadIdx.x == 1023) carry_s = base + __popcll(b);
            __syncthreads();
        }
        m = carry_s;
    } else {
        m = n;
        if (s.count) {
            const long long c = s.count[0];
            m = c < 0 ? 0 : (c < n ? c : n);
        }
    }
    if (threadIdx.x == 0) {
        const long long total = state[0];
        work[n] = total;
        work[n + 1] = m;
        state[0] = total + m;
        state[1] = total + m < capacity ? total + m : capacity;
    }
}

__global__ __launch_bounds__(256) void k_replay_copy(ReplaySrc s, long long capacity, float *__restrict__ ring, const long long *__restrict__ work) {
    const int lane = threadIdx.x % REPLAY_LANES;
    const long long row = (long long)blockIdx.x * (256 / REPLAY_LANES) + threadIdx.x / REPLAY_LANES;
    if (row >= s.n) return;
    const long long head = work[s.n], m = work[s.n + 1];
    const long long k = (s.mask || s.packed) ? work[row] : (row < m ? row : -1);
    if (k < 0 || k < m - capacity) return;
    const int D = s.D, A = s.A, W = 2 * D + A + 4;
    float *dst = ring + (size_t)((head + k) % capacity) * W;
    if (s.packed) {
        const float *src = s.packed + (size_t)row * W;
        for (int i = lane; i < W; i += REPLAY_LANES) dst[i] = (i == D + A + 3) ? 0.0f : src[i];
        return;
    }
    for (int i = lane; i < W; i += REPLAY_LANES) {
        float v;
        if (i < D) v = (float)s.ob[row * D + i];
        else if (i < D + A) v = (float)s.ac[row * s.ac_ld + (i - D)];
        else if (i == D + A) v = (float)s.rew[row];
        else if (i == D + A + 1) v = (float)s.done[row];
        else if (i == D + A + 2) v = s.intra64 ? (float)((const long long *)s.intra)[row] : (float)((const int *)s.intra)[row];
        else if (i == D + A + 3) v = s.ac_type ? (float)s.ac_type[row] : 0.0f;
        else v = (float)s.ob_next[row * D + (i - D - A - 4)];
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_replay_sample(const uint32_t *__restrict__ ring, const long long *__restrict__ state, long long capacity, int W, long long rows,
                                                      unsigned long long key, unsigned long long draw_base, uint32_t *__restrict__ out,
                                                      long long *__restrict__ out_idx) {
    const int lane = threadIdx.x % REPLAY_LANES;
    const long long r = (long long)blockIdx.x * (256 / REPLAY_LANES) + threadIdx.x / REPLAY_LANES;
    if (r >= rows) return;
    const long long size = state[1] < capacity ? state[1] : capacity;      // (never beyond the ring, whatever a loaded state says)
    uint32_t *dst = out + (size_t)r * W;
    if (size <= 0) {
        for (int i = lane; i < W; i += REPLAY_LANES) dst[i] = 0u;
        if (lane == 0) out_idx[r] = -1;
        return;
    }
    // randint(0, size) = min(int(u * size), size - 1), as mopa_reuse.inc draws
    const double u = rng_uniform_k(key, draw_base + (unsigned long long)r);
    long long idx = (long long)(u * (double)size);
    idx = idx < size - 1 ? idx : size - 1;
    const uint32_t *src = ring + (size_t)idx * W;
    for (int i = lane; i < W; i += REPLAY_LANES) dst[i] = src[i];
    if (lane == 0) out_idx[r] = idx;
}

static int replay_shape_check(const char *who, int64_t capacity, int32_t D, int32_t A) {
    if (capacity < 1) return fail(MOPA_ERR_INVALID_ARG, std::string(who) + ": capacity < 1");
    if (D < 1) return fail(MOPA_ERR_INVALID_ARG, std::string(who) + ": D < 1");
    if (A < 1) return fail(MOPA_ERR_INVALID_ARG, std::string(who) + ": A < 1");
    if (D > (1 << 24) || A > (1 << 24) || capacity > 0x7fffffffffffLL / (2 * (int64_t)D + A + 4))
        return fail(MOPA_ERR_INVALID_ARG, std::string(who) + ": ring too large (D, A <= 2^24, capacity * W < 2^47)");
    return MOPA_OK;
}

extern "C" int mopa_replay_append(int64_t capacity, int32_t D, int32_t A, float *ring_dev, int64_t *state_dev, int64_t n,
                                  const uint8_t *mask_dev, const int64_t *count_dev, const double *ob_dev, const double *ac_dev, int32_t ac_ld,
                                  const double *rew_dev, const uint8_t *done_dev, const void *intra_dev, int32_t intra_is_int64,
                                  const double *ob_next_dev, const int32_t *ac_type_dev, const float *packed_dev, int64_t *work_dev, void *stream) {
    if (const int rc = replay_shape_check("replay append", capacity, D, A)) return rc;
    if (n < 0 || n > 0x7fffffffLL) return fail(MOPA_ERR_INVALID_ARG, "replay append: n < 0 (or above 2^31 - 1)");
    if (mask_dev && count_dev) return fail(MOPA_ERR_INVALID_ARG, "replay append: both a mask and a count");
    if (!ring_dev || !state_dev || !work_dev) return fail(MOPA_ERR_INVALID_ARG, "replay append: null buffer (ring, state, work)");
    if (packed_dev) {
        if (mask_dev || count_dev) return fail(MOPA_ERR_INVALID_ARG, "replay append: a packed source is masked by its stepped column: no mask, no count");
        if (ob_dev || ac_dev || rew_dev || done_dev || intra_dev || ob_next_dev || ac_type_dev)
            return fail(MOPA_ERR_INVALID_ARG, "replay append: both a packed source and columns");
    } else {
        if (!ob_dev || !ac_dev || !rew_dev || !done_dev || !intra_dev || !ob_next_dev) return fail(MOPA_ERR_INVALID_ARG, "replay append: null source column");
        if (ac_ld < A) return fail(MOPA_ERR_INVALID_ARG, "replay append: ac_ld < A");
    }
    if (n == 0) return MOPA_OK;
    ReplaySrc s;
    s.n = n; s.D = D; s.A = A; s.ac_ld = ac_ld; s.intra64 = intra_is_int64 != 0;
    s.mask = mask_dev; s.count = (const long long *)count_dev;
    s.ob = ob_dev; s.ac = ac_dev; s.rew = rew_dev; s.ob_next = ob_next_dev; s.done = done_dev; s.intra = intra_dev; s.ac_type = ac_type_dev;
    s.packed = packed_dev;
    const hipStream_t st = (hipStream_t)stream;
    const int per = 256 / REPLAY_LANES;
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, st, s, (long long)capacity, (long long *)state_dev, (long long *)work_dev);
    hipLaunchKernelGGL(k_replay_copy, dim3((unsigned)((n + per - 1) / per)), dim3(256), 0, st, s, (long long)capacity, ring_dev, (const long long *)work_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_replay_sample(int64_t capacity, int32_t D, int32_t A, const float *ring_dev, const int64_t *state_dev, int64_t B, int64_t n_batches,
                                  uint64_t seed, uint64_t stream_id, uint64_t draw_base, float *out_dev, int64_t *out_idx_dev, void *stream) {
    if (const int rc = replay_shape_check("replay sample", capacity, D, A)) return rc;
    if (B < 1) return fail(MOPA_ERR_INVALID_ARG, "replay sample: B < 1");
    if (n_batches < 1) return fail(MOPA_ERR_INVALID_ARG, "replay sample: n_batches < 1");
    if (B > 0x7fffffffLL || n_batches > 0x7fffffffLL || B * n_batches > 0x7fffffffLL)
        return fail(MOPA_ERR_INVALID_ARG, "replay sample: B * n_batches above 2^31 - 1");
    if (!ring_dev || !state_dev || !out_dev || !out_idx_dev) return fail(MOPA_ERR_INVALID_ARG, "replay sample: null buffer");
    const long long rows = B * n_batches;
    const int per = 256 / REPLAY_LANES;
    hipLaunchKernelGGL(k_replay_sample, dim3((unsigned)((rows + per - 1) / per)), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)ring_dev,
                       (const long long *)state_dev, (long long)capacity, 2 * D + A + 4, rows, (unsigned long long)rng_key(seed, stream_id), (unsigned long long)draw_base,
                       (uint32_t *)out_dev, (long long *)out_idx_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
