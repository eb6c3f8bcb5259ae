// mopa_pullback.inc -- the rollout's invalid-target back-off as one launch (SURVEY 8f row 2).
// (included at the end of mopa_hip.hip)
//
// Reference: rl/mopa_rollouts.py:133-143 -- while the planner target is invalid and fewer than num_trials steps were
// taken: target += step_size * (cur - target) / ||cur - target||  (Euclidean norm over the FULL qpos vector).
// One wave per env; the norm's squares are summed left to right (the order the host form shares), every validity test is
// on the target's own qpos row.  The sequence of candidate targets does not depend on the verdicts -- only where it stops
// does -- so the next kMS candidates are generated ahead (each from its predecessor, same arithmetic) and validated in ONE
// multi-state pass (plan_states_valid_ms, the planner's routine): a quarter of the sequential passes.  That routine takes
// one row of passive values for all its states, which is what a back-off has when target and current state agree on the
// passive coordinates (they then stay equal: the step of such a coordinate is exactly 0); otherwise the kernel falls
// back to one state per pass.
// (two waves per SIMD: the non-inlined validity routines then save ~40 registers to scratch around every call, and it still pays:
//  wave-per-env pull-back 1.00 -> 0.81 ms per 3000 targets, wave-per-segment motion checks 46 -> 83 M motions/s)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pullback(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                     const double *__restrict__ cur, double *__restrict__ target, long long E,
                                                     double step_size, int num_trials, int32_t *__restrict__ n_trials,
                                                     unsigned char *__restrict__ valid, int extra_lds_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + extra_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long e = (long long)blockIdx.x * kWavesPerBlock + wave;
    if (e >= E) return;
    const int nq = h.nq, na = h.na;
    // per wave: the target row [nq], its active coordinates [na], then the multi-state slabs
    const int row_bytes = ((nq + na) * 8 + 15) & ~15;
    const int ms_bytes = ms_bytes_per_wave(h.nmg, na, h.n_pq, ms_sc_doubles(h.nmj, h.nmb), h.npair);
    unsigned char *wbase = smem + extra_lds_off + ((sizeof(SceneHdr) + 15) & ~15) + (size_t)wave * (row_bytes + ms_bytes);
    double *tq = reinterpret_cast<double *>(wbase);
    double *ta = tq + nq;
    MsLds ms;
    ms.grec = reinterpret_cast<double *>(wbase + row_bytes);
    ms.qbuf = ms.grec + kMS * h.nmg * kGeomStride;
    ms.qs = ms.qbuf + kMS * (na + h.n_pq + ms_sc_doubles(h.nmj, h.nmb));
    ms.wl = reinterpret_cast<unsigned *>(ms.qs + kMS * na);
    const double *c = cur + e * nq;
    double *tg = target + e * nq;
    for (int i = lane; i < nq; i += 64) tq[i] = tg[i];
    wave_sync();
    for (int i = lane; i < na; i += 64) ta[i] = tq[v.ints[h.o_act_adr + i]];
    wave_sync();
    // do target and current state agree on every passive coordinate?
    bool same = true;
    for (int i = lane; i < h.n_pq; i += 64) {
        const int adr = v.ints[h.o_pq_adr + i];
        same = same && (__double_as_longlong(c[adr]) == __double_as_longlong(tq[adr]));
    }
    // (a target identical to the current state has no direction to move in: 0 / 0 -- left to the one-state loop)
    bool moves = false;
    for (int i = lane; i < na; i += 64) {
        const int adr = v.ints[h.o_act_adr + i];
        moves = moves || (c[adr] - tq[adr] != 0.0);
    }
    const bool multi = __all(same) && __any(moves);
    bool ok = false;
    int trials = 0;
    if (multi) {
        // slot 0 of the first pass is the target itself (trial 0); the other slots are the candidates that follow
        bool first = true;
        for (;;) {
            int ns = 0;
            if (first) {
                if (lane < na) ms.qs[lane] = ta[lane];
                ns = 1;
            }
            const int base_trials = trials + (first ? 0 : 0);
            int gen = 0;
            while (ns < kMS && trials + gen < num_trials) {
                double acc = 0.0;
                for (int i = 0; i < nq; i++) {       // every lane the same sequential sum
                    const double d = c[i] - tq[i];
                    acc = acc + d * d;
                }
                const double nrm = sqrt(acc);
                wave_sync();
                for (int i = lane; i < nq; i += 64) {
                    const double d = c[i] - tq[i];
                    tq[i] = tq[i] + (step_size * d) / nrm;
                }
                wave_sync();
                if (lane < na) ms.qs[ns * na + lane] = tq[v.ints[h.o_act_adr + lane]];
                ns++; gen++;
                wave_sync();
            }
            if (ns == 0) break;                       // trial budget exhausted, still invalid
            wave_sync();
            const unsigned okm = plan_states_valid_ms(lh, v.dbl, v.ints, ms.grec, ms.qbuf, ms.wl, ms.qs, lane, ns, c);
            if (okm) {
                const int s = __ffs(okm) - 1;         // the first valid state of the pass ends the back-off
                trials = base_trials + s + (first ? 0 : 1);
                // rewind the row to that candidate: only active coordinates ever change
                if (lane < na) tq[v.ints[h.o_act_adr + lane]] = ms.qs[s * na + lane];
                ok = true;
                break;
            }
            trials += gen;
            first = false;
            if (trials >= num_trials) break;
        }
        wave_sync();
    } else {
        ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, ta, tq);
        while (!ok && trials < num_trials) {
            double acc = 0.0;
            for (int i = 0; i < nq; i++) {       // every lane the same sequential sum
                const double d = c[i] - tq[i];
                acc = acc + d * d;
            }
            const double nrm = sqrt(acc);
            wave_sync();
            for (int i = lane; i < nq; i += 64) {
                const double d = c[i] - tq[i];
                tq[i] = tq[i] + (step_size * d) / nrm;
            }
            wave_sync();
            for (int i = lane; i < na; i += 64) ta[i] = tq[v.ints[h.o_act_adr + i]];
            wave_sync();
            trials++;
            ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, ta, tq);
        }
    }
    // (a target that was valid as it came is left exactly as it came: the candidates generated ahead of its verdict have
    // touched the row -- e.g. a passive -0.0 becomes +0.0 after one step, as in the reference once it does step)
    if (!(ok && trials == 0))
        for (int i = lane; i < nq; i += 64) tg[i] = tq[i];
    if (lane == 0) {
        n_trials[e] = trials;
        valid[e] = ok ? 1 : 0;
    }
}

// ---- the throughput form: candidates for all invalid targets at once, one lane-per-state validity launch ----
// k_pullback above walks one env per wave: an env that needs many steps costs that many dependent validity passes (a
// 100-step back-off: 25 passes of ~35 us), and the launch lasts as long as its slowest env.  The sequence of candidate
// targets does not depend on any verdict, so here every invalid target's WHOLE sequence (num_trials rows) is generated
// first (one lane per env, the same arithmetic step by step), all rows are validated by the lane-per-state kernel K1 in
// one launch, and the first valid row of each env is picked.  More states are checked than the sequential loop would
// (it stops at the first valid one) -- K1 does them at >1 G/s -- and the outcome is the same row, count and verdict.
__global__ void k_pb_active(const SceneHdr h, const int32_t *__restrict__ g_int, const double *__restrict__ rows, long long n,
                            double *__restrict__ qa, const long long *__restrict__ n_dev, unsigned int *__restrict__ zero4 /* nullable */) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (zero4 && i < 4) zero4[i] = 0u;       // the slot counter of the launches that follow (saves its own zeroing launch)
    if (n_dev && *n_dev < n) n = *n_dev;
    if (i >= n * h.na) return;
    const long long r = i / h.na;
    const int a = (int)(i - r * h.na);
    qa[i] = rows[r * h.nq + g_int[h.o_act_adr + a]];
}
// invalid targets get a slot (arrival order); the valid ones are finished: 0 steps taken
__global__ void k_pb_slots(const unsigned char *__restrict__ valid0, long long E, int num_trials, unsigned int *__restrict__ ctr,
                           int32_t *__restrict__ slot_env, int32_t *__restrict__ n_trials, unsigned char *__restrict__ valid) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    if (valid0[e] || num_trials == 0) {
        n_trials[e] = 0;
        valid[e] = valid0[e];
        return;
    }
    slot_env[atomicAdd(ctr, 1u)] = (int32_t)e;
}
// one wave per invalid target, one lane per qpos coordinate (nq <= 64): the running row stays in registers, the norm's squares
// are summed left to right by broadcasting them lane by lane (v_readlane), every coordinate takes its step at once
__global__ __launch_bounds__(kBlock) void k_pb_gen(int nq, const double *__restrict__ cur, const double *__restrict__ target,
                                                   const unsigned int *__restrict__ ctr, double step_size, int num_trials,
                                                   const int32_t *__restrict__ slot_env, double *__restrict__ cand,
                                                   long long *__restrict__ n_rows) {
    const int lane = threadIdx.x & 63;
    const unsigned slot = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const unsigned n_inv = *ctr;            // final: k_pb_slots has finished
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_rows = (long long)n_inv * num_trials;
    if (slot >= n_inv) return;
    const long long e = slot_env[slot];
    const bool on = lane < nq;
    const double c = on ? cur[e * nq + lane] : 0.0;
    double r = on ? target[e * nq + lane] : 0.0;
    double *next = cand + (size_t)slot * num_trials * nq;
    // (a coordinate whose target equals its current value never moves: d = 0 in every trial, its square adds an exact +0.0 to the running sum.
    //  Of a rollout's qpos row only the arm's entries differ -- 7 of Push's 18 --, so the sum walks the set bits of this mask, still left to
    //  right: the same bits, 100 trials of a 7-term instead of an 18-term dependent chain: 156 -> ~60 us per call of 4096 envs)
    const unsigned long long nz = __ballot(on && (c - r) != 0.0);
    for (int j = 0; j < num_trials; j++) {
        const double d = c - r;
        const double sq = d * d;
        const int lo = __double2loint(sq), hi = __double2hiint(sq);
        double acc = 0.0;
        for (unsigned long long m = nz; m; m &= m - 1ull) {
            const int i = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m));
            acc = acc + __hiloint2double(__builtin_amdgcn_readlane(hi, i), __builtin_amdgcn_readlane(lo, i));
        }
        const double nrm = sqrt(acc);
        r = r + (step_size * d) / nrm;
        if (on) next[lane] = r;
        next += nq;
    }
}
// one WAVE per invalid target: the first valid candidate by a ballot over 64 candidates at a time (one thread walking its 100 verdict bytes one
// dependent load after the other took 22 us), the chosen row copied one coordinate per lane
__global__ __launch_bounds__(kBlock) void k_pb_pick(int nq, double *__restrict__ target, int num_trials, const unsigned int *__restrict__ ctr,
                                                    const int32_t *__restrict__ slot_env, const double *__restrict__ cand,
                                                    const unsigned char *__restrict__ cand_valid, int32_t *__restrict__ n_trials,
                                                    unsigned char *__restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const unsigned slot = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (slot >= *ctr) return;
    const int e = slot_env[slot];
    const unsigned char *cv = cand_valid + (size_t)slot * num_trials;
    int j = num_trials;
    for (int base = 0; base < num_trials; base += 64) {
        const int idx = base + lane;
        const unsigned long long m = __ballot(idx < num_trials && cv[idx] != 0);
        if (m) { j = base + (int)__builtin_ctzll(m); break; }
    }
    const bool ok = j < num_trials;
    if (!ok) j = num_trials - 1;
    const double *row = cand + ((size_t)slot * num_trials + j) * nq;
    double *tg = target + (size_t)e * nq;
    for (int i = lane; i < nq; i += 64) tg[i] = row[i];
    if (lane == 0) {
        n_trials[e] = j + 1;
        valid[e] = ok ? 1 : 0;
    }
}

static int pullback_wave_per_env(MopaScene *S, const double *cur, double *target, int64_t E, double step_size, int num_trials,
                                 int32_t *n_trials, uint8_t *valid, void *stream) {
    const int off = (S->lds_bytes + 15) & ~15;
    const int lds = off + (((int)sizeof(SceneHdr) + 15) & ~15) +
                    kWavesPerBlock * ((((S->nq + S->na) * (int)sizeof(double) + 15) & ~15) +
                                      ms_bytes_per_wave(S->hdr.nmg, S->na, S->hdr.n_pq, ms_sc_doubles(S->hdr.nmj, S->hdr.nmb), S->hdr.npair));
    if (lds > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "pull-back LDS does not fit");
    dim3 grid((unsigned)((E + kWavesPerBlock - 1) / kWavesPerBlock)), block(kBlock);
    hipLaunchKernelGGL(k_pullback, grid, block, lds, (hipStream_t)stream, S->hdr, S->d_dbl, S->d_int, cur, target, (long long)E,
                       step_size, num_trials, n_trials, valid, off);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_pullback_batch(MopaScene *S, const double *cur, double *target, int64_t E, double step_size, int num_trials,
                                   int32_t *n_trials, uint8_t *valid, void *stream) {
    if (!S || (E > 0 && (!cur || !target || !n_trials || !valid))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E < 0 || num_trials < 0) return fail(MOPA_ERR_INVALID_ARG, "bad pull-back parameters");
    MOPA_REFUSE_GLUED(S, "the pull-back (mopa_pullback_batch)");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    // few envs: the wave-per-env walk (no read-back); MOPA_PULLBACK=wave|batch pins the form for A/B runs and tests
    const char *force = getenv("MOPA_PULLBACK");
    const bool batch = force ? std::strcmp(force, "batch") == 0 : E >= 256;
    if (!batch || !S->k1.use_v2 || S->nq > 64) return pullback_wave_per_env(S, cur, target, E, step_size, num_trials, n_trials, valid, stream);
    StreamScratch &sc = scratch_for(S, st);
    const int nq = S->nq, na = S->na;
    // 1. verdicts of the targets as they come
    HIP_TRY(grow(S, sc.pb_small, (size_t)E * (na * sizeof(double) + sizeof(int32_t) + 1) + 64));
    unsigned int *ctr = sc.pb_small.as<unsigned int>();
    double *qa0 = reinterpret_cast<double *>(sc.pb_small.as<unsigned char>() + 64);
    int32_t *slot_env = reinterpret_cast<int32_t *>(qa0 + (size_t)E * na);
    unsigned char *valid0 = reinterpret_cast<unsigned char *>(slot_env + E);
    hipLaunchKernelGGL(k_pb_active, dim3((unsigned)((E * na + 255) / 256)), dim3(256), 0, st, S->hdr, S->d_int, target, (long long)E, qa0,
                       (const long long *)nullptr, ctr);
    int rc = launch_is_valid(S, qa0, target, E, 1, nullptr, valid0, nullptr, stream);
    if (rc != MOPA_OK) return rc;
    // 2. the whole candidate sequence of every invalid target (rows are appended per invalid env: slot = arrival order).
    //    Their number stays on the device: the launches below are sized for the worst case (every target invalid) and read
    //    the count themselves (the validity launch through launch_is_valid's device-side count), so the call never waits
    //    for the GPU.  Only batches whose worst case would not be a sane allocation read the count back.
    hipLaunchKernelGGL(k_pb_slots, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, valid0, (long long)E, num_trials, ctr, slot_env,
                       n_trials, valid);
    if (num_trials == 0) return MOPA_OK;
    int64_t n_inv_max = E;
    const size_t row_bytes = (size_t)num_trials * (nq + na) * sizeof(double) + num_trials;
    if ((size_t)E * row_bytes > ((size_t)1 << 30) || !S->k1.use_v5) {
        unsigned int n_inv = 0;
        HIP_TRY(hipMemcpyAsync(&n_inv, ctr, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_inv == 0) return MOPA_OK;
        n_inv_max = n_inv;
    }
    HIP_TRY(grow(S, sc.pb_rows, (size_t)n_inv_max * num_trials * nq * sizeof(double)));
    HIP_TRY(grow(S, sc.pb_act, (size_t)n_inv_max * num_trials * (na * sizeof(double) + 1) + 16));
    double *cand = sc.pb_rows.as<double>();
    long long *n_rows_dev = reinterpret_cast<long long *>(ctr + 2);      // pb_small starts with 64 bytes of counters
    hipLaunchKernelGGL(k_pb_gen, dim3((unsigned)((n_inv_max + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, nq, cur, target, ctr,
                       step_size, num_trials, slot_env, cand, n_rows_dev);
    HIP_TRY(hipGetLastError());
    // 3. one validity launch over all candidate rows, 4. first valid row per env
    const int64_t n_rows = n_inv_max * num_trials;
    double *qa = sc.pb_act.as<double>();
    unsigned char *cand_valid = reinterpret_cast<unsigned char *>(qa + (size_t)n_rows * na);
    hipLaunchKernelGGL(k_pb_active, dim3((unsigned)((n_rows * na + 255) / 256)), dim3(256), 0, st, S->hdr, S->d_int, cand, (long long)n_rows, qa,
                       (const long long *)n_rows_dev, (unsigned int *)nullptr);
    rc = launch_is_valid(S, qa, cand, n_rows, 1, nullptr, cand_valid, nullptr, stream, S->k1.use_v5 ? n_rows_dev : nullptr);
    if (rc != MOPA_OK) return rc;
    hipLaunchKernelGGL(k_pb_pick, dim3((unsigned)((n_inv_max + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, nq, target, num_trials, ctr, slot_env, cand, cand_valid,
                       n_trials, valid);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

static const LdsKernels kPullbackLds({(const void *)k_pullback});
