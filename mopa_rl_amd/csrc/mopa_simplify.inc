// mopa_simplify.inc -- K9: vertex-reducing path simplification, one wave per path.
// (included by mopa_hip.hip behind mopa_check_motion_batch: the kernel has the shape of k_check_motion)
//
// OMPL's PathSimplifier::reduceVertices and collapseCloseVertices restated (DESIGN.md "K9 path simplification"): both only
// REMOVE waypoints, so the result is a subset of the planner's rows and is required identical to the sequential form of
// tests/simplify_ref.py.  Every decision is taken from wave-uniform values: the list of surviving row indices (16-bit) and the
// pairs collapseCloseVertices has found blocked live in the wave's LDS, the counters in scalar registers; the rows themselves are
// only read until the final compaction.  A motion check is k_check_motion's loop over the two endpoint rows' active entries
// gathered into LDS, with path row 0 as the env row.  No atomics.  shortcutPath, the B-spline pass and checkAndRepair are not
// built.

struct SimplifyArgs {
    double *path;                       // [E, max_path, nq] in/out
    int32_t *path_len;                  // [E] in/out
    const int32_t *status;              // [E] nullable
    long long E;
    int max_path, passes;
    unsigned long long seed, env_id_base;
    const unsigned long long *env_ids, *seeds;      // nullable, as in MopaPlanParams
    long long *info;                    // [E, 2] nullable: motion checks made, draws consumed
    int hdr_lds_off, list_lds_off, list_bytes;      // LDS: SceneHdr copy, the waves' lists, bytes of one wave's lists
};

// per wave behind the header copy: [2 * na doubles: the endpoints of the check][max_path words: blocked pairs][max_path halves: surviving rows]
static int simplify_list_bytes(int na, int max_path) { return (16 * na + 4 * max_path + 2 * max_path + 15) & ~15; }
static int simplify_lds_bytes(const MopaScene *S, int max_path) {
    return ((S->lds_bytes + 15) & ~15) + (((int)sizeof(SceneHdr) + 15) & ~15) + kWavesPerBlock * simplify_list_bytes(S->na, max_path);
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_simplify_paths(SceneHdr h, const double *__restrict__ g_dbl,
                                                                                                     const int32_t *__restrict__ g_int, SimplifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + a.hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int na = h.na, nq = h.nq;
    unsigned char *lbase = smem + a.list_lds_off + wave * a.list_bytes;
    double *ends = reinterpret_cast<double *>(lbase);                                   // [2][na]
    unsigned *blocked = reinterpret_cast<unsigned *>(ends + 2 * na);                    // [max_path]: original row i << 16 | original row j
    unsigned short *idx = reinterpret_cast<unsigned short *>(blocked + a.max_path);     // [max_path]: surviving rows, ascending
    double *tst = v.qbuf + na + h.n_pq;                                                 // spare [na] doubles behind the joint-value buffer
    const int *adr = v.ints + h.o_act_adr;
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long e = (long long)blockIdx.x * kWavesPerBlock + wave; e < a.E; e += stride) {
        const int n_in = a.path_len[e];
        if ((a.status && a.status[e] != 0) || n_in < 3 || n_in > a.max_path) continue;       // skipped: nothing of it is touched
        double *pe = a.path + (size_t)e * a.max_path * nq;
        const unsigned long long key = rng_key(a.seeds ? a.seeds[e] : a.seed, a.env_ids ? a.env_ids[e] : a.env_id_base + (unsigned long long)e);
        for (int i = lane; i < n_in; i += 64) idx[i] = (unsigned short)i;
        wave_sync();
        int cnt = n_in;
        long long n_checks = 0, n_draws = 0;

        auto survivor = [&](int k) -> int { return __builtin_amdgcn_readfirstlane((int)idx[k]); };
        // K2's rule between the surviving vertices ia < ib
        auto check = [&](int ia, int ib) -> bool {
            const double *ra = pe + (size_t)survivor(ia) * nq, *rb = pe + (size_t)survivor(ib) * nq;
            for (int i = lane; i < na; i += 64) { ends[i] = ra[adr[i]]; ends[na + i] = rb[adr[i]]; }
            wave_sync();
            n_checks++;
            const int nd = __builtin_amdgcn_readfirstlane(valid_segment_count(h, v, ends, ends + na));
            bool ok = true;
            for (int k = nd; k >= (nd > 0 ? 1 : 0) && ok; k--) {
                const double t = (nd > 0) ? (double)k / (double)nd : 1.0;
                for (int i = lane; i < na; i += 64) tst[i] = (k == nd) ? ends[na + i] : interp_dim(h, v, i, ends[i], ends[na + i], t);
                wave_sync();
                ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, pe);
            }
            return ok;
        };
        // erase the survivors strictly between ia and ib (64 entries at a time: a chunk's targets lie below the next chunk's sources)
        auto erase = [&](int ia, int ib) {
            const int gap = ib - ia - 1;
            for (int base = ib; base < cnt; base += 64) {
                const int s = base + lane;
                const unsigned short val = s < cnt ? idx[s] : (unsigned short)0;
                wave_sync();
                if (s < cnt) idx[s - gap] = val;
                wave_sync();
            }
            cnt -= gap;
        };
        auto uniform_int = [&](int lo, int hi) -> int {
            const int m = hi - lo + 1;
            const double u = rng_uniform_k(key, 0x8000000000000000ull + (unsigned long long)n_draws);
            n_draws++;
            const int r = (int)(u * (double)m);
            return lo + (r < m - 1 ? r : m - 1);
        };
        auto reduce = [&]() -> bool {
            const int n = cnt;
            if (!(a.passes & 1) || n < 3) return false;
            if (check(0, cnt - 1)) {
                if (lane == 0) idx[1] = idx[cnt - 1];
                wave_sync();
                cnt = 2;
                return true;
            }
            bool result = false;
            int nochange = 0;
            for (int i = 0; i < n && nochange < n; i++, nochange++) {
                const int count = cnt, max_n = count - 1;
                const int range = 1 + (33 * count + 50) / 100;
                int p1 = uniform_int(0, max_n);
                int p2 = uniform_int(p1 - range > 0 ? p1 - range : 0, max_n < p1 + range ? max_n : p1 + range);
                if ((p1 > p2 ? p1 - p2 : p2 - p1) < 2) {
                    if (p1 < max_n - 1) p2 = p1 + 2;
                    else if (p1 > 1) p2 = p1 - 2;
                    else continue;
                }
                if (p1 > p2) { const int t = p1; p1 = p2; p2 = t; }
                p1 = __builtin_amdgcn_readfirstlane(p1);
                p2 = __builtin_amdgcn_readfirstlane(p2);
                if (check(p1, p2)) {
                    erase(p1, p2);
                    nochange = 0;
                    result = true;
                }
            }
            return result;
        };
        auto collapse = [&]() {
            const int n = cnt;
            if (!(a.passes & 2) || n < 3) return;
            int n_blocked = 0, nochange = 0;
            for (int s = 0; s < n && nochange < n; s++, nochange++) {
                // the closest pair (i, j >= i + 2) that is not blocked; a lane scans its j in ascending (i, j) order with a strict <,
                // then the lanes' candidates are merged by (distance, i, j): the first minimum of the ascending scan
                double best = __builtin_inf();
                unsigned best_ij = 0xffffffffu;
                for (int i = 0; i + 2 < cnt; i++) {
                    const unsigned oi = (unsigned)survivor(i);
                    const double *ri = pe + (size_t)oi * nq;
                    for (int j = i + 2 + lane; j < cnt; j += 64) {
                        const unsigned oj = idx[j];
                        const double *rj = pe + (size_t)oj * nq;
                        double d = 0.0;
                        for (int c = 0; c < na; c++) d += dist_dim(h, v, c, ri[adr[c]], rj[adr[c]]);
                        if (d < best) {
                            const unsigned keyij = (oi << 16) | oj;
                            bool is_blocked = false;
                            for (int b = 0; b < n_blocked; b++) is_blocked |= blocked[b] == keyij;
                            if (!is_blocked) { best = d; best_ij = ((unsigned)i << 16) | (unsigned)j; }
                        }
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double od = __shfl_xor(best, off, 64);
                    const unsigned oij = (unsigned)__shfl_xor((int)best_ij, off, 64);
                    if (od < best || (od == best && oij < best_ij)) { best = od; best_ij = oij; }
                }
                best_ij = (unsigned)__builtin_amdgcn_readfirstlane((int)best_ij);
                if (best_ij == 0xffffffffu) break;
                const int bi = (int)(best_ij >> 16), bj = (int)(best_ij & 0xffffu);
                if (check(bi, bj)) {
                    erase(bi, bj);
                    nochange = 0;
                } else {
                    if (lane == 0) blocked[n_blocked] = ((unsigned)idx[bi] << 16) | (unsigned)idx[bj];
                    n_blocked++;       // (at most one per iteration, at most n <= max_path iterations)
                    wave_sync();
                }
            }
        };

        // the non-metric-space part of PathSimplifier::simplify's loop, without its wall-clock condition
        bool try_more = true;
        while (try_more) {
            try_more = reduce();
            collapse();
            for (int times = 0; try_more && times < 5; times++) try_more = reduce();
        }

        // compaction in place, ascending (target row <= source row; row 0 never moves)
        for (int k = 1; k < cnt; k++) {
            const int src = survivor(k);
            if (src != k)
                for (int i = lane; i < nq; i += 64) pe[(size_t)k * nq + i] = pe[(size_t)src * nq + i];
        }
        if (lane == 0) {
            a.path_len[e] = cnt;
            if (a.info) { a.info[2 * e] = n_checks; a.info[2 * e + 1] = n_draws; }
        }
        wave_sync();
    }
}

static void simplify_register_lds() {
    (void)hipFuncSetAttribute((const void *)k_simplify_paths, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
}

extern "C" int mopa_simplify_paths_max_path(const MopaScene *S) {
    if (!S) return -1;
    int mp = (kMaxLdsBytes - simplify_lds_bytes(S, 0)) / (6 * kWavesPerBlock) - 4;
    return std::max(0, std::min(mp, 65535));        // (16-bit row indices)
}

extern "C" int mopa_simplify_paths_batch(MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev,
                                         const int32_t *status_dev, uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev,
                                         const uint64_t *seeds_dev, int32_t passes, int64_t *info_dev, void *stream) {
    if (!S || (E > 0 && (!path_dev || !path_len_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E < 0 || max_path < 2 || passes < 1 || passes > 3) return fail(MOPA_ERR_INVALID_ARG, "E < 0, max_path < 2 or passes outside 1..3");
    if (max_path > mopa_simplify_paths_max_path(S))
        return fail(MOPA_ERR_UNSUPPORTED, "path simplification: max_path beyond what the per-wave LDS lists hold (" +
                                              std::to_string(mopa_simplify_paths_max_path(S)) + ")");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    SimplifyArgs a;
    a.path = path_dev; a.path_len = path_len_dev; a.status = status_dev; a.E = (long long)E; a.max_path = max_path; a.passes = passes;
    a.seed = seed; a.env_id_base = env_id_base;
    a.env_ids = reinterpret_cast<const unsigned long long *>(env_ids_dev); a.seeds = reinterpret_cast<const unsigned long long *>(seeds_dev);
    a.info = reinterpret_cast<long long *>(info_dev);
    a.hdr_lds_off = (S->lds_bytes + 15) & ~15;
    a.list_lds_off = a.hdr_lds_off + (((int)sizeof(SceneHdr) + 15) & ~15);
    a.list_bytes = simplify_list_bytes(S->na, max_path);
    hipLaunchKernelGGL(k_simplify_paths, dim3(grid_for(S, E)), dim3(kBlock), simplify_lds_bytes(S, max_path), (hipStream_t)stream, S->hdr, S->d_dbl,
                       S->d_int, a);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
