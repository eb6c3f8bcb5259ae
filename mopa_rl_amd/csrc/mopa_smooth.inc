// mopa_smooth.inc -- K9: smoothBSpline between shortcutPath and the vertex-reducing passes, one wave per path.
// (included by mopa_hip.hip behind mopa_shortcut.inc, whose kernel body k_smooth_paths instantiates with SMOOTH = true:
// k_shortcut_paths is the same body with SMOOTH = false and keeps its code)
//
// OMPL's PathSimplifier::smoothBSpline restated (DESIGN.md "K9 path simplification: smoothBSpline"; the sequential form is
// tests/smooth_ref.py, which the result has to equal bit for bit): up to three steps, each of which puts a vertex into the middle
// of every segment and then pulls every old interior vertex towards the middle of its two new neighbours when the two motions
// that creates pass K2's rule and the vertex moves by more than a hundredth of the path's length.  Three deviations keep every
// segment of a result one that has itself passed the motion check, so that there is nothing for checkAndRepair to do: a vertex
// moves only if the outer halves of its two old segments pass too, a step in which nothing moves is undone, and a midpoint
// between two vertices that stayed is kept only if both its halves pass.  No row is ever taken back once it is written, so the
// rows stay in the path's own max_path slots: subdivision pops free slots, a move overwrites its row's active entries, dropped
// midpoints push their slots back.  The state checks of the midpoints in front of the candidates do not depend on one another
// and run kMS = 4 states per validity pass (plan_states_valid_ms, the planner's routine); every motion check goes through
// plan_state_valid_impl as in k_shortcut_paths.  Counters are wave-uniform scalars.  No atomics, no read-back.

// per wave: k_shortcut_paths' lists, then the verdict bytes and moved bits (smooth_flag_bytes), then the validity pass' slabs
static int smooth_list_bytes(const MopaScene *S, int max_path) {
    return shortcut_list_bytes(S->na, S->nq, max_path) + smooth_flag_bytes(max_path) +
           ms_bytes_per_wave(S->hdr.nmg, S->na, S->hdr.n_pq, ms_sc_doubles(S->hdr.nmj, S->hdr.nmb), S->hdr.npair);
}
static int smooth_lds_bytes(const MopaScene *S, int max_path) {
    return ((S->lds_bytes + 15) & ~15) + (((int)sizeof(SceneHdr) + 15) & ~15) + kWavesPerBlock * smooth_list_bytes(S, max_path);
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_smooth_paths(SceneHdr h, const double *__restrict__ g_dbl,
                                                                                                   const int32_t *__restrict__ g_int, ShortcutArgs a) {
    shortcut_paths_body<true>(h, g_dbl, g_int, a);
}

static void smooth_register_lds() {
    (void)hipFuncSetAttribute((const void *)k_smooth_paths, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
}

extern "C" int mopa_smooth_paths_max_path(const MopaScene *S) {
    if (!S) return -1;
    // a row costs a wave 16 bytes of lists, a verdict byte and a moved bit; the three paddings stay below 4 rows' worth
    int mp = (kMaxLdsBytes - smooth_lds_bytes(S, 0)) / (18 * kWavesPerBlock) - 4;
    return std::max(0, std::min(mp, 65535));        // (16-bit slots)
}

extern "C" int mopa_smooth_paths_batch(MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev,
                                       const int32_t *status_dev, uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev,
                                       const uint64_t *seeds_dev, int32_t passes, int32_t max_rounds, int64_t *info_dev, void *stream) {
    if (!S || (E > 0 && (!path_dev || !path_len_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E < 0 || max_path < 2 || passes < 1 || passes > 15 || max_rounds < 1)
        return fail(MOPA_ERR_INVALID_ARG, "E < 0, max_path < 2, passes outside 1..15 or max_rounds < 1");
    if (max_path > mopa_smooth_paths_max_path(S) || smooth_lds_bytes(S, max_path) > kMaxLdsBytes)
        return fail(MOPA_ERR_UNSUPPORTED, "path smoothing: max_path beyond what the per-wave LDS lists hold (" +
                                              std::to_string(mopa_smooth_paths_max_path(S)) + ")");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    ShortcutArgs a;
    a.path = path_dev; a.path_len = path_len_dev; a.status = status_dev; a.E = (long long)E; a.max_path = max_path; a.passes = passes;
    a.max_rounds = max_rounds; a.seed = seed; a.env_id_base = env_id_base;
    a.env_ids = reinterpret_cast<const unsigned long long *>(env_ids_dev); a.seeds = reinterpret_cast<const unsigned long long *>(seeds_dev);
    a.info = reinterpret_cast<long long *>(info_dev);
    a.hdr_lds_off = (S->lds_bytes + 15) & ~15;
    a.list_lds_off = a.hdr_lds_off + (((int)sizeof(SceneHdr) + 15) & ~15);
    a.list_bytes = smooth_list_bytes(S, max_path);
    hipLaunchKernelGGL(k_smooth_paths, dim3(grid_for(S, E)), dim3(kBlock), smooth_lds_bytes(S, max_path), (hipStream_t)stream, S->hdr, S->d_dbl,
                       S->d_int, a);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
