// mopa_valid_launch.inc -- the host side of K1 (included by mopa_hip.hip behind mopa_scene_create): which validity kernels a
// batch gets and with what launch shape (k1_plan), the one table of K1 instantiations, and the launch itself.
// The scene's share of the policy (K1Policy: generations, centre placement, entry caps, LDS sizes) is filled by the scene
// compiler's last step (mopa_scene_build.inc: SceneBuild::k1_policy); everything decided per batch is decided in k1_plan.

// ---------------------------------------------------------------------------
// thresholds
// ---------------------------------------------------------------------------
// Kernel choice: the lane-per-state kernel needs ~175 us for a 64-state tile however few tiles there are, the
// wave-per-state kernel ~23 us per state-wave with 8+ waves per CU in flight -- so small batches (one state per
// env, e.g. the collision gate of the kinematic env.step) go to the latter.  Measured crossover on MI355X:
// 8192 states 155 vs 171 us, 12288 states 202 vs 168 us  =>  ~36 states per CU.
static int64_t k1_lane_min(const MopaScene *S) { return S->k1.v2_forced ? 64 : std::max<int64_t>(64, (int64_t)S->n_cu * 36); }
// motion validation: from this many segments on they are expanded into their states for the lane-per-state kernel (mopa_motion.inc)
static int64_t k1_motion_expand_min(const MopaScene *S) { return S->k1.v2_forced ? 64 : std::max<int64_t>(64, (int64_t)S->n_cu * 16); }

// ---------------------------------------------------------------------------
// the K1 instantiations: every one the library launches is in one of these tables (plus MOPA_K1_BAKED_SCENES), and
// k1_kernels walks their whole domain for the LDS list (mopa_hip.hip: LdsKernels)
// ---------------------------------------------------------------------------
using K1FnV1 = decltype(&k_is_valid<false, false>);
using K1FnV2 = decltype(&k_is_valid_v2<false, false>);
using K1FnV5 = decltype(&k_is_valid_v5<false, true, false>);
#define MOPA_K1_COUNT(i_, T_) +1
constexpr int kK1BakedScenes = 0 MOPA_K1_BAKED_SCENES(MOPA_K1_COUNT);
#undef MOPA_K1_COUNT

static K1FnV1 k1_kernel_v1(bool want_md, bool mesh) {
    static const K1FnV1 tab[2][2] = {{k_is_valid<false, false>, k_is_valid<true, false>}, {k_is_valid<false, true>, k_is_valid<true, true>}};
    return tab[mesh][want_md];
}
static K1FnV2 k1_kernel_v2(bool want_md, bool mesh) {
    static const K1FnV2 tab[2][2] = {{k_is_valid_v2<false, false>, k_is_valid_v2<true, false>}, {k_is_valid_v2<false, true>, k_is_valid_v2<true, true>}};
    return tab[mesh][want_md];
}
// baked: index in MOPA_K1_BAKED_SCENES (0: the generic walk).  nullptr: no such instantiation -- the gate reads the centres from
// the slab, and a baked scene has its centre table in LDS and no mesh pairs.
static K1FnV5 k1_kernel_v5(bool want_md, bool cen_lds, bool gate, int baked) {
    static const K1FnV5 generic[3][2] = {{k_is_valid_v5<false, true, false>, k_is_valid_v5<true, true, false>},
                                         {k_is_valid_v5<false, false, false>, k_is_valid_v5<true, false, false>},
                                         {k_is_valid_v5<false, false, true>, k_is_valid_v5<true, false, true>}};
    if (cen_lds && gate) return nullptr;
    if (!baked) return generic[cen_lds ? 0 : (gate ? 2 : 1)][want_md];
    if (!cen_lds) return nullptr;
#define MOPA_K1_CASE(i_, T_) if (baked == i_) return !want_md ? k_is_valid_v5<false, true, false, T_> : k_is_valid_v5<true, true, false, T_>;
    MOPA_K1_BAKED_SCENES(MOPA_K1_CASE)
#undef MOPA_K1_CASE
    return nullptr;
}

// LDS words per wave of baked scene #baked's axis table (0: none)
static int k1_baked_axis_words(int baked) {
#define MOPA_K1_AXW(i_, T_) if (baked == i_) return k1_axis_words<T_>;
    MOPA_K1_BAKED_SCENES(MOPA_K1_AXW)
#undef MOPA_K1_AXW
    return 0;
}

// tiles per narrow-phase drain of baked scene #baked (k1_tiles_per_drain; 0 / generic: 1), and the LDS words per wave its second
// verdict word (and depth words) take out of the entry buffer
static int k1_baked_tiles_per_drain(int baked, bool want_md) {
#define MOPA_K1_TPD(i_, T_) if (baked == i_) return want_md ? k1_tiles_per_drain<T_, true> : k1_tiles_per_drain<T_, false>;
    MOPA_K1_BAKED_SCENES(MOPA_K1_TPD)
#undef MOPA_K1_TPD
    return 1;
}
static int k1_baked_pair_words(int baked, bool want_md) {
#define MOPA_K1_PRW(i_, T_) if (baked == i_) return want_md ? k1_pair_words<T_, true> : k1_pair_words<T_, false>;
    MOPA_K1_BAKED_SCENES(MOPA_K1_PRW)
#undef MOPA_K1_PRW
    return 0;
}

// allow the dynamic LDS size
// the attribute is per function, not per scene: register the device maximum once so scenes of different sizes can
// coexist in one process in any creation order (each launch still passes its own, checked, size)
static std::vector<const void *> k1_kernels() {
    std::vector<const void *> ks;
    for (int md = 0; md < 2; md++)
        for (int mesh = 0; mesh < 2; mesh++) {
            ks.push_back((const void *)k1_kernel_v1(md, mesh));
            ks.push_back((const void *)k1_kernel_v2(md, mesh));
        }
    for (int md = 0; md < 2; md++)
        for (int cen_lds = 0; cen_lds < 2; cen_lds++)
            for (int gate = 0; gate < 2; gate++)
                for (int baked = 0; baked <= kK1BakedScenes; baked++) ks.push_back((const void *)k1_kernel_v5(md, cen_lds, gate, baked));      // (null: no such instantiation)
    return ks;
}
static const LdsKernels kK1Lds(k1_kernels());

// ---------------------------------------------------------------------------
// the plan of one validity batch
// ---------------------------------------------------------------------------
// The launch knobs (all A/B and test knobs; this is the only place that reads them).  Read per call, but for the two grid
// overrides, which are read once per process.
struct K1Knobs {
    bool no_dual_dispatch, debug_mesh, rows_cap_set, pair_tail_set;
    long long rows_cap, pair_tail;
    int rows_blocks, fb_blocks;  // 0: not set
};
static K1Knobs k1_knobs() {
    static const int rows_blocks = std::getenv("MOPA_MESH_ROWS_BLOCKS") ? atoi(std::getenv("MOPA_MESH_ROWS_BLOCKS")) : 0;
    static const int fb_blocks = std::getenv("MOPA_MESH_FALLBACK_BLOCKS") ? atoi(std::getenv("MOPA_MESH_FALLBACK_BLOCKS")) : 0;
    K1Knobs k;
    k.no_dual_dispatch = std::getenv("MOPA_NO_DUAL_DISPATCH") != nullptr;
    k.debug_mesh = std::getenv("MOPA_DEBUG_MESH") != nullptr;
    const char *rc = std::getenv("MOPA_MESH_ROWS_CAP");
    k.rows_cap_set = rc != nullptr;
    k.rows_cap = rc ? atoll(rc) : 0;
    const char *pt = std::getenv("MOPA_K1_PAIR_TAIL_TILES");     // pair drain: the last tiles of a launch that are pulled one at a time
    k.pair_tail_set = pt != nullptr;
    k.pair_tail = pt ? atoll(pt) : 0;
    k.rows_blocks = rows_blocks;
    k.fb_blocks = fb_blocks;
    return k;
}

struct K1Plan {
    const char *refusal = nullptr;   // non-null: MOPA_ERR_UNSUPPORTED with this text, nothing is launched
    // wave-per-state launch (k_is_valid): the whole batch, or -- dual dispatch, next to the lane-per-state launch -- the device-side
    // counts below n_small
    bool wave = false;
    int wave_grid = 0, wave_lds = 0;
    long long n_small = 0;           // lane-per-state launch: counts below it are the wave-per-state launch's (0: it serves every count)
    // lane-per-state launch (k_is_valid_v5 / k_is_valid_v2), 64-state tiles
    bool lane = false, v5 = false;
    int64_t blocks = 0;
    size_t waves = 0;
    int lane_lds = 0, ent_cap = 0;   // ent_cap: hdr.v5_ent_cap of this launch
    bool cen_lds = false, gate = false;   // with `baked` and want_md: the k_is_valid_v5 instantiation; gate: the mesh gate (state list) is on
    int baked = 0;
    int tiles_per_drain = 1;         // pose-slab regions per wave (a pair-drain scene: 2)
    long long pair_tiles = 0;        // pair drain: the leading tiles pulled two at a time (even); the rest go out singly
    bool rows = false;               // the gate hands its mesh pairs to k_mesh_rows
    long long rows_cap = 0;          // rows the gate may hand over per launch; beyond it a state goes to the state list
    unsigned rows_grid = 0;
    int rows_lds = 0;
    bool mesh_pass = false;          // second pass of the MESH instantiation of k_is_valid_v2 (gated: the fallback for the state list)
    unsigned mesh_grid = 0;
    int mesh_lds = 0;
    bool debug_mesh = false;
};

// Everything launch_is_valid decides, from the scene's policy, the batch and the knobs.  No HIP call, no allocation.
static K1Plan k1_plan(const MopaScene *S, int64_t N, bool want_md, bool has_env_idx, bool has_n_dev) {
    const K1Policy &P = S->k1;
    const K1Knobs knobs = k1_knobs();
    K1Plan p;
    const int64_t v2_min = k1_lane_min(S);
    if (has_n_dev && !(P.use_v2 && P.use_v5)) { p.refusal = "a device-side state count needs the lane-per-state kernel"; return p; }
    p.wave_lds = S->lds_bytes;
    p.lane = P.use_v2 && (N >= v2_min || ((has_env_idx || has_n_dev) && P.v2_forced));
    if (!p.lane) {
        p.wave = true;
        p.wave_grid = grid_for(S, N);
        return p;
    }
    // Small batches with explicit env rows or a device-side count used to be sent to the lane-per-state kernel regardless -- at the latency of
    // one 64-state tile (133 us on Push, 289 us on Assembly) for a few hundred states.  The wave-per-state kernel takes env_idx / n_dev too now;
    // a batch whose count is only known on the device and whose WORST CASE is large gets both launches: each reads the count and one of them
    // leaves at once (the wave-per-state one if the count reached v2_min, the lane-per-state one below it).
    if (has_n_dev && !P.v2_forced && N >= v2_min && !knobs.no_dual_dispatch) {
        p.wave = true;
        p.wave_grid = grid_for(S, v2_min);
        p.n_small = v2_min;
    }
    // one lane per state, 64-state tiles; 2 workgroups per CU keep the pose slab small and L2 resident
    const int64_t tiles = (N + 63) / 64;
    p.blocks = std::min<int64_t>((tiles + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)S->n_cu * 2);
    p.waves = (size_t)p.blocks * kWavesPerBlock;
    p.v5 = P.use_v5 != 0;
    p.cen_lds = P.v5_cen_lds;
    p.baked = S->k1_baked;       // (set only for scenes with the centre table in LDS and no mesh pairs)
    p.ent_cap = want_md ? P.v5_ent_cap_md : S->hdr.v5_ent_cap;
    if (p.baked) {
        // the axis table of a baked scene (k1_axis_words, a multiple of 64 words) comes out of the entry buffer: the wave's LDS, and
        // with it two workgroups per CU, stay as the scene compiler sized them.  No room for it: the generic kernel
        // -- and so do the words a pair-drain scene needs for its second tile (k1_pair_words_of)
        const int ax = k1_baked_axis_words(p.baked) + k1_baked_pair_words(p.baked, want_md);
        if (p.ent_cap - ax >= 256) p.ent_cap -= ax;
        else if (ax > 0) p.baked = 0;
        p.tiles_per_drain = k1_baked_tiles_per_drain(p.baked, want_md);
        // the last tiles go out one at a time, one per wave of the launch: the waves then finish within one tile of each other, as
        // without the pair drain, and a batch of no more tiles than waves runs as it did (MOPA_K1_PAIR_TAIL_TILES: another tail; tests)
        if (p.tiles_per_drain > 1) p.pair_tiles = std::max<long long>(0, (long long)tiles - (knobs.pair_tail_set ? std::max<long long>(0, knobs.pair_tail) : (long long)p.waves)) & ~1ll;
    }
    p.lane_lds = !p.v5 ? P.v2_lds_bytes : (want_md ? P.v5_lds_bytes_md : P.v5_lds_bytes);
    // rows the gate may hand over per launch (typically 1-2 % of the states have one): beyond it a state goes to the state list
    p.rows_cap = knobs.rows_cap_set ? knobs.rows_cap : std::min<long long>(std::max<long long>(4096, (long long)N / 2), 1ll << 22);      // (at most 1 GiB of rows; beyond: the state list)
    p.gate = p.v5 && !p.cen_lds && S->n_mesh_gp > 0;
    p.rows = p.gate && p.rows_cap > 0;
    // a device-side count stops the main pass at *n_dev; an ungated mesh pass would still walk all N worst-case rows
    // (uninitialised candidates beyond *n_dev): only the gated form (work list built by the main pass) is served
    if (has_n_dev && S->n_mesh_gp > 0 && !p.gate) { p.refusal = "a device-side state count on a scene with mesh pairs needs the gated mesh pass"; return p; }
    // (159 registers: three waves per SIMD -- the rows are latency chains, so all the slots are offered; idle waves leave at once)
    p.rows_grid = (unsigned)(knobs.rows_blocks > 0 ? knobs.rows_blocks : 3 * S->n_cu);
    p.rows_lds = (int)((size_t)S->n_mesh_dbl * sizeof(double));
    p.mesh_pass = S->n_mesh_gp > 0;
    p.mesh_lds = P.v2_lds_bytes;
    // (the MESH instantiation holds one wave per SIMD: n_cu workgroups are all that run at once, and the gated pass sizes its tiles by
    //  the waves of the launch -- a second round of workgroups would only find the counter exhausted)
    // (with the row list in front of it the gated pass only serves the states whose rows did not fit: a quarter of the CUs)
    const unsigned fb = knobs.fb_blocks > 0 ? (unsigned)knobs.fb_blocks : (p.rows ? (unsigned)std::max(1, S->n_cu / 4) : (unsigned)S->n_cu);
    p.mesh_grid = p.gate ? std::min<unsigned>((unsigned)p.blocks, fb) : (unsigned)p.blocks;
    p.debug_mesh = p.gate && knobs.debug_mesh;
    return p;
}

extern "C" int mopa_scene_valid_kernel(const MopaScene *S, int64_t N, char *out, int32_t cap) {
    if (!S || !out || cap < 24) return fail(MOPA_ERR_INVALID_ARG, "null argument / buffer under 24 bytes");
    const K1Plan p = k1_plan(S, N, false, false, false);
    std::snprintf(out, (size_t)cap, "%s", !p.lane ? "k_is_valid" : (p.v5 ? "k_is_valid_v5" : "k_is_valid_v2"));
    return MOPA_OK;
}
extern "C" int mopa_scene_k1_drain_plan(const MopaScene *S, int64_t N, int32_t want_md, int32_t *tiles_per_drain, int32_t *ent_cap) {
    if (!S || !tiles_per_drain || !ent_cap) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const K1Plan p = k1_plan(S, N, want_md != 0, false, false);
    const bool v5 = p.lane && p.v5;
    *tiles_per_drain = v5 ? p.tiles_per_drain : 0;
    *ent_cap = v5 ? p.ent_cap : 0;
    return MOPA_OK;
}
// the form mopa_check_motion_batch takes for N segments: the wave-per-segment kernel, or the expansion into states
extern "C" int mopa_scene_motion_kernel(const MopaScene *S, int64_t N, char *out, int32_t cap) {
    if (!S || !out || cap < 24) return fail(MOPA_ERR_INVALID_ARG, "null argument / buffer under 24 bytes");
    std::snprintf(out, (size_t)cap, "%s", S->k1.use_v2 && N >= k1_motion_expand_min(S) ? "k_motion_expand" : "k_check_motion");
    return MOPA_OK;
}

// MOPA_V5_TIMELINE (the diagnostic build of tools/k1_wave_timeline.py): the rows of the last lane-per-state launch, [waves][kTlRow]
// words, copied out once the device is idle; returns the number of rows (mopa_valid_v5.inc has the row's layout)
#ifdef MOPA_V5_TIMELINE
constexpr size_t kK1TimelineWords = kTlRow;
static unsigned long long *g_k1_timeline = nullptr;
static long long g_k1_timeline_rows = 0;
extern "C" long long mopa_k1_timeline_read(unsigned long long *out, long long cap_rows) {
    if (!out || !g_k1_timeline || hipDeviceSynchronize() != hipSuccess) return -1;
    const long long n = std::min(cap_rows, g_k1_timeline_rows);
    if (n > 0 && hipMemcpy(out, g_k1_timeline, (size_t)n * kTlRow * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}
#else
constexpr size_t kK1TimelineWords = 0;
#endif

// state validity of N states; env row of state i = env_idx ? env_idx[i] : i / samples_per_env
// n_dev (nullable): the number of states is only known on the device (*n_dev <= N, N then sizes the launch): served by the
// lane-per-state kernel, which reads it when it starts -- no host read-back between the producer of the states and this launch
// attach (the public entry point; env_idx == nullptr): on a glued scene qpos_env holds ordinary rows, and every env row attaches at its
// own joint values behind the argument checks, as in mopa_check_motion_batch; every other caller hands over attached rows
static int launch_is_valid(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env,
                           const int *env_idx, uint8_t *valid, double *min_dist, void *stream, const long long *n_dev = nullptr,
                           bool attach = false) {
    if (!S || !valid || (N > 0 && (!q_active || !qpos_env))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    if (attach && S->glue_b >= 0) {
        const int rc = glue_attach_scratch(S, qpos_env, (N + samples_per_env - 1) / samples_per_env, st, &qpos_env);
        if (rc) return rc;
    }
    dim3 block(kBlock);
    const K1Plan p = k1_plan(S, N, min_dist != nullptr, env_idx != nullptr, n_dev != nullptr);
    if (p.refusal) return fail(MOPA_ERR_UNSUPPORTED, p.refusal);
    if (p.wave) {
        // (on its own it serves every count: n_small out of reach)
        hipLaunchKernelGGL(k1_kernel_v1(min_dist != nullptr, S->hdr.has_mesh != 0), dim3(p.wave_grid), block, p.wave_lds, st, S->hdr, S->d_dbl, S->d_int, q_active, qpos_env,
                           (long long)N, (long long)samples_per_env, valid, min_dist, env_idx, n_dev, p.lane ? p.n_small : (long long)(1ll << 62));
    }
    if (!p.lane) {
        HIP_TRY(hipGetLastError());
        return MOPA_OK;
    }
    StreamScratch &sc = scratch_for(S, st);
    if (p.waves > sc.slab_waves || (size_t)p.tiles_per_drain > sc.slab_tiles) {
        // (a pair-drain plan keeps one slab region per tile of a drain: on Push 2 x 57 KB per wave, 235 MB per stream at 2048 waves)
        const size_t want = std::max(std::max(p.waves, sc.slab_waves), (size_t)S->n_cu * 2 * kWavesPerBlock);
        const size_t tiles = std::max((size_t)p.tiles_per_drain, sc.slab_tiles);
        HIP_TRY(grow(S, sc.slab, (want * tiles * (size_t)(S->hdr.nmg + S->hdr.n_save) * kSlabStride + 16 + want * kK1TimelineWords) * sizeof(double)));
        HIP_TRY(grow(S, sc.mpr, want * (size_t)kMprCapV5 * kMprRow * sizeof(double)));
        HIP_TRY(grow(S, sc.cen, want * (size_t)S->hdr.nmg * 3 * 64 * sizeof(float)));
        sc.slab_waves = want;
        sc.slab_tiles = tiles;
    }
    if (!sc.k1_ctr.p) {
        // zeroed ONCE, synchronously (never inside a stream capture: a first call under capture fails loudly here instead of baking a
        // memset node into the graph).  INVARIANT the kernels keep (tile_ctr_release): every wave of a launch reaches the release, the
        // last one puts [0] and [1] back to zero -- a kernel edit that adds an early return before the release breaks later launches.
        HIP_TRY(grow(S, sc.k1_ctr, 64));
        HIP_TRY(hipMemset(sc.k1_ctr.p, 0, 64));
        HIP_TRY(hipStreamSynchronize(nullptr));      // (a device memset may return before it has run: `st` need not wait for the null stream)
    }
    unsigned long long *const d_ctr = sc.k1_ctr.as<unsigned long long>();
    double *const d_slab = sc.slab.as<double>();
    dim3 grid((unsigned)p.blocks);
#ifdef MOPA_V2_PROFILE
    // [6 profile words | 2 pad] live right behind the slabs of this launch's waves
    double *d_tail = d_slab + (size_t)p.blocks * kWavesPerBlock * p.tiles_per_drain * (S->hdr.nmg + S->hdr.n_save) * kSlabStride;
    unsigned long long *d_prof = (unsigned long long *)d_tail;
    (void)zero_async(d_prof, 6 * 8, st);
#endif
#ifdef MOPA_V5_TIMELINE
    // the waves' timeline rows live right behind the slabs of this launch's waves (where k_is_valid_v5 looks for them)
    g_k1_timeline = reinterpret_cast<unsigned long long *>(d_slab + (size_t)p.blocks * kWavesPerBlock * p.tiles_per_drain * (S->hdr.nmg + S->hdr.n_save) * kSlabStride);
    g_k1_timeline_rows = p.v5 ? (long long)p.waves : 0;
    HIP_TRY(zero_async(g_k1_timeline, p.waves * (size_t)kTlRow * 8, st));
#endif
    long long *mesh_list = nullptr;
    unsigned long long *rows_cnt = nullptr;
    double *mesh_rows = nullptr;
    if (p.gate) {
        HIP_TRY(grow(S, sc.mesh_list, ((size_t)N + 2) * sizeof(long long)));
        rows_cnt = sc.mesh_list.as<unsigned long long>();
        mesh_list = sc.mesh_list.as<long long>() + 1;
        HIP_TRY(zero_async(rows_cnt, 2 * sizeof(long long), st));
        if (p.rows) {
            HIP_TRY(grow(S, sc.mesh_rows, (size_t)p.rows_cap * kMprRow * sizeof(double)));
            mesh_rows = sc.mesh_rows.as<double>();
        }
    }
    if (p.v5) {
        SceneHdr hk = S->hdr;
        hk.v5_ent_cap = p.ent_cap;
        hipLaunchKernelGGL(k1_kernel_v5(min_dist != nullptr, p.cen_lds, p.gate, p.baked), grid, block, p.lane_lds, st, hk, S->d_dbl, S->d_int, S->d_gp_tab, q_active, qpos_env,
                           (long long)N, (long long)samples_per_env, valid, min_dist, d_slab, env_idx, sc.mpr.as<double>(), mesh_list, sc.cen.as<float>(),
                           n_dev, d_ctr, mesh_rows, p.rows_cap, rows_cnt, p.n_small, p.pair_tiles);
        if (p.rows)
            hipLaunchKernelGGL(min_dist ? k_mesh_rows<true> : k_mesh_rows<false>, dim3(p.rows_grid), block, p.rows_lds, st, S->hdr, S->d_dbl, (const double *)mesh_rows,
                               (const unsigned long long *)rows_cnt, p.rows_cap, S->n_mesh_dbl, valid, min_dist);
    } else
        hipLaunchKernelGGL(k1_kernel_v2(min_dist != nullptr, false), grid, block, p.lane_lds, st, S->hdr, S->d_dbl, S->d_int, q_active, qpos_env, (long long)N,   // main lists carry no mesh pair
                           (long long)samples_per_env, valid, min_dist, d_slab, 0, env_idx, (const long long *)nullptr, d_ctr);
    if (p.mesh_pass)
        // second pass: the mesh pairs only (MESH instantiation), verdict AND-ed / depth min-ed into the first pass's
        hipLaunchKernelGGL(k1_kernel_v2(min_dist != nullptr, true), dim3(p.mesh_grid), block, p.mesh_lds, st, S->hdr_mesh, S->d_dbl, S->d_int, q_active, qpos_env, (long long)N,
                           (long long)samples_per_env, valid, min_dist, d_slab, 1, env_idx, (const long long *)mesh_list, d_ctr);
    HIP_TRY(hipGetLastError());
    if (p.debug_mesh) {     // diagnostics: how many states the gate lets through
        long long cnt[2] = {0, 0};
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(cnt, mesh_list - 1, sizeof(cnt), hipMemcpyDeviceToHost);
        fprintf(stderr, "[mopa] mesh gate: %lld rows handed to k_mesh_rows (cap %lld), %lld of %lld states go to the second pass\n", cnt[0], p.rows_cap, cnt[1], (long long)N);
    }
#ifdef MOPA_V2_PROFILE
    {
        unsigned long long hp[6];
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(hp, d_prof, 48, hipMemcpyDeviceToHost);
        if (hp[5]) fprintf(stderr, "[v2 profile] per tile cycles: body %.0f geom %.0f cull+push %.0f flush %.0f total %.0f (tiles %llu)\n",
                           (double)hp[0] / hp[5], (double)hp[1] / hp[5], (double)hp[2] / hp[5], (double)hp[3] / hp[5], (double)hp[4] / hp[5], hp[5]);
    }
#endif
    return MOPA_OK;
}

extern "C" int mopa_is_valid_batch(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N,
                                   int64_t samples_per_env, uint8_t *valid, double *min_dist, void *stream) {
    return launch_is_valid(S, q_active, qpos_env, N, samples_per_env, nullptr, valid, min_dist, stream, nullptr, true);
}
// the same with the state count on the device (*n_dev <= N; N sizes the launch): states from *n_dev on are neither read nor written
extern "C" int mopa_is_valid_batch_counted(MopaScene *S, const double *q_active, const double *qpos_env, int64_t N, int64_t samples_per_env,
                                           uint8_t *valid, double *min_dist, const int64_t *n_dev, void *stream) {
    if (!n_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    return launch_is_valid(S, q_active, qpos_env, N, samples_per_env, nullptr, valid, min_dist, stream, reinterpret_cast<const long long *>(n_dev), true);
}
