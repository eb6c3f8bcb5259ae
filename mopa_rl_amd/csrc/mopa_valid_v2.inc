// mopa_valid_v2.inc -- K1 (second generation): state validity with one LANE per state for forward
// kinematics + broad phase, and a wave-wide LDS work queue for the narrow phase.
// (included by mopa_hip.hip after the SceneHdr / LdsView definitions)
//
// Why: the first-generation kernel (one wave per state) issued ~4.4k FP64 VALU wave-instructions per
// state with ~12 % of lanes active (profiles/r01): FK used 14 of 64 lanes and the narrow phase saw a
// dozen surviving pairs.  Here a wave owns a tile of 64 states:
//   * FK runs once per tile with every lane working on its own state (scene constants are wave-uniform
//     -> scalar loads), so its cost is amortised 64x;
//   * each moving geom is culled against its partners while its pose is still in registers; all lanes
//     test the SAME pair, so there is no divergence in the broad phase;
//   * survivors (state, pair) are appended -- ballot + prefix popcount -- to a ring queue in LDS that
//     carries the posed geoms; whenever 64 entries are pending the wave runs the narrow phase on them
//     with all lanes busy.  Entries arrive grouped by pair type, so a batch executes few type branches;
//   * verdicts go to an LDS bit mask (ds_or) and are written as one coalesced 64-byte store per tile;
//     a state that is already invalid stops queueing work (per-state early-out).
// Moving-vs-moving pairs need the pose of an earlier geom: poses are parked in a per-wave slab in
// global memory ([slot][7][64 lanes], perfectly coalesced, L2 resident) and read back lane-per-state.
// The arithmetic per body / geom / pair is unchanged, so results stay bit-identical to the oracle.

#ifdef MOPA_V2_PROFILE
// phase timers (wave-cycles via s_memtime), summed over waves into prof[0..5]:
//   0 body pose, 1 geom pose + slab store, 2 cull + queue push, 3 narrow phase (flush), 4 whole tile, 5 tiles
#define V2_T0() long long _t0 = __builtin_readcyclecounter()
#define V2_ACC(k) do { long long _t1 = __builtin_readcyclecounter(); prof_acc[k] += _t1 - _t0; _t0 = _t1; } while (0)
#else
#define V2_T0() do {} while (0)
#define V2_ACC(k) do {} while (0)
#endif
constexpr int kQCapV2 = 128;                 // ring capacity (entries); a batch is 64
constexpr int kSlabStride = 7 * 64;          // doubles per slab slot: pos[3] quat[4] x 64 lanes

struct alignas(32) V2BodyI { int jn, jntadr, load, sf, save, mgadr, mgnum, jt_qsrc; };
struct alignas(16) V2GeomI { int g, store, padr, pnum; };

struct V2Lds {
    double *qa;                 // [7][kQCapV2]   posed "current" geom: pos, quat
    double *qb;                 // [7][kQCapV2]   posed partner (moving partners only)
    int *qw;                    // [kQCapV2]      partner gid | code<<8 | cur_is_g2<<12 | partner_moving<<13 | cur gid<<14 | lane<<22
    unsigned long long *bad;    // [1]            bit l set = state of lane l is invalid
    unsigned long long *md;     // [64]           sortable bits of the running minimum distance per state
};

MOPA_D unsigned long long f64_sortable(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
MOPA_D double f64_unsortable(unsigned long long u) {
    u = (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u;
    return __longlong_as_double((long long)u);
}

#ifndef MOPA_MESH_TILE
#define MOPA_MESH_TILE 0
#endif
constexpr int kMeshTileStates = MOPA_MESH_TILE;   // gated mesh pass: states per wave (its pairs are few and slow: spread them over many waves); 0 = one tile per wave of the launch
constexpr int kV2LdsPerWave = ((2 * 7 * kQCapV2 * 8) + 64 * 8 + 8 + kQCapV2 * 4 + 15) & ~15;

// narrow phase on `n` (<= 64) queue entries starting at ring position `head`.  The MESH instantiation (the light second
// pass over the handful of mesh pairs) gives every entry a QUAD of lanes: they evaluate the same pair and share the
// exhaustive vertex searches of the hull's support function (mopa_device.hpp: mesh_support_local<4>), which is where
// its time goes -- 16 entries per round instead of 64, each ~4x sooner.
template <bool WANT_MD, bool MESH>
MOPA_D void v2_flush(const SceneHdr &h, const LdsView &v, const V2Lds &q, int lane, int head, int n) {
    constexpr int G = MESH ? 4 : 1;
    for (int base = 0; base < n; base += 64 / G) {
    const int ent = base + lane / G;
    if (ent < n) {
        const int idx = (head + ent) & (kQCapV2 - 1);
        const int w = q.qw[idx];
        const int pg = w & 0xff, code = (w >> 8) & 0xf, cur_is_g2 = (w >> 12) & 1, pmov = (w >> 13) & 1;
        const int cg = (w >> 14) & 0xff, sl = (w >> 22) & 0x3f;
        const double *D = v.dbl;
        const int *I = v.ints;
        double RC[15], RP[15];
        {
            RC[0] = q.qa[0 * kQCapV2 + idx]; RC[1] = q.qa[1 * kQCapV2 + idx]; RC[2] = q.qa[2 * kQCapV2 + idx];
            Q4 gq{q.qa[3 * kQCapV2 + idx], q.qa[4 * kQCapV2 + idx], q.qa[5 * kQCapV2 + idx], q.qa[6 * kQCapV2 + idx]};
            quat2mat(RC + GO_MAT, gq);
            const double *sz = D + h.o_g_rec + cg * kGeomStride + GO_SIZE;
            RC[12] = sz[0]; RC[13] = sz[1]; RC[14] = sz[2];
        }
        if (pmov) {
            RP[0] = q.qb[0 * kQCapV2 + idx]; RP[1] = q.qb[1 * kQCapV2 + idx]; RP[2] = q.qb[2 * kQCapV2 + idx];
            Q4 gq{q.qb[3 * kQCapV2 + idx], q.qb[4 * kQCapV2 + idx], q.qb[5 * kQCapV2 + idx], q.qb[6 * kQCapV2 + idx]};
            quat2mat(RP + GO_MAT, gq);
            const double *sz = D + h.o_g_rec + pg * kGeomStride + GO_SIZE;
            RP[12] = sz[0]; RP[13] = sz[1]; RP[14] = sz[2];
        } else {
            const double *sr = D + h.o_g_rec + pg * kGeomStride;
#pragma unroll
            for (int i = 0; i < 15; i++) RP[i] = sr[i];
        }
        double R1[15], R2[15];
#pragma unroll
        for (int i = 0; i < 15; i++) {
            R1[i] = cur_is_g2 ? RP[i] : RC[i];
            R2[i] = cur_is_g2 ? RC[i] : RP[i];
        }
        const int t1 = I[h.o_g_type + (cur_is_g2 ? pg : cg)], t2 = I[h.o_g_type + (cur_is_g2 ? cg : pg)];
        const double d = geom_dist<MESH, G>(code, R1, t1, R2, t2, D);
        if ((lane & (G - 1)) == 0) {
            if (d <= h.thr) atomicOr(q.bad, 1ull << sl);
            if (WANT_MD) atomicMin(q.md + sl, f64_sortable(d));
        }
    }
    }
    wave_sync();
}

template <bool WANT_MD, bool MESH>
__global__ __launch_bounds__(kBlock) void k_is_valid_v2(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                         const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                         long long N, long long samples_per_env, unsigned char *__restrict__ valid,
                                                         double *__restrict__ min_dist, double *__restrict__ slab_all, int combine,
                                                         const int *__restrict__ env_idx /* nullable: env row of every state */,
                                                         const long long *__restrict__ list /* nullable: [0] = count, then the states of a gated second pass */,
                                                         unsigned long long *__restrict__ tile_ctr /* [0] next tile, [1] waves done; zero between launches */) {
    if (list && list[0] == 0) {       // gated second pass with nothing listed (the usual case since the gate hands its mesh pairs to k_mesh_rows): leave before the scene is staged
        tile_ctr_release(tile_ctr, threadIdx.x & 63);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS: [scene doubles][scene ints][per-wave queue region x4]
    double *s_dbl = reinterpret_cast<double *>(smem);
    int *s_int = reinterpret_cast<int *>(s_dbl + h.n_dbl);
    stage_scene(h, g_dbl, g_int, s_dbl, s_int);
    LdsView v;
    v.dbl = s_dbl; v.ints = s_int; v.grec = nullptr; v.qbuf = nullptr; v.sc = nullptr; v.wl = nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V2Lds q;
    {
        unsigned char *base = reinterpret_cast<unsigned char *>(s_int + ((h.n_int + 1) & ~1)) + wave * kV2LdsPerWave;
        q.qa = reinterpret_cast<double *>(base);
        q.qb = q.qa + 7 * kQCapV2;
        q.md = reinterpret_cast<unsigned long long *>(q.qb + 7 * kQCapV2);
        q.bad = q.md + 64;
        q.qw = reinterpret_cast<int *>(q.bad + 1);
    }
    // wave-uniform scene data is read through the global pointers (scalar loads)
    const double *__restrict__ GD = g_dbl;
    const int32_t *__restrict__ GI = g_int;
    const int nslab = h.nmg + h.n_save;
    double *slab = slab_all + ((size_t)blockIdx.x * kWavesPerBlock + wave) * (size_t)nslab * kSlabStride + lane;
    if (list) N = list[0];     // gated second pass: only the listed states (written by the first pass on the same stream)
    // ... in small tiles (kMeshTileStates): the list is short (< 1 % of the states) and its pairs are the expensive ones (portal refinement
    // against a 106-vertex hull, ~60 us per batch), so the work is spread over many waves instead of filling few
    // (round 6: the tile is sized so that every wave of the launch gets at most ONE -- ceil(N / waves), at least 1, at most 64: with fixed
    //  8-state tiles 1095 tiles met 1024 resident waves and the pass lasted two tiles, 0.23 ms; MOPA_MESH_TILE > 0 at build time restores
    //  the fixed size)
    const long long n_waves = (long long)gridDim.x * kWavesPerBlock;
    int tile_states = 64;
    if (list) {
        const long long per = (N + n_waves - 1) / n_waves;
        tile_states = kMeshTileStates > 0 ? kMeshTileStates : (int)(per < 1 ? 1 : (per > 64 ? 64 : per));
    }
    const long long n_tiles = (N + tile_states - 1) / tile_states;
    // dynamic tile scheduling: tiles differ a lot in cost (early-outs, number of broad-phase survivors), so
    // every wave pulls its next 64-state tile from a global counter (zero between launches: the last wave to leave resets it)
    for (;;) {
        long long tile = 0;
        if (lane == 0) tile = (long long)atomicAdd(tile_ctr, 1ull);
        tile = __shfl(tile, 0, 64);
        if (tile >= n_tiles) break;
        long long s = tile * tile_states + lane;
        const bool act = lane < tile_states && s < N;
        if (!act) s = N - 1;
        if (list) s = list[1 + s];
        const double *qa_row = q_active + s * h.na;
        const double *env_row = qpos_env + (env_idx ? (long long)env_idx[s] : s / samples_per_env) * h.nq;
        if (lane == 0) *q.bad = 0ull;
        if (WANT_MD) q.md[lane] = f64_sortable(0.0);   // deepest penetration: min(0, min over pairs)
        wave_sync();
        bool dead = !act;
        int head = 0, count = 0;
        V3 pos{0.0, 0.0, 0.0};
        Q4 quat{1.0, 0.0, 0.0, 0.0};
        double mat[9];
#ifdef MOPA_V2_PROFILE
        long long prof_acc[6] = {0, 0, 0, 0, 0, 0};
        const long long _tile0 = __builtin_readcyclecounter();
#endif
        // all planned joint values of this lane's state are requested together (one memory latency)
        double qact[8];
#pragma unroll
        for (int a = 0; a < 8; a++) qact[a] = (a < h.na) ? qa_row[a] : 0.0;
        V2_T0();
        for (int b = 0; b < h.nmb; b++) {
            // ---------- pose of moving body b (same operation order as the parent-first sweep) ----------
            // packed per-body record: 8 ints through ONE scalar load, 16 doubles through one batch of LDS
            // broadcast reads (instead of a dozen dependent single-dword scalar loads)
            const V2BodyI bi = *reinterpret_cast<const V2BodyI *>(GI + h.o_mbr + 8 * b);
            const double *bd = s_dbl + h.o_mbd + 16 * b;   // pos[3] quat[4] axis[3] jpos[3] ref
            const int jt0 = bi.jt_qsrc & 0x7f, qsrc0 = bi.jt_qsrc >> 8;
            const bool jp00 = (bi.jt_qsrc & 0x80) != 0;   // joint anchor at the body origin (wave-uniform => scalar branch)
            if (bi.jn == 1 && jt0 == J_FREE) {
                const double *qp = env_row + GI[h.o_pq_adr + (qsrc0 - h.na)];   // free joints are never planned over
                fk_free_step(qp, pos, quat);
            } else {
                V3 ppos;
                Q4 pquat;
                if (bi.load == -2) {            // parent is a static frame
                    sf_frame_ld(h, s_dbl, bi.sf, ppos, pquat, mat);
                } else if (bi.load >= 0) {      // parent pose was parked when the DFS left its subtree
                    const double *sp = slab + (size_t)(h.nmg + bi.load) * kSlabStride;
                    pose7_ld<64>(sp, ppos, pquat);
                    quat2mat(mat, pquat);
                } else {                        // parent is the previous body
                    ppos = pos;
                    pquat = quat;
                }
                if (jt0 == J_GLUE) {            // the carried body of a glued scene: local pose out of the env row's free-joint slots
                    const double *qp = env_row + GI[h.o_pq_adr + (qsrc0 - h.na)];
                    fk_glue_step(ppos, pquat, mat, qp, pos, quat);
                } else {
                    V3 vv = mat_vec(mat, ld3(bd));
                    pos = add3(ppos, vv);
                    quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
                }
                for (int jj = 0; jj < bi.jn; jj++) {
                    V3 ax, jp;
                    double ref;
                    int jt, src;
                    bool jp0;
                    if (jj == 0) {
                        ax = ld3(bd + 7); jp = ld3(bd + 10); ref = bd[13]; jt = jt0; src = qsrc0; jp0 = jp00;
                    } else {                    // bodies with several joints: generic (slow) path
                        const int j = bi.jntadr + jj;
                        ax = ld3(GD + h.o_mj_axis + 3 * j); jp = ld3(GD + h.o_mj_pos + 3 * j); ref = GD[h.o_mj_ref + j];
                        jt = GI[h.o_mj_type + j]; src = GI[h.o_mj_qsrc + j]; jp0 = is_zero3(jp);
                    }
                    double qv;
                    if (src < h.na && h.na <= 8) {
                        qv = qact[0];
#pragma unroll
                        for (int a = 1; a < 8; a++) qv = (src == a) ? qact[a] : qv;
                    } else {
                        qv = (src < h.na) ? qa_row[src] : env_row[GI[h.o_pq_adr + (src - h.na)]];
                    }
                    const double dq = qv - ref;
                    apply_joint(jt, ax, jp, jp0, dq, pos, quat);
                }
                quat = quat_normalize(quat);
            }
            quat2mat(mat, quat);
            V2_ACC(0);
            if (bi.save >= 0) {
                double *sp = slab + (size_t)(h.nmg + bi.save) * kSlabStride;
                pose7_st<64>(sp, pos, quat);
            }
            // ---------- moving geoms of this body ----------
            for (int m = bi.mgadr; m < bi.mgadr + bi.mgnum; m++) {
                const V2GeomI gi = *reinterpret_cast<const V2GeomI *>(GI + h.o_mgr + 4 * m);
                const double *gd = s_dbl + h.o_mgd + 8 * m;   // lpos[3] lquat[4] rbound
                const int g = gi.g;
                const V3 gp = add3(pos, mat_vec(mat, ld3(gd)));
                const Q4 gq = quat_mul(quat, Q4{gd[3], gd[4], gd[5], gd[6]});
                if (gi.store & 1) {
                    double *sp = slab + (size_t)m * kSlabStride;
                    pose7_st<64>(sp, gp, gq);
                }
                const double rbg = gd[7];
                V2_ACC(1);
                const int p0 = gi.padr, p1 = p0 + gi.pnum;
                for (int p = p0; p < p1; p++) {
                    const int w = GI[h.o_gp_word + p];
                    const int pg = w & 0xff, pmov = (w >> 13) & 1, pslot = (w >> 14) & 0xff;
                    const double rbp = GD[h.o_g_rbound + pg];
                    bool cull;
                    const double *sp = slab + (size_t)pslot * kSlabStride;
                    if (pmov) {
                        // bounding spheres; operand order (g1, g2) as in the pair list
                        const V3 pp{sp[0], sp[64], sp[128]};
                        const V3 diff = ((w >> 12) & 1) ? sub3(gp, pp) : sub3(pp, gp);
                        const double rs = ((w >> 12) & 1) ? (rbp + rbg) : (rbg + rbp);
                        cull = dot3(diff, diff) > rs * rs;
                    } else {
                        const double *sr = GD + h.o_g_rec + pg * kGeomStride;
                        const V3 pp = ld3(sr + GO_POS);
                        if (GI[h.o_g_type + pg] == G_PLANE) {
                            // plane is always g1: signed distance of the geom centre vs its bounding radius
                            cull = dot3(sub3(gp, pp), col3(sr + GO_MAT, 2)) > rbg;
                        } else {
                            const V3 diff = ((w >> 12) & 1) ? sub3(gp, pp) : sub3(pp, gp);
                            const double rs = ((w >> 12) & 1) ? (rbp + rbg) : (rbg + rbp);
                            // bounding spheres, then the static partner's world AABB vs this geom's bounding sphere
                            cull = dot3(diff, diff) > rs * rs || aabb_cull(pp, GD + h.o_g_aabb + 3 * pg, gp, rbg);
                        }
                    }
                    const bool surv = !cull && !dead;
                    const unsigned long long mask = __ballot(surv);
                    if (mask) {
                        if (surv) {
                            const int idx = (head + count + __popcll(mask & ((1ull << lane) - 1ull))) & (kQCapV2 - 1);
                            q.qa[0 * kQCapV2 + idx] = gp.x; q.qa[1 * kQCapV2 + idx] = gp.y; q.qa[2 * kQCapV2 + idx] = gp.z;
                            q.qa[3 * kQCapV2 + idx] = gq.w; q.qa[4 * kQCapV2 + idx] = gq.x; q.qa[5 * kQCapV2 + idx] = gq.y;
                            q.qa[6 * kQCapV2 + idx] = gq.z;
                            if (pmov) {
#pragma unroll
                                for (int c = 0; c < 7; c++) q.qb[c * kQCapV2 + idx] = sp[c * 64];
                            }
                            q.qw[idx] = (w & 0x3fff) | (g << 14) | (lane << 22);
                        }
                        count += __popcll(mask);
                        if (count >= 64) {
                            V2_ACC(2);
                            wave_sync();
                            v2_flush<WANT_MD, MESH>(h, v, q, lane, head, 64);
                            V2_ACC(3);
                            head = (head + 64) & (kQCapV2 - 1);
                            count -= 64;
                            if (!WANT_MD) dead = dead || ((*q.bad >> lane) & 1ull);
                        }
                    }
                }
            }
        }
        V2_ACC(2);
        if (count > 0) {
            wave_sync();
            v2_flush<WANT_MD, MESH>(h, v, q, lane, head, count);
        }
        V2_ACC(3);
#ifdef MOPA_V2_PROFILE
        prof_acc[4] = __builtin_readcyclecounter() - _tile0;
        prof_acc[5] = 1;
        if (lane == 0 && min_dist == nullptr)
            for (int k = 0; k < 6; k++) atomicAdd((unsigned long long *)(slab_all + (size_t)gridDim.x * kWavesPerBlock * nslab * kSlabStride) + k, (unsigned long long)prof_acc[k]);
#endif
        wave_sync();
        if (act) {
            // combine: this launch covers a subset of the pairs (the mesh pairs); fold into the previous launch's result
            const unsigned char ok = ((*q.bad >> lane) & 1ull) ? 0 : 1;
            valid[s] = combine ? (unsigned char)(valid[s] & ok) : ok;
            if (WANT_MD) {
                const double mdv = f64_unsortable(q.md[lane]);
                min_dist[s] = (combine && min_dist[s] < mdv) ? min_dist[s] : mdv;
            }
        }
        wave_sync();
    }
    tile_ctr_release(tile_ctr, lane);
}
