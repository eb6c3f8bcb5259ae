// mopa_hip.hip -- libmopa_hip.so: scene compilation, HIP kernels and the C ABI
// declared in include/mopa_hip.h.  Target: gfx950 (MI355X), wave64.
//
// Kernels:
//   K1 state validity, two generations
//      k_is_valid_v2 (mopa_valid_v2.inc, production for large batches): one LANE per state, 64-state tiles,
//        FK per lane, cull while the pose is in registers, wave-wide narrow phase from an LDS ring queue;
//      k_is_valid (this file): one wave64 per state -- small batches, single-state API calls and the device
//        routine the planner kernels call.  Scene constants (~10 KB) are staged once per workgroup in LDS.
//   K2 k_check_motion  one wave per segment (OMPL DiscreteMotionValidator semantics)
//      k_motion_report (mopa_motion_report.inc) the same walk in ascending order: where a segment is blocked, and by which pairs
//      k_clearance_states (mopa_motion_clearance.inc) one wave per expanded state: how near a segment comes, where, and to which pair
//   K3 k_rrt_connect   (mopa_planner.inc) one wave per env
//   K4 k_env_step      (mopa_env.inc) one lane per env, kinematic env.step
//   FP64 VALU bound, no MFMA (there is no dense contraction on this path).
// Host side of K1: the scene compiler and the scene's K1 policy in mopa_scene_build.inc, the launch plan (k1_plan), the table of
// K1 instantiations and launch_is_valid in mopa_valid_launch.inc.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <map>
#include <mutex>
#include "../../include/mopa_hip.h"
#include "mopa_device.hpp"
#include "mopa_frames.hpp"
#include "mopa_manifold.hpp"
#include "mopa_sep.hpp"
#include "mopa_witness.hpp"
#include "mopa_fk.hpp"
#include "mopa_host.hpp"
#include "mopa_model_host.hpp"

using namespace mopa;

// ---------------------------------------------------------------------------
// error plumbing (mopa_host.hpp: fail / HIP_TRY / DeviceGuard / ON_DEVICE / DevBuf, shared with mopa_envdyn.hip)
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
int mopa_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
constexpr double kV5MaxReach = 32.0;        // metres: beyond this the FP32 broad phase is not used (see mopa_scene_create)
// The kernels that take more dynamic LDS than the default allows: every file that defines some adds them with a file-scope
// `static const LdsKernels` object, next to the kernels; scene_create walks the list (null entries: holes of a kernel table).
static std::vector<const void *> &lds_kernels() {
    static std::vector<const void *> list;
    return list;
}
struct LdsKernels {
    LdsKernels(const std::vector<const void *> &ks) { lds_kernels().insert(lds_kernels().end(), ks.begin(), ks.end()); }
};

extern "C" const char *mopa_last_error(void) { return g_err.c_str(); }
extern "C" const char *mopa_version(void) { return "mopa_hip 0.1.0 (gfx950)"; }
extern "C" int mopa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------
// device scene: a header of counts/offsets (kernel argument, lives in SGPRs)
// plus one blob of doubles and one of ints that every workgroup copies to LDS.
// ---------------------------------------------------------------------------
struct SceneHdr {
    int na, nq, n_pq, nmb, nmj, nsf, ng, nmg, npair;
    int n_dbl, n_int;            // blob sizes
    // double-blob offsets
    int o_mb_pos, o_mb_quat, o_sf_pos, o_sf_quat, o_sf_mat, o_mj_axis, o_mj_pos, o_mj_ref;
    int o_g_lpos, o_g_lquat, o_g_rbound, o_g_rec, o_act_lo, o_act_hi, o_act_ext;
    int o_act_ref, o_act_hinge;   // per active joint value slot: the joint's reference value (doubles), 1 = hinge (ints)
    int o_g_aabb;   // [ng][3] world-AABB half extents of static geoms (second-stage cull), zeros for moving geoms
    // int-blob offsets
    int o_mb_parent, o_mb_jntadr, o_mb_jntnum, o_mj_type, o_mj_qsrc, o_g_type, o_g_slot, o_g_mb;
    int o_mg_geom, o_chain_adr, o_chain_len, o_chain_items, o_pairs, o_pq_adr, o_act_adr, o_act_so2;
    // second-generation validity kernel (mopa_valid_v2.inc): DFS program + per-geom pair lists
    int n_save, n_gp;
    int v5_ent_cap;   // k_is_valid_v5: survivor-entry buffer capacity per wave
    int o_mesh, has_mesh;   // mesh hull vertices (doubles); has_mesh selects the MESH kernel instantiations
    int o_mb_load, o_mb_save, o_mb_mgadr, o_mb_mgnum, o_mg_padr, o_mg_pnum, o_mg_store, o_gp_word;
    int o_mbr, o_mbd, o_mgr, o_mgd;   // packed per-body / per-geom records (ints: 8 / 4, doubles: 16 / 8)
    // planner FK (mopa_planner.inc: ms_fk): per moving geom slot 8 ints -- [0..3] the chain's bodies, one per byte (0xff past the
    // end), [4] chain length, [5] static frame of the chain root's parent; pfk_maxlen = longest chain (0: a chain is longer than
    // 16 bodies -> the planner keeps the generic walk)
    int o_pfk, pfk_maxlen;
    // k_is_valid_v5, tiles whose 64 states share one env row: the moving bodies no ACTIVE coordinate reaches (a manipulated object's free
    // body and what is welded to it: Assembly's furniture = 21 bodies, 20 geoms) are posed ONCE per tile, one body per lane, level by level,
    // instead of by every lane in its walk.  o_pas_b: the bodies (moving-body ids) in level order, o_pas_lv [n_pas_lv + 1]: level starts,
    // o_mb_pas [nmb]: position in that list or -1 (bit 16: nothing continues from this body's registers), o_pas_g: the moving-geom slots
    // on them, o_mg_pas [nmg]: position or -1.  n_pas_b = 0: off.
    int n_pas_b, n_pas_g, n_pas_lv, o_pas_b, o_pas_lv, o_mb_pas, o_pas_g, o_mg_pas;
    // per-wave LDS slab (in doubles): geom records, qbuf; then worklist (u16)
    int wave_dbl, wave_bytes;
    double thr, range, resolution;
    double nn_eps;   // planner: bound on |FP32 mirror distance - FP64 distance| of the nearest-neighbour sweep (mopa_planner.inc)
};

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;

struct StreamScratch {
    DevBuf slab;        // lane-per-state kernels: pose slabs of the launch's waves + [profile words | tile counter]
    DevBuf mpr;         // v5: per-wave ring of deferred cylinder pairs
    DevBuf cen;         // v5, scenes whose FP32 centre table does not fit LDS: the per-wave tables in global memory
    DevBuf k1_ctr;      // validity kernels' tile counter + exit count (self-resetting: tile_ctr_release)
    DevBuf mesh_list;   // [0] = number of rows in mesh_rows, [1] = count, then the states with a mesh pair past the main pass's broad phase
    DevBuf mesh_rows;   // complete records of the mesh pairs within reach ([cap][kMprRow] doubles; k_mesh_rows)
    size_t slab_waves = 0, slab_tiles = 0;   // what `slab` is sized for: waves, and slab regions per wave (tiles per drain)
    DevBuf mv_cnt, mv_off, mv_env, mv_q, mv_valid, mv_scan;   // expanded motion validation (mopa_motion.inc)
    DevBuf mr_fbq;                                            // motion report: first_bad_q when the caller keeps no rows but asks for blockers
    DevBuf mc_d, mc_p;                                        // clearance report (mopa_motion_clearance.inc): per expanded state its clearance and nearest pair
    DevBuf plan_q, plan_p, plan_ctr;                          // planner: both trees of every env, env counter (mopa_planner.inc)
    DevBuf race_rec, race_word;                               // K3 race (mopa_race.inc): the members' records, one race word per query
    DevBuf ip_walk;                                           // straight-line pre-check: walk states + verdicts (mopa_paths.inc)
    DevBuf pb_small, pb_rows, pb_act;                         // batched pull-back: verdicts / slots, candidate rows, their active coordinates + verdicts
    DevBuf ct_valid, ct_md, ct_ctr;                           // contact report (mopa_contacts.inc): stage 1's verdicts and depths, stage 2's chunk counter
    DevBuf star_tree, star_k;                                 // RRT* (mopa_rrtstar.inc): one tree slab per wave of a launch, the table k(n)
    DevBuf glue_rows;                                         // glued scene: the attached rows of a call's env rows (mopa_glue.inc)
    int star_k_n = 0;                                         // entries of star_k, computed for rewire factor star_k_rf
    double star_k_rf = 0.0;
};

// The scene's share of the K1 policy: filled once, by the last step of the scene compiler (mopa_scene_build.inc: SceneBuild::k1_policy);
// what a batch gets out of it is decided in k1_plan (mopa_valid_launch.inc).
struct K1Policy {
    int use_v2 = 1;              // lane-per-state kernels (second generation and up) for large batches
    int use_v5 = 0;              // third generation (FP32 broad phase out of LDS) in their place
    bool v2_forced = false;      // MOPA_VALID_KERNEL=v2 / v5: lane-per-state kernel for every N >= 64 (tests, A/B runs)
    bool v5_cen_lds = true;      // FP32 centre table of a tile in LDS (false: read back from the pose slab; scenes with many moving geoms)
    int v2_lds_bytes = 0;
    int v5_lds_bytes = 0;        // verdict-only instantiations of k_is_valid_v5 (hdr.v5_ent_cap entries per wave)
    int v5_lds_bytes_md = 0, v5_ent_cap_md = 0;   // depth-reporting instantiations
    int64_t motion_chunk = 1;    // K2, expanded motion (mopa_motion.inc: motion_for_chunks): segments per chunk of the pipeline
};

struct MopaScene {
    int device = 0;
    SceneHdr hdr{};
    SceneHdr hdr_mesh{};      // same scene, per-geom pair lists = the mesh pairs only (second pass of the lane-per-state kernels)
    int n_mesh_dbl = 0;       // doubles of the hull-vertex block at hdr.o_mesh (k_mesh_rows stages it in LDS)
    int n_mesh_gp = 0;
    std::vector<double> h_dbl;
    std::vector<int32_t> h_int;
    std::vector<int32_t> h_gp_tab;
    double *d_dbl = nullptr;
    int32_t *d_int = nullptr;
    int lds_bytes = 0;
    // host copies for the single-query forms
    int nq = 0, na = 0, ngeom_model = 0, npair_model = 0;
    std::vector<int32_t> active_idx;
    std::vector<int32_t> pair_slot;   // model pair index -> device pair index or -1
    std::vector<int32_t> pair_model;  // device pair index -> model pair index (contact report)
    int32_t *d_pair_model = nullptr;
    int32_t *d_pair_slot = nullptr;   // pair_slot on the device (contact frames)
    bool pruned = false;              // created with pair_cull_radius: the pair list is proven down to the contact threshold only
    std::vector<int32_t> geom_model_of_dev;  // (identity; device geoms == model collidable geoms)
    uint64_t seed = 0;
    std::string status = "none";
    // scratch for single-query calls
    double *d_q = nullptr;      // nq + na + big scratch
    uint8_t *d_valid = nullptr;
    double *d_md = nullptr;
    double *d_dbg = nullptr;
    size_t dbg_doubles = 0;
    int n_cu = 256;
    int32_t *d_gp_tab = nullptr;   // v5: FP32 broad-phase table [n_gp][8]
    K1Policy k1;              // which validity kernels the scene gets (filled by the scene compiler's last step)
    // glued scene (mopa_scene_create_glued): model body ids (-1: not glued), their moving-body ids, qpos address of body_b's free joint
    int glue_a = -1, glue_b = -1, glue_mb_a = -1, glue_mb_b = -1, glue_adr = -1;
    int k1_baked = 0;         // k_is_valid_v5 on a baked scene: its index in MOPA_K1_BAKED_SCENES (0: the generic instantiation)
    // Launch scratch, one set PER STREAM: a scene may be driven from several streams at once (validity on one stream while
    // the planner or the previous step's motion check runs on another); calls on the same stream are ordered by the
    // stream.  Buffers only ever grow; an outgrown buffer may still be read by kernels in flight, so it is retired and
    // freed with the scene, never on the hot path.
    std::mutex mu;
    std::map<hipStream_t, StreamScratch> scratch;
    std::vector<void *> retired;
};

static StreamScratch &scratch_for(MopaScene *S, hipStream_t st) {
    std::lock_guard<std::mutex> lock(S->mu);
    return S->scratch[st];       // std::map: references stay valid across later insertions
}
// make `b` hold at least `bytes`; returns a HIP error code
static hipError_t grow(MopaScene *S, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return hipSuccess;
    const size_t want = std::max(bytes, b.cap + b.cap / 2);
    void *np = nullptr;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess) return e;
    if (b.p) {
        std::lock_guard<std::mutex> lock(S->mu);
        S->retired.push_back(b.p);
    }
    b.p = np;
    b.cap = want;
    return hipSuccess;
}
// The work counter of the report kernels (k_contact_rows, k_proximity_rows, k_clearance_states; one per stream, shared: calls on a
// stream are ordered): zeroed once, synchronously; the kernels put it back to zero themselves (tile_ctr_release).
static int ensure_report_ctr(MopaScene *S, StreamScratch &sc) {
    if (sc.ct_ctr.p) return MOPA_OK;
    HIP_TRY(grow(S, sc.ct_ctr, 64));
    HIP_TRY(hipMemset(sc.ct_ctr.p, 0, 64));
    HIP_TRY(hipStreamSynchronize(nullptr));      // (a device memset may return before it has run: the call's stream need not wait for the null stream)
    return MOPA_OK;
}

// Zero a few 8-byte words on a stream.  A kernel, not hipMemsetAsync: these launches are also captured into HIP graphs
// (rollout.py, cfg.use_graphs), and small memset nodes proved unreliable there.
__global__ void k_zero_words(unsigned long long *p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0ull;
}
static hipError_t zero_async(void *p, size_t bytes, hipStream_t st) {
    hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long *>(p), (int)((bytes + 7) / 8));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
MOPA_D void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
MOPA_D bool wave_any(bool p) { return __ballot(p) != 0ull; }
MOPA_D double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_xor(v, off, 64);
        v = (o < v) ? o : v;
    }
    return v;
}

// A persistent kernel's work counter that needs no zeroing launch: ctr[0] hands out the work items, ctr[1] counts the waves that have
// found none left; the last of the grid's waves to say so puts both back to zero for the next launch on the stream.
MOPA_D void tile_ctr_release(unsigned long long *ctr, int lane) {
    if (lane == 0) {
        const unsigned long long done = atomicAdd(ctr + 1, 1ull);
        if (done + 1ull == (unsigned long long)gridDim.x * (blockDim.x >> 6)) {
            atomicExch(ctr, 0ull);
            atomicExch(ctr + 1, 0ull);
        }
    }
}
// ... and the pull of its next work item, 64 bits.  The index is wave-uniform: through readfirstlane it and every address formed
// from it stay in scalar registers.
MOPA_D long long wave_pull64(unsigned long long *ctr, int lane) {
    unsigned long long t = 0ull;
    if (lane == 0) t = atomicAdd(ctr, 1ull);
    const unsigned t_lo = __builtin_amdgcn_readfirstlane((unsigned)t), t_hi = __builtin_amdgcn_readfirstlane((unsigned)(t >> 32));
    return (long long)(((unsigned long long)t_hi << 32) | t_lo);
}
// wave-wide minimum under the (distance, index) order -- a strictly smaller distance, or an equal one with a lower index; every
// lane ends with the winner.  The one selection rule of the proximity and clearance reports.
MOPA_D void wave_argmin(double &bd, int &bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
}
// the rest of report row s ([K] entries of `pair` and `dist`) from entry `from` on is unused: pair -1, distance kFar
MOPA_D void row_fill_unused(int32_t *__restrict__ pair, double *__restrict__ dist, long long s, int K, int from, int lane) {
    for (int i = from + lane; i < K; i += 64) {
        pair[s * K + i] = -1;
        dist[s * K + i] = kFar;
    }
}

struct LdsView {
    const double *dbl;   // shared scene doubles
    const int *ints;     // shared scene ints
    double *grec;        // per-wave posed records of moving geoms [nmg*kGeomStride]
    double *qbuf;        // per-wave joint values: [na active][n_pq passive]
    double *sc;          // per-wave [nmj][2]: sin, cos of half the angle of every moving hinge joint of the state in qbuf
    unsigned short *wl;  // per-wave worklist [npair]
};

MOPA_D void stage_scene(const SceneHdr &h, const double *g_dbl, const int32_t *g_int, double *s_dbl, int *s_int) {
    for (int i = threadIdx.x; i < h.n_dbl; i += blockDim.x) s_dbl[i] = g_dbl[i];
    for (int i = threadIdx.x; i < h.n_int; i += blockDim.x) s_int[i] = g_int[i];
    __syncthreads();
}

// What k_is_valid_v5 reads out of LDS on a baked scene, in the places stage_scene puts it (so LdsView and the header's offsets serve
// unchanged): the walk and pass A run on literals, which leaves the geom records and types, the moving geoms' geom ids (v5_flush,
// v5_load_rec2) and word 7 of every pair-table entry (pass A's broadcast, v5_flush).  Everything else in the blobs stays uncopied --
// about a third of stage_scene's bytes on Push, before a workgroup's first tile.  Ends with __syncthreads(), as stage_scene does.
MOPA_D void stage_scene_k1_baked(const SceneHdr &h, const double *g_dbl, const int32_t *g_int, const int32_t *g_tab, double *s_dbl, int *s_int, int *s_tab) {
    for (int i = threadIdx.x; i < h.ng * kGeomStride; i += blockDim.x) s_dbl[h.o_g_rec + i] = g_dbl[h.o_g_rec + i];
    for (int i = threadIdx.x; i < h.ng; i += blockDim.x) s_int[h.o_g_type + i] = g_int[h.o_g_type + i];
    for (int i = threadIdx.x; i < h.nmg; i += blockDim.x) s_int[h.o_mg_geom + i] = g_int[h.o_mg_geom + i];
    for (int i = threadIdx.x; i < h.n_gp; i += blockDim.x) s_tab[8 * i + 7] = g_tab[8 * i + 7];
    __syncthreads();
}

MOPA_D LdsView make_view(const SceneHdr &h, unsigned char *smem) {
    LdsView v;
    double *s_dbl = reinterpret_cast<double *>(smem);
    int *s_int = reinterpret_cast<int *>(s_dbl + h.n_dbl);
    int int_pad = (h.n_int + 1) & ~1;
    // (readfirstlane: the wave index is wave-uniform, but derived from threadIdx the compiler keeps it -- and every pointer
    //  computed from it -- in vector registers: two VGPRs per pointer held across the planner's non-inlined validity calls)
    unsigned char *wave_base = reinterpret_cast<unsigned char *>(s_int + int_pad) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * h.wave_bytes;
    v.dbl = s_dbl;
    v.ints = s_int;
    v.grec = reinterpret_cast<double *>(wave_base);
    v.qbuf = v.grec + h.nmg * kGeomStride;
    v.sc = v.qbuf + h.na + h.n_pq + h.na;
    v.wl = reinterpret_cast<unsigned short *>(v.sc + 2 * h.nmj);
    return v;
}
// the scene tables read where they are, in global memory, by kernels that stage nothing: no per-wave slab
MOPA_D LdsView global_view(const double *g_dbl, const int32_t *g_int) {
    LdsView v;
    v.dbl = g_dbl; v.ints = g_int; v.grec = nullptr; v.qbuf = nullptr; v.sc = nullptr; v.wl = nullptr;
    return v;
}

// posed record of geom g: moving geoms live in the wave slab, static ones in the shared blob
MOPA_D const double *geom_rec(const SceneHdr &h, const LdsView &v, int g) {
    int slot = v.ints[h.o_g_slot + g];
    return (slot >= 0) ? (v.grec + slot * kGeomStride) : (v.dbl + h.o_g_rec + g * kGeomStride);
}

// broad phase of one candidate pair: bounding spheres (plane: signed distance), then -- exactly one geom static --
// the static geom's world AABB against the moving geom's bounding sphere
MOPA_D bool pair_culled(const SceneHdr &h, const LdsView &v, int g1, int g2, const double *A, const double *B) {
    const int *I = v.ints;
    const double *D = v.dbl;
    const int t1 = I[h.o_g_type + g1];
    if (bp_cull(A, t1, D[h.o_g_rbound + g1], B, D[h.o_g_rbound + g2])) return true;
    if (t1 == G_PLANE) return false;
    const bool s1 = I[h.o_g_slot + g1] < 0, s2 = I[h.o_g_slot + g2] < 0;
    if (s1 == s2) return false;
    const int gs = s1 ? g1 : g2, gm = s1 ? g2 : g1;
    return aabb_cull(ld3((s1 ? A : B) + GO_POS), D + h.o_g_aabb + 3 * gs, ld3((s1 ? B : A) + GO_POS), D[h.o_g_rbound + gm]);
}
// pair_culled with every bound widened by `band`: no pair at distance <= band is dropped
MOPA_D bool pair_culled_band(const SceneHdr &h, const LdsView &v, int g1, int g2, const double *A, const double *B, double band) {
    const int *I = v.ints;
    const double *D = v.dbl;
    const double rba = D[h.o_g_rbound + g1], rbb = D[h.o_g_rbound + g2];
    const V3 diff = sub3(ld3(B + GO_POS), ld3(A + GO_POS));
    if (I[h.o_g_type + g1] == G_PLANE) return dot3(diff, col3(A + GO_MAT, 2)) > rbb + band;
    const double rs = rba + rbb + band;
    if (dot3(diff, diff) > rs * rs) return true;
    const bool s1 = I[h.o_g_slot + g1] < 0, s2 = I[h.o_g_slot + g2] < 0;
    if (s1 == s2) return false;
    return aabb_cull(ld3((s1 ? A : B) + GO_POS), D + h.o_g_aabb + 3 * (s1 ? g1 : g2), ld3((s1 ? B : A) + GO_POS), (s1 ? rbb : rba) + band);
}
// the two as cull callables of wave_broad_phase (by value: nothing but the band to carry)
struct CullZeroMargin {
    MOPA_D bool operator()(const SceneHdr &h, const LdsView &v, int g1, int g2, const double *A, const double *B) const { return pair_culled(h, v, g1, g2, A, B); }
};
struct CullBand {
    double band;
    MOPA_D bool operator()(const SceneHdr &h, const LdsView &v, int g1, int g2, const double *A, const double *B) const { return pair_culled_band(h, v, g1, g2, A, B, band); }
};

// Forward kinematics for the state whose joint values are in v.qbuf.
// Lane l < nmg walks the ancestor chain of moving geom l (same operation order
// as a parent-first sweep over the body tree) and writes the posed geom.
// fk_one_geom: the per-lane work for moving geom `lane` of the state in v.qbuf -> v.grec.
MOPA_D void fk_one_geom(const SceneHdr &h, const LdsView &v, int lane) {
    // Reads the PACKED per-body records (ints o_mbr: jn, jntadr, -, static-frame id, -, -, -, joint-0 word; doubles o_mbd:
    // pos[3] quat[4] axis[3] jpos[3] ref) -- two levels of dependent LDS reads per body (chain item -> record -> joint value)
    // where the separate tables needed six; the arithmetic and its order are unchanged; the pieces are mopa_fk.hpp's.
    const double *D = v.dbl;
    const int *I = v.ints;
    const int g = I[h.o_mg_geom + lane];
    const int b = I[h.o_g_mb + g];
    const int cadr = I[h.o_chain_adr + b], clen = I[h.o_chain_len + b];
    V3 pos{0.0, 0.0, 0.0};
    Q4 quat{1.0, 0.0, 0.0, 0.0};
    double mat[9];
    for (int k = 0; k < clen; k++) {
        const int body = I[h.o_chain_items + cadr + k];
        const int *r = I + h.o_mbr + 8 * body;
        const int jn = r[0], ja = r[1], w7 = r[7];
        const double *bd = D + h.o_mbd + 16 * body;
        const int jt0 = w7 & 0x7f, qsrc0 = w7 >> 8;
        if (jn == 1 && jt0 == J_FREE) {
            const double *qp = v.qbuf + qsrc0;
            fk_free_step(qp, pos, quat);
        } else if (jt0 == J_GLUE) {
            // a glued scene's carried body: the jointless step under body_a (a moving body, so k > 0: pos / quat / mat are the parent's),
            // local pose out of the state's free-joint slots
            const double *qp = v.qbuf + qsrc0;
            fk_glue_step(pos, quat, mat, qp, pos, quat);
            quat = quat_normalize(quat);
        } else {
            V3 ppos;
            Q4 pquat;
            if (k == 0) {
                const int sf = r[3];
                sf_frame_ld(h, D, sf, ppos, pquat, mat);
            } else {
                ppos = pos;
                pquat = quat;
            }
            pos = add3(ppos, mat_vec(mat, ld3(bd)));
            quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
            if (jn > 0) {
                const double dq = v.qbuf[qsrc0] - bd[13];
                apply_joint_sc(jt0, ld3(bd + 7), ld3(bd + 10), (w7 & 0x80) != 0, dq, v.sc[2 * ja], v.sc[2 * ja + 1], pos, quat);
            }
            for (int j = ja + 1; j < ja + jn; j++) {       // bodies with more than one joint: the separate joint tables
                V3 ax = ld3(D + h.o_mj_axis + 3 * j), jp = ld3(D + h.o_mj_pos + 3 * j);
                double dq = v.qbuf[I[h.o_mj_qsrc + j]] - D[h.o_mj_ref + j];
                apply_joint_sc(I[h.o_mj_type + j], ax, jp, is_zero3(jp), dq, v.sc[2 * j], v.sc[2 * j + 1], pos, quat);
            }
            quat = quat_normalize(quat);
        }
        quat2mat(mat, quat);
    }
    V3 gp;
    Q4 gq;
    fk_geom_pose(pos, quat, mat, D + h.o_mgd + 8 * lane, gp, gq);       // lpos[3] lquat[4] rbound of moving geom `lane`
    fk_geom_rec_st(v.grec + lane * kGeomStride, gp, gq, D + h.o_g_rec + g * kGeomStride);    // (the size is constant: copied from the shared record)
}
MOPA_D void wave_fk(const SceneHdr &h, const LdsView &v, int lane) {
    if (lane < h.nmg) fk_one_geom(h, v, lane);
    wave_sync();
}

// The per-state pair sweep, first half: broad phase over the scene's candidate pairs of the posed state + ballot compaction of the
// survivors into v.wl (order-preserving => the worklist stays sorted by pair type, i.e. by narrow-phase class).
// cull(h, v, g1, g2, A, B): true drops the pair (CullZeroMargin, or CullBand at a report's band).  Returns the number of survivors.
template <class Cull>
MOPA_D int wave_broad_phase(const SceneHdr &h, const LdsView &v, int lane, Cull cull) {
    const int *I = v.ints;
    int wl_count = 0;
    for (int base = 0; base < h.npair; base += 64) {
        int p = base + lane;
        bool surv = false;
        if (p < h.npair) {
            int pk = I[h.o_pairs + p];
            int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff;
            const double *A = geom_rec(h, v, g1), *B = geom_rec(h, v, g2);
            surv = !cull(h, v, g1, g2, A, B);
        }
        unsigned long long mask = __ballot(surv);
        if (surv) {
            int idx = wl_count + __popcll(mask & ((1ull << lane) - 1ull));
            v.wl[idx] = (unsigned short)p;
        }
        wl_count += __popcll(mask);
    }
    wave_sync();
    return wl_count;
}
// ... second half, as the reports run it (every survivor, no early-out): a lane per survivor, f(p, g1, g2, code) with p the device
// pair index, g1 / g2 its geoms and code its narrow-phase class
template <class F>
MOPA_D void wave_each_survivor(const SceneHdr &h, const LdsView &v, int lane, int wl_count, F f) {
    const int *I = v.ints;
    for (int base = 0; base < wl_count; base += 64) {
        const int i = base + lane;
        if (i < wl_count) {
            const int p = v.wl[i];
            const int pk = I[h.o_pairs + p];
            f(p, pk & 0xff, (pk >> 8) & 0xff, (pk >> 16) & 0xff);
        }
    }
}

// Collision sweep for the posed state.  Returns the wave-uniform verdict.
// WANT_MD: also produce the minimum distance over broad-phase survivors
// (disables the early-out so the minimum is complete).
template <bool WANT_MD, bool MESH = false>
MOPA_D bool wave_collide(const SceneHdr &h, const LdsView &v, int lane, double &min_dist) {
    const int *I = v.ints;
    // 1. broad phase
    const int wl_count = wave_broad_phase(h, v, lane, CullZeroMargin{});
    // 2. narrow phase over the survivors
    bool bad = false;
    double md = 0.0;   // deepest penetration: min(0, min over pairs)
    for (int base = 0; base < wl_count; base += 64) {
        int i = base + lane;
        if (i < wl_count) {
            int pk = I[h.o_pairs + v.wl[i]];
            int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
            const double *A = geom_rec(h, v, g1), *B = geom_rec(h, v, g2);
            if (!WANT_MD && code == PC_CONVEX) {       // verdict only: the deep-overlap shortcut may stand in for the refinement
                if (convex_pair_bad(A, I[h.o_g_type + g1], B, I[h.o_g_type + g2], h.thr)) bad = true;
            } else {
                double d = geom_dist<MESH>(code, A, I[h.o_g_type + g1], B, I[h.o_g_type + g2], v.dbl);
                if (d < md) md = d;
                if (d <= h.thr) bad = true;
            }
        }
        if (!WANT_MD && wave_any(bad)) break;
    }
    bool any_bad = wave_any(bad);
    if (WANT_MD) min_dist = wave_min(md);
    wave_sync();   // worklist / geom slab are about to be reused
    return !any_bad;
}

// sin/cos of half the joint angle for every moving hinge joint of the state in v.qbuf, one joint per lane: taken out of
// the serial walk down the kinematic chain (it is ~half of a body's critical path there).  Same arithmetic.
MOPA_D void wave_sincos_table(const SceneHdr &h, const LdsView &v, int lane) {
    for (int j = lane; j < h.nmj; j += 64) {
        double sn = 0.0, cs = 1.0;
        if (v.ints[h.o_mj_type + j] == J_HINGE) mopa_sincos(0.5 * (v.qbuf[v.ints[h.o_mj_qsrc + j]] - v.dbl[h.o_mj_ref + j]), sn, cs);
        v.sc[2 * j] = sn;
        v.sc[2 * j + 1] = cs;
    }
    wave_sync();
}

// fill v.qbuf for (env row, active vector)
MOPA_D void wave_load_state(const SceneHdr &h, const LdsView &v, int lane, const double *q_active, const double *qpos_row) {
    if (lane < h.na) v.qbuf[lane] = q_active[lane];
    else if (lane < h.na + h.n_pq) v.qbuf[lane] = qpos_row[v.ints[h.o_pq_adr + lane - h.na]];
    // models with na + n_pq > 64 loop
    for (int i = lane + 64; i < h.na + h.n_pq; i += 64)
        v.qbuf[i] = (i < h.na) ? q_active[i] : qpos_row[v.ints[h.o_pq_adr + i - h.na]];
    wave_sync();
    wave_sincos_table(h, v, lane);
}

// ---------------------------------------------------------------------------
// K1: state validity, one wave per state
// ---------------------------------------------------------------------------
template <bool WANT_MD, bool MESH>
__global__ __launch_bounds__(kBlock) void k_is_valid(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                      const double *__restrict__ q_active, const double *__restrict__ qpos_env,
                                                      long long N, long long samples_per_env, unsigned char *__restrict__ valid,
                                                      double *__restrict__ min_dist, const int *__restrict__ env_idx /* nullable: env row of every state */,
                                                      const long long *__restrict__ n_dev /* nullable: the state count lives on the device (<= N) */,
                                                      long long n_small /* with n_dev: this launch serves counts below it only (the lane-per-state launch behind it the others) */) {
    if (n_dev) {
        const long long nd = *n_dev;
        if (nd >= n_small) return;
        if (nd < N) N = nd;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long s = (long long)blockIdx.x * kWavesPerBlock + wave; s < N; s += stride) {
        long long env = env_idx ? (long long)env_idx[s] : s / samples_per_env;
        wave_load_state(h, v, lane, q_active + s * h.na, qpos_env + env * h.nq);
        wave_fk(h, v, lane);
        double md;
        bool ok = wave_collide<WANT_MD, MESH>(h, v, lane, md);
        if (lane == 0) {
            valid[s] = ok ? 1 : 0;
            if (WANT_MD) min_dist[s] = md;
        }
    }
}

// ---------------------------------------------------------------------------
// K2: discrete motion validation, one wave per segment
// ---------------------------------------------------------------------------
// --- OMPL state-space helpers, per 1-D subspace (RealVectorStateSpace(1) / SO2StateSpace) ---
MOPA_D double dist_dim(const SceneHdr &h, const LdsView &v, int a, double x, double y) {
    double d = fabs(x - y);
    if (v.ints[h.o_act_so2 + a] && d > kPi) d = 2.0 * kPi - d;
    return d;
}
MOPA_D double interp_dim(const SceneHdr &h, const LdsView &v, int a, double from, double to, double t) {
    double diff = to - from;
    if (!v.ints[h.o_act_so2 + a] || fabs(diff) <= kPi) return fma(diff, t, from);
    if (diff > 0.0) diff = 2.0 * kPi - diff; else diff = -2.0 * kPi - diff;
    double r = fma(-diff, t, from);
    if (r > kPi) r -= 2.0 * kPi; else if (r < -kPi) r += 2.0 * kPi;
    return r;
}
// CompoundStateSpace::validSegmentCount = max over subspaces of ceil(d_i / (resolution * extent_i))
MOPA_D int valid_segment_count(const SceneHdr &h, const LdsView &v, const double *qa, const double *qb) {
    int nd = 0;
    for (int a = 0; a < h.na; a++) {
        double seg = h.resolution * v.dbl[h.o_act_ext + a];
        int c = (int)ceil(dist_dim(h, v, a, qa[a], qb[a]) / seg);
        if (c > nd) nd = c;
    }
    return nd;
}

__device__ __noinline__ bool plan_state_valid_impl(const SceneHdr *hp, const double *dbl, const int *ints, double *grec,
                                                   double *qbuf, unsigned short *wl, int lane, const double *qa, const double *row);

// (two waves per SIMD: the non-inlined validity routines then save ~40 registers to scratch around every call, and it still pays:
//  wave-per-env pull-back 1.00 -> 0.81 ms per 3000 targets, wave-per-segment motion checks 46 -> 83 M motions/s)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_check_motion(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                         const double *__restrict__ qa_all, const double *__restrict__ qb_all,
                                                         const double *__restrict__ qpos_env, long long N, long long samples_per_env,
                                                         unsigned char *__restrict__ valid, int hdr_lds_off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    // the non-inlined validity routine reads the header through an LDS pointer (a pointer to the by-value kernel
    // argument would live in scratch memory)
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long s = (long long)blockIdx.x * kWavesPerBlock + wave; s < N; s += stride) {
        const double *qa = qa_all + s * h.na, *qb = qb_all + s * h.na;
        const double *row = qpos_env + (s / samples_per_env) * h.nq;
        int nd = valid_segment_count(h, v, qa, qb);
        bool ok = true;
        // k == nd is the end state (tested first, as OMPL does; also the only test when qa == qb); interior
        // states in index order -- the verdict is order independent.  One call site -> one copy of FK+collision.
        double *tst = v.qbuf + h.na + h.n_pq;   // spare [na] doubles behind the joint-value buffer
        for (int k = nd; k >= (nd > 0 ? 1 : 0) && ok; k--) {
            const double t = (nd > 0) ? (double)k / (double)nd : 1.0;
            if (lane < h.na) tst[lane] = (k == nd) ? qb[lane] : interp_dim(h, v, lane, qa[lane], qb[lane], t);
            for (int i = lane + 64; i < h.na; i += 64) tst[i] = (k == nd) ? qb[i] : interp_dim(h, v, i, qa[i], qb[i], t);
            wave_sync();
            ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row);
        }
        if (lane == 0) valid[s] = ok ? 1 : 0;
    }
}

// The same rule for the kernels that run one wave per path or query (K9, RRT*): the segment from ends[0..na) to ends[na..2 na), both
// in the wave's LDS and written by the caller just before; `tst` as above, `lh` the header copy in LDS.  The verdict is wave-uniform.
MOPA_D bool motion_valid_ends(const SceneHdr &h, const LdsView &v, const SceneHdr *lh, int lane, const double *ends, double *tst,
                              const double *row) {
    const int na = h.na;
    wave_sync();
    const int nd = __builtin_amdgcn_readfirstlane(valid_segment_count(h, v, ends, ends + na));
    bool ok = true;
    for (int k = nd; k >= (nd > 0 ? 1 : 0) && ok; k--) {
        const double t = (nd > 0) ? (double)k / (double)nd : 1.0;
        for (int i = lane; i < na; i += 64) tst[i] = (k == nd) ? ends[na + i] : interp_dim(h, v, i, ends[i], ends[na + i], t);
        wave_sync();
        ok = plan_state_valid_impl(lh, v.dbl, v.ints, v.grec, v.qbuf, v.wl, lane, tst, row);
    }
    ok = __builtin_amdgcn_readfirstlane((int)ok) != 0;
    wave_sync();
    return ok;
}

// ---------------------------------------------------------------------------
// debug kernels (parity hooks): posed geoms and per-pair distances of one state
// ---------------------------------------------------------------------------
template <bool MESH>
__global__ __launch_bounds__(kBlock) void k_debug_state(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                        const double *__restrict__ q_active, const double *__restrict__ qpos_row,
                                                        double *__restrict__ out_rec /*[ng*16]*/, double *__restrict__ out_dist /*[npair]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave != 0) return;
    wave_load_state(h, v, lane, q_active, qpos_row);
    wave_fk(h, v, lane);
    for (int g = lane; g < h.ng; g += 64) {
        const double *r = geom_rec(h, v, g);
        for (int i = 0; i < kGeomStride; i++) out_rec[g * kGeomStride + i] = (i < 15) ? r[i] : 0.0;
    }
    for (int p = lane; p < h.npair; p += 64) {
        int pk = v.ints[h.o_pairs + p];
        int g1 = pk & 0xff, g2 = (pk >> 8) & 0xff, code = (pk >> 16) & 0xff;
        const double *A = geom_rec(h, v, g1), *B = geom_rec(h, v, g2);
        double d = kFar;
        if (!pair_culled(h, v, g1, g2, A, B))
            d = geom_dist<MESH>(code, A, v.ints[h.o_g_type + g1], B, v.ints[h.o_g_type + g2], v.dbl);
        out_dist[p] = d;
    }
}
static const LdsKernels kHipLds({(const void *)k_check_motion, (const void *)k_debug_state<false>, (const void *)k_debug_state<true>});

#include "mopa_valid_v2.inc"
#include "mopa_valid_v5.inc"

// ---------------------------------------------------------------------------
// host: scene compilation (scene_build_host, k1_fingerprint, k1_baked_index)
// ---------------------------------------------------------------------------
#include "mopa_scene_build.inc"

// Host export of what K1 reads from a scene (no device needed): sizes[8] = n_dbl, n_int, n_tab (int32 words of the FP32 pair
// table + its per-geom tail), sizeof(SceneHdr), use_v5, centres in LDS, mesh pairs, nmg.  The buffers may be null (sizes only).
static int scene_k1_export(const MopaSceneDesc *desc, int glue_a, int glue_b, int64_t *sizes, double *dbl, int32_t *ints, int32_t *tab, void *hdr,
                           uint64_t *fingerprint) {
    if (!desc || !sizes) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MopaScene *S = new MopaScene();
    const int rc = scene_build_host(desc, S, glue_a, glue_b);
    if (rc != MOPA_OK) { delete S; return rc; }
    sizes[0] = (int64_t)S->h_dbl.size(); sizes[1] = (int64_t)S->h_int.size(); sizes[2] = (int64_t)S->h_gp_tab.size();
    sizes[3] = (int64_t)sizeof(SceneHdr); sizes[4] = S->k1.use_v5; sizes[5] = S->k1.v5_cen_lds ? 1 : 0; sizes[6] = S->n_mesh_gp; sizes[7] = S->hdr.nmg;
    if (dbl) std::memcpy(dbl, S->h_dbl.data(), S->h_dbl.size() * sizeof(double));
    if (ints) std::memcpy(ints, S->h_int.data(), S->h_int.size() * sizeof(int32_t));
    if (tab) std::memcpy(tab, S->h_gp_tab.data(), S->h_gp_tab.size() * sizeof(int32_t));
    if (hdr) std::memcpy(hdr, &S->hdr, sizeof(SceneHdr));
    if (fingerprint) *fingerprint = k1_fingerprint(S);
    delete S;
    return MOPA_OK;
}
extern "C" int mopa_scene_k1_export(const MopaSceneDesc *desc, int64_t *sizes, double *dbl, int32_t *ints, int32_t *tab, void *hdr,
                                    uint64_t *fingerprint) {
    return scene_k1_export(desc, -1, -1, sizes, dbl, ints, tab, hdr, fingerprint);
}
// the same export of the glued compile (mopa_scene_create_glued's host half; its refusals are this call's status codes)
extern "C" int mopa_scene_k1_export_glued(const MopaSceneDesc *desc, int32_t body_a, int32_t body_b, int64_t *sizes, double *dbl, int32_t *ints,
                                          int32_t *tab, void *hdr, uint64_t *fingerprint) {
    if (body_a < 0 || body_b < 0) return fail(MOPA_ERR_INVALID_ARG, "glue: body id out of range");
    return scene_k1_export(desc, body_a, body_b, sizes, dbl, ints, tab, hdr, fingerprint);
}

// Offsets of the header fields tools/bake_k1_scenes.py reads from an exported header (the compiler's layout, by name).
extern "C" int mopa_scene_hdr_offset(const char *field) {
    if (!field) return -1;
#define MOPA_HDR_FIELD(f_) if (!std::strcmp(field, #f_)) return (int)offsetof(SceneHdr, f_);
    MOPA_HDR_FIELD(na) MOPA_HDR_FIELD(nq) MOPA_HDR_FIELD(n_pq) MOPA_HDR_FIELD(nmb) MOPA_HDR_FIELD(nmg) MOPA_HDR_FIELD(nsf)
    MOPA_HDR_FIELD(n_save) MOPA_HDR_FIELD(n_pas_b) MOPA_HDR_FIELD(n_dbl) MOPA_HDR_FIELD(n_int) MOPA_HDR_FIELD(o_mbr) MOPA_HDR_FIELD(o_mbd)
    MOPA_HDR_FIELD(o_mgd) MOPA_HDR_FIELD(o_sf_pos) MOPA_HDR_FIELD(o_sf_quat) MOPA_HDR_FIELD(o_sf_mat) MOPA_HDR_FIELD(o_act_ref)
    MOPA_HDR_FIELD(o_pq_adr) MOPA_HDR_FIELD(o_mg_geom) MOPA_HDR_FIELD(thr)
    MOPA_HDR_FIELD(o_mb_parent) MOPA_HDR_FIELD(o_chain_adr) MOPA_HDR_FIELD(o_chain_len) MOPA_HDR_FIELD(o_chain_items) MOPA_HDR_FIELD(o_g_mb)
    MOPA_HDR_FIELD(o_mb_load) MOPA_HDR_FIELD(o_mb_save) MOPA_HDR_FIELD(pfk_maxlen) MOPA_HDR_FIELD(n_gp) MOPA_HDR_FIELD(npair) MOPA_HDR_FIELD(o_pairs)
    MOPA_HDR_FIELD(o_g_rec) MOPA_HDR_FIELD(o_g_type) MOPA_HDR_FIELD(o_g_aabb)
    MOPA_HDR_FIELD(n_pas_g) MOPA_HDR_FIELD(n_pas_lv) MOPA_HDR_FIELD(v5_ent_cap) MOPA_HDR_FIELD(o_act_so2) MOPA_HDR_FIELD(o_mj_type) MOPA_HDR_FIELD(o_mj_qsrc) MOPA_HDR_FIELD(nmj)
#undef MOPA_HDR_FIELD
    return -1;
}

// The baked walk of k_is_valid_v5 (k1_fk_baked) run on the host: each moving geom's world position and rotation matrix
namespace {
struct K1HostSink {
    double *out;   // [nmg][12]
    void operator()(int m, V3 gp, Q4 gq) {
        double *o = out + 12 * m;
        o[0] = gp.x; o[1] = gp.y; o[2] = gp.z;
        quat2mat(o + 3, gq);
    }
    void resident(int, double) {}
    void axis(int, unsigned) {}
};
// the resident pairs' distances alone (what the kernel folds into verdict and depth before pass A)
struct K1ResHostSink {
    double *out;   // [n_res]
    void operator()(int, V3, Q4) {}
    void resident(int r, double d) { out[r] = d; }
    void axis(int, unsigned) {}
};
// what pass A reads: the FP32 centres and the packed axis words, as V5FkSink leaves them in LDS
struct K1PassAHostSink {
    float *cen;       // [nmg][3]
    unsigned *axw;    // [n_ax]
    void operator()(int m, V3 gp, Q4) { cen[3 * m] = (float)gp.x; cen[3 * m + 1] = (float)gp.y; cen[3 * m + 2] = (float)gp.z; }
    void resident(int, double) {}
    void axis(int slot, unsigned word) { axw[slot] = word; }
};
// static partner K of geom slot M under the built rule (keep_new) and the bounding-radius rule (keep_old); other entries stay 2
template <class TR, int M, int K>
void k1_static_host_pair(const float *c, float hx, float hy, float hz, uint8_t *keep_new, uint8_t *keep_old) {
    if constexpr (K >= TR::nmov[M] && K < TR::nmov[M] + TR::nstat[M]) {
        keep_new[TR::padr[M] + K] = k1_static_keep<TR, M, K, k1_axis_on<TR>>(c[0], c[1], c[2], hx, hy, hz) ? 1 : 0;
        keep_old[TR::padr[M] + K] = k1_static_keep<TR, M, K, false>(c[0], c[1], c[2], 0.0f, 0.0f, 0.0f) ? 1 : 0;
    }
}
template <class TR, int M, int... K>
void k1_static_host_geom(const float *cen, const unsigned *axw, uint8_t *keep_new, uint8_t *keep_old, float *axis, std::integer_sequence<int, K...>) {
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;
    if constexpr (k1_axis_owner<TR>(M)) {
        k1_axis_unpack(axw[TR::ax_slot[M]], axis[3 * M], axis[3 * M + 1], axis[3 * M + 2]);
        k1_axis_reach<TR, M>(axw[TR::ax_slot[M]], hx, hy, hz);
    }
    (k1_static_host_pair<TR, M, K>(cen + 3 * M, hx, hy, hz, keep_new, keep_old), ...);
}
template <class TR, int... M>
void k1_static_host(int64_t n, const double *q_active, const double *qpos_env, uint8_t *keep_new, uint8_t *keep_old, float *axis, std::integer_sequence<int, M...>) {
    constexpr int n_ent = (int)(sizeof(TR::tab) / (8 * sizeof(unsigned)));
    for (int64_t s = 0; s < n; s++) {
        float cen[3 * TR::nmg];
        unsigned axw[k1_axis_words<TR> / 64 + 1] = {};
        K1PassAHostSink sink{cen, axw};
        k1_fk_baked<TR>(q_active + (size_t)s * TR::na, qpos_env + (size_t)s * TR::nq, sink, std::make_integer_sequence<int, TR::nmb>{});
        uint8_t *kn = keep_new + (size_t)s * n_ent, *ko = keep_old + (size_t)s * n_ent;
        float *a = axis + (size_t)s * 3 * TR::nmg;
        std::memset(kn, 2, n_ent); std::memset(ko, 2, n_ent);
        for (int i = 0; i < 3 * TR::nmg; i++) a[i] = -1.0f;
        (k1_static_host_geom<TR, M>(cen, axw, kn, ko, a, std::make_integer_sequence<int, TR::pnum[M]>{}), ...);
    }
}
// the production path of the baked kernel per state: the sparse walk, and the dense one over it when the state's guard flag is up
template <class TR>
void k1_fk_host(int64_t n, const double *q_active, const double *qpos_env, double *out) {
    for (int64_t s = 0; s < n; s++) {
        K1HostSink sink{out + (size_t)s * 12 * TR::nmg};
        bool trip = true;
        if constexpr (k1_sparse_on<TR>)
            trip = k1_fk_baked<TR, true>(q_active + (size_t)s * TR::na, qpos_env + (size_t)s * TR::nq, sink, std::make_integer_sequence<int, TR::nmb>{});
        if (trip) k1_fk_baked<TR>(q_active + (size_t)s * TR::na, qpos_env + (size_t)s * TR::nq, sink, std::make_integer_sequence<int, TR::nmb>{});
    }
}
// raw poses (position, quaternion) of one walk, no re-run: SPARSE with the guard's flag per state, dense with flags 0
struct K1PoseHostSink {
    double *out;   // [nmg][7]
    void operator()(int m, V3 gp, Q4 gq) { pose7_st<1>(out + 7 * m, gp, gq); }
    void resident(int, double) {}
    void axis(int, unsigned) {}
};
template <class TR, bool SPARSE>
void k1_pose_host(int64_t n, const double *q_active, const double *qpos_env, double *out, uint8_t *tripped) {
    for (int64_t s = 0; s < n; s++) {
        K1PoseHostSink sink{out + (size_t)s * 7 * TR::nmg};
        const bool trip = k1_fk_baked<TR, SPARSE>(q_active + (size_t)s * TR::na, qpos_env + (size_t)s * TR::nq, sink, std::make_integer_sequence<int, TR::nmb>{});
        if (tripped) tripped[s] = trip ? 1 : 0;
    }
}
template <class TR>
void k1_res_host(int64_t n, const double *q_active, const double *qpos_env, double *out) {
    for (int64_t s = 0; s < n; s++) {
        K1ResHostSink sink{out + (size_t)s * k1_n_res<TR>};
        k1_fk_baked<TR>(q_active + (size_t)s * TR::na, qpos_env + (size_t)s * TR::nq, sink, std::make_integer_sequence<int, TR::nmb>{});
    }
}
}  // namespace
extern "C" int mopa_k1_baked_fk_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out) {
    if (n < 0 || (n > 0 && (!q_active || !qpos_env || !out))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
#define MOPA_K1_FK_HOST(i_, T_) if (index == i_) { k1_fk_host<T_>(n, q_active, qpos_env, out); return MOPA_OK; }
    MOPA_K1_BAKED_SCENES(MOPA_K1_FK_HOST)
#undef MOPA_K1_FK_HOST
    return fail(MOPA_ERR_INVALID_ARG, "no baked scene #" + std::to_string(index));
}
// The sparse walk of baked scene #index alone, on the host: out[n][nmg][7] raw poses (position, quaternion), tripped[n] the guard's
// flag per state; no dense re-run.  mopa_k1_baked_fk_pose_host: the same layout from the dense walk (what tools/bake_k1_scenes.py
// looks for exact zeros in when it marks the sparse bodies).
extern "C" int mopa_k1_baked_fk_sparse_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out, uint8_t *tripped) {
    if (n < 0 || (n > 0 && (!q_active || !qpos_env || !out || !tripped))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
#define MOPA_K1_SPARSE_HOST(i_, T_) if (index == i_) { k1_pose_host<T_, true>(n, q_active, qpos_env, out, tripped); return MOPA_OK; }
    MOPA_K1_BAKED_SCENES(MOPA_K1_SPARSE_HOST)
#undef MOPA_K1_SPARSE_HOST
    return fail(MOPA_ERR_INVALID_ARG, "no baked scene #" + std::to_string(index));
}
extern "C" int mopa_k1_baked_fk_pose_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out) {
    if (n < 0 || (n > 0 && (!q_active || !qpos_env || !out))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
#define MOPA_K1_POSE_HOST(i_, T_) if (index == i_) { k1_pose_host<T_, false>(n, q_active, qpos_env, out, nullptr); return MOPA_OK; }
    MOPA_K1_BAKED_SCENES(MOPA_K1_POSE_HOST)
#undef MOPA_K1_POSE_HOST
    return fail(MOPA_ERR_INVALID_ARG, "no baked scene #" + std::to_string(index));
}
// The resident pairs of baked scene #index as the walk evaluates them, on the host: out[n][n_res] distances in the order of the
// traits' list; *n_res (nullable) receives the number of resident pairs (0 in a MOPA_V5_NO_RESIDENT build).
extern "C" int mopa_k1_baked_resident_host(int index, int64_t n, const double *q_active, const double *qpos_env, double *out, int32_t *n_res) {
    if (n < 0 || (n > 0 && (!q_active || !qpos_env || !out))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
#define MOPA_K1_RES_HOST(i_, T_) if (index == i_) { if (n_res) *n_res = k1_n_res<T_>; if (k1_n_res<T_> > 0) k1_res_host<T_>(n, q_active, qpos_env, out); return MOPA_OK; }
    MOPA_K1_BAKED_SCENES(MOPA_K1_RES_HOST)
#undef MOPA_K1_RES_HOST
    return fail(MOPA_ERR_INVALID_ARG, "no baked scene #" + std::to_string(index));
}

// Pass A's static partners of baked scene #index on the host, per state: keep_new / keep_old [n][n_ent] (n_ent: the table's
// entries) hold 1 / 0 for a static non-plane entry kept / culled by the built rule (axis extents, unless the build is a
// MOPA_V5_NO_AXIS_CULL one) and by the bounding-radius rule, 2 for every other entry; axis [n][nmg][3]: the unpacked |axis| of
// the axis owners as pass A reads it before the clamp, -1 for the other geoms.  *n_ent (nullable) receives the entry count.
extern "C" int mopa_k1_baked_static_host(int index, int64_t n, const double *q_active, const double *qpos_env, uint8_t *keep_new, uint8_t *keep_old,
                                         float *axis, int32_t *n_ent) {
    if (n < 0 || (n > 0 && (!q_active || !qpos_env || !keep_new || !keep_old || !axis))) return fail(MOPA_ERR_INVALID_ARG, "null argument / negative count");
#define MOPA_K1_STATIC_HOST(i_, T_) if (index == i_) { if (n_ent) *n_ent = (int32_t)(sizeof(T_::tab) / (8 * sizeof(unsigned))); \
        k1_static_host<T_>(n, q_active, qpos_env, keep_new, keep_old, axis, std::make_integer_sequence<int, T_::nmg>{}); return MOPA_OK; }
    MOPA_K1_BAKED_SCENES(MOPA_K1_STATIC_HOST)
#undef MOPA_K1_STATIC_HOST
    return fail(MOPA_ERR_INVALID_ARG, "no baked scene #" + std::to_string(index));
}

static int scene_create(const MopaSceneDesc *desc, int glue_a, int glue_b, MopaScene **out) {
    if (!desc || !out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MopaScene *S = new MopaScene();
    {
        const int rc = scene_build_host(desc, S, glue_a, glue_b);
        if (rc != MOPA_OK) { delete S; return rc; }
    }
    {
        // K1 on a baked scene (mopa_valid_v5_baked.inc) when the fingerprint matches; MOPA_K1_BAKED=0: always the generic kernel (A/B runs)
        const char *eb = std::getenv("MOPA_K1_BAKED");
        const uint64_t fp = k1_fingerprint(S);
        // (a glued scene's tables never equal a baked scene's: it runs the generic kernels)
        const bool allowed = !(eb && std::string(eb) == "0") && S->k1.use_v5 && S->k1.v5_cen_lds && S->n_mesh_gp == 0 && S->glue_b < 0;
        S->k1_baked = allowed ? k1_baked_index(fp) : 0;
        if (std::getenv("MOPA_DEBUG"))
            fprintf(stderr, "[mopa] scene fingerprint %016llx: k_is_valid_v5 %s%s\n", (unsigned long long)fp, S->k1_baked ? "baked #" : "generic",
                    S->k1_baked ? std::to_string(S->k1_baked).c_str() : (eb && std::string(eb) == "0" ? " (MOPA_K1_BAKED=0)" : ""));
    }
    const MopaModel &m = desc->model;
    const SceneHdr &h = S->hdr;

    // --- device upload ---
    if (const int rc = pick_device(desc->device, &S->device, "no HIP device visible: libmopa_hip has no CPU fallback")) { delete S; return rc; }
    DeviceGuard guard(S->device);      // the caller's current device is restored on every exit path
    if (!guard.ok()) { delete S; return fail(MOPA_ERR_HIP, "cannot switch to the requested HIP device"); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, S->device) == hipSuccess) S->n_cu = prop.multiProcessorCount;
    auto up = [&](void **dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e1 = up((void **)&S->d_dbl, S->h_dbl.data(), S->h_dbl.size() * 8);
    hipError_t e2 = up((void **)&S->d_int, S->h_int.data(), S->h_int.size() * 4);
    if (e2 == hipSuccess) e2 = up((void **)&S->d_gp_tab, S->h_gp_tab.data(), S->h_gp_tab.size() * 4);
    if (e2 == hipSuccess) e2 = up((void **)&S->d_pair_model, S->pair_model.data(), S->pair_model.size() * 4);
    if (e2 == hipSuccess) e2 = up((void **)&S->d_pair_slot, S->pair_slot.data(), S->pair_slot.size() * 4);
    S->dbg_doubles = (size_t)kGeomStride * m.ngeom + (size_t)h.npair + 8;
    hipError_t e3 = hipMalloc((void **)&S->d_q, sizeof(double) * (size_t)(m.nq + S->na + 8));
    hipError_t e4 = hipMalloc((void **)&S->d_valid, 8);
    hipError_t e5 = hipMalloc((void **)&S->d_md, 8);
    hipError_t e6 = hipMalloc((void **)&S->d_dbg, sizeof(double) * S->dbg_doubles);
    for (hipError_t e : {e1, e2, e3, e4, e5, e6})
        if (e != hipSuccess) { mopa_scene_destroy(S); return fail(MOPA_ERR_HIP, std::string("device allocation: ") + hipGetErrorString(e)); }
    // allow the dynamic LDS size
    // the attribute is per function, not per scene: register the device maximum once so scenes of different sizes can
    // coexist in one process in any creation order (each launch still passes its own, checked, size)
    for (const void *k : lds_kernels())
        if (k) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    *out = S;
    return MOPA_OK;
}
extern "C" int mopa_scene_create(const MopaSceneDesc *desc, MopaScene **out) { return scene_create(desc, -1, -1, out); }
extern "C" int mopa_scene_create_glued(const MopaSceneDesc *desc, int32_t body_a, int32_t body_b, MopaScene **out) {
    if (body_a < 0 || body_b < 0) return fail(MOPA_ERR_INVALID_ARG, "glue: body id out of range");
    return scene_create(desc, body_a, body_b, out);
}

extern "C" void mopa_scene_destroy(MopaScene *S) {
    if (!S) return;
    DeviceGuard guard(S->device);
    (void)hipDeviceSynchronize();      // nothing of this scene may still be running when its tables go away
    for (void *q : {(void *)S->d_dbl, (void *)S->d_int, (void *)S->d_q, (void *)S->d_valid, (void *)S->d_md, (void *)S->d_dbg, (void *)S->d_gp_tab, (void *)S->d_pair_model, (void *)S->d_pair_slot})
        if (q) (void)hipFree(q);
    for (auto &kv : S->scratch) {
        StreamScratch &sc = kv.second;
        for (DevBuf *b : {&sc.slab, &sc.mpr, &sc.cen, &sc.mesh_list, &sc.mesh_rows, &sc.mv_cnt, &sc.mv_off, &sc.mv_env, &sc.mv_q, &sc.mv_valid, &sc.mv_scan, &sc.mr_fbq, &sc.mc_d, &sc.mc_p, &sc.plan_q,
                          &sc.plan_p, &sc.plan_ctr, &sc.pb_small, &sc.pb_rows, &sc.pb_act, &sc.ip_walk, &sc.ct_valid, &sc.ct_md, &sc.ct_ctr, &sc.star_tree, &sc.star_k, &sc.race_rec, &sc.race_word, &sc.glue_rows})
            if (b->p) (void)hipFree(b->p);
    }
    for (void *q : S->retired) (void)hipFree(q);
    delete S;
}

extern "C" int mopa_scene_num_active(const MopaScene *S) { return S ? S->na : -1; }
extern "C" int mopa_scene_active_idx(const MopaScene *S, int32_t *out) {
    if (!S || !out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    std::memcpy(out, S->active_idx.data(), sizeof(int32_t) * S->na);
    return MOPA_OK;
}
extern "C" int mopa_scene_num_pairs(const MopaScene *S) { return S ? S->hdr.npair : -1; }
extern "C" int mopa_scene_lds_bytes(const MopaScene *S) { return S ? S->lds_bytes : -1; }

extern "C" int mopa_scene_k1_baked(const MopaScene *S) { return S ? S->k1_baked : -1; }

static int grid_for(const MopaScene *S, int64_t N) {
    int64_t blocks = (N + kWavesPerBlock - 1) / kWavesPerBlock;
    int64_t cap = (int64_t)S->n_cu * 8;
    return (int)std::max<int64_t>(1, std::min(blocks, cap));
}
// ... and of the persistent report kernels (k_contact_rows, k_proximity_rows, k_clearance_states: two waves per SIMD, i.e. two
// workgroups per CU are resident), which pull their n work items from a counter
static int64_t report_blocks(const MopaScene *S, int64_t n) {
    return std::max<int64_t>(1, std::min<int64_t>((n + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)S->n_cu * 2));
}
// The reports' shared argument rules.  A batch of states or segments:
static int state_batch_rule(int64_t N, int64_t samples_per_env) {
    if (N < 0 || samples_per_env <= 0) return fail(MOPA_ERR_INVALID_ARG, "N < 0 or samples_per_env <= 0");
    return MOPA_OK;
}
// a scene created with pair_cull_radius serves a report only where its pair list is proven (`needs`: what is asked beyond that)
static int refuse_pruned(const char *needs) {
    return fail(MOPA_ERR_UNSUPPORTED, std::string("a scene with pair_cull_radius is proven down to its contact_threshold only: ") + needs + " the full scene");
}
// the per-wave distance arrays of k_contact_rows / k_proximity_rows ([npair_model] doubles each) behind the scene's LDS: their
// byte offset and the launch's LDS size
static int pair_dist_lds(const MopaScene *S, const char *what, int *pd_off, size_t *lds) {
    *pd_off = (S->lds_bytes + 15) & ~15;
    *lds = (size_t)*pd_off + (size_t)kWavesPerBlock * S->npair_model * sizeof(double);
    if (*lds > (size_t)kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, std::string(what) + ": the per-wave distance arrays do not fit LDS");
    return MOPA_OK;
}

// glue_bodies: k_glue_attach / k_glue_rows, mopa_glue_attach_batch / mopa_glue_rows_batch / mopa_scene_glue, MOPA_REFUSE_GLUED
#include "mopa_glue.inc"

// K1 host side: thresholds, kernel table, k1_plan, launch_is_valid, mopa_is_valid_batch, mopa_scene_valid_kernel
#include "mopa_valid_launch.inc"

#include "mopa_motion.inc"

extern "C" int mopa_check_motion_batch(MopaScene *S, const double *qa, const double *qb, const double *qpos_env, int64_t N,
                                       int64_t samples_per_env, uint8_t *valid, void *stream) {
    if (!S || !valid || (N > 0 && (!qa || !qb || !qpos_env))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (const int rc = state_batch_rule(N, samples_per_env)) return rc;
    if (N == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    hipStream_t st = (hipStream_t)stream;
    if (S->glue_b >= 0) {       // glued scene: every env row attaches at its own joint values
        const int rc = glue_attach_scratch(S, qpos_env, (N + samples_per_env - 1) / samples_per_env, st, &qpos_env);
        if (rc) return rc;
    }
    // large batches: expand every segment into its states, validate them with the lane-per-state kernel, AND per segment
    if (S->k1.use_v2 && N >= k1_motion_expand_min(S)) return motion_expanded(S, qa, qb, qpos_env, N, samples_per_env, valid, st);
    dim3 grid(grid_for(S, N)), block(kBlock);
    const int hdr_off = (S->lds_bytes + 15) & ~15;
    if (hdr_off + (int)sizeof(SceneHdr) > kMaxLdsBytes) return fail(MOPA_ERR_LIMIT, "motion validation LDS does not fit");
    hipLaunchKernelGGL(k_check_motion, grid, block, hdr_off + sizeof(SceneHdr), st, S->hdr, S->d_dbl, S->d_int, qa, qb, qpos_env,
                       (long long)N, (long long)samples_per_env, valid, hdr_off);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

// the active entries of a full qpos
static std::vector<double> active_of(const MopaScene *S, const double *qpos_host) {
    std::vector<double> act(S->na);
    for (int a = 0; a < S->na; a++) act[a] = qpos_host[S->active_idx[a]];
    return act;
}
// split a full qpos into (active vector, env row) on the scene's scratch
static int upload_state(MopaScene *S, const double *qpos_host) {
    std::vector<double> buf(qpos_host, qpos_host + S->nq);
    const std::vector<double> act = active_of(S, qpos_host);
    buf.insert(buf.end(), act.begin(), act.end());
    HIP_TRY(hipMemcpy(S->d_q, buf.data(), sizeof(double) * buf.size(), hipMemcpyHostToDevice));
    return MOPA_OK;
}

extern "C" int mopa_is_valid_state(MopaScene *S, const double *qpos_host, int32_t *valid_out, double *min_dist_out) {
    if (!S || !qpos_host || !valid_out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    rc = mopa_is_valid_batch(S, S->d_q + S->nq, S->d_q, 1, 1, S->d_valid, min_dist_out ? S->d_md : nullptr, nullptr);
    if (rc) return rc;
    uint8_t v = 0;
    HIP_TRY(hipMemcpy(&v, S->d_valid, 1, hipMemcpyDeviceToHost));
    if (min_dist_out) HIP_TRY(hipMemcpy(min_dist_out, S->d_md, 8, hipMemcpyDeviceToHost));
    *valid_out = v;
    return MOPA_OK;
}

static int run_debug(MopaScene *S, const double *qpos_host) {
    ON_DEVICE(S->device);
    int rc = upload_state(S, qpos_host);
    if (rc) return rc;
    const double *row = S->d_q;
    if (S->glue_b >= 0) {       // glued scene: the state attaches at its own joint values, as in mopa_is_valid_state
        rc = glue_attach_scratch(S, S->d_q, 1, nullptr, &row);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(S->hdr.has_mesh ? k_debug_state<true> : k_debug_state<false>, dim3(1), dim3(kBlock), S->lds_bytes, nullptr, S->hdr, S->d_dbl, S->d_int, S->d_q + S->nq,
                       row, S->d_dbg, S->d_dbg + (size_t)kGeomStride * S->hdr.ng);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return MOPA_OK;
}

extern "C" int mopa_debug_fk(MopaScene *S, const double *qpos_host, double *gpos, double *gmat) {
    if (!S || !qpos_host || !gpos || !gmat) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    int rc = run_debug(S, qpos_host);
    if (rc) return rc;
    ON_DEVICE(S->device);
    std::vector<double> rec((size_t)kGeomStride * S->hdr.ng);
    HIP_TRY(hipMemcpy(rec.data(), S->d_dbg, rec.size() * 8, hipMemcpyDeviceToHost));
    for (int g = 0; g < S->hdr.ng; g++) {
        std::memcpy(gpos + 3 * g, &rec[(size_t)kGeomStride * g + GO_POS], 24);
        std::memcpy(gmat + 9 * g, &rec[(size_t)kGeomStride * g + GO_MAT], 72);
    }
    return MOPA_OK;
}

extern "C" int mopa_debug_pair_dist(MopaScene *S, const double *qpos_host, double *dist) {
    if (!S || !qpos_host || !dist) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    int rc = run_debug(S, qpos_host);
    if (rc) return rc;
    ON_DEVICE(S->device);
    std::vector<double> d(S->hdr.npair);
    if (!d.empty()) HIP_TRY(hipMemcpy(d.data(), S->d_dbg + (size_t)kGeomStride * S->hdr.ng, d.size() * 8, hipMemcpyDeviceToHost));
    for (int p = 0; p < S->npair_model; p++) dist[p] = (S->pair_slot[p] >= 0) ? d[S->pair_slot[p]] : MOPA_FAR;
    return MOPA_OK;
}

extern "C" const char *mopa_planner_status(const MopaScene *S) { return S ? S->status.c_str() : "none"; }

// batched contact report: mopa_contacts_batch / mopa_contacts_state
#include "mopa_contacts.inc"
// contact frames behind it: mopa_contact_frames_batch / _state, pair level mopa_geom_frames_batch / _host
#include "mopa_contact_frames.inc"
#include "mopa_contact_manifold.inc"
// proximity report: k_proximity_rows, mopa_proximity_batch / _state, pair level mopa_geom_sep_batch / _host
#include "mopa_proximity.inc"
// witness points behind its exact route: k_proximity_witness, mopa_proximity_witness_batch / _state, pair level mopa_geom_witness_batch / _host
#include "mopa_proximity_witness.inc"
// K2 motion report: k_motion_report / k_motion_report_reduce, mopa_motion_report_batch / mopa_motion_report
#include "mopa_motion_report.inc"
// K2 clearance report: k_clearance_states / k_motion_clearance_reduce, mopa_motion_clearance_batch / mopa_motion_clearance
#include "mopa_motion_clearance.inc"

// The planner entry points are defined in mopa_planner.inc (K3).
#include "mopa_planner.inc"
#include "mopa_pullback.inc"
// K9: path simplification, one kernel body at three levels -- the vertex-removing passes (k_simplify_paths, mopa_simplify_paths_batch),
// shortcutPath in front of them (k_shortcut_paths, mopa_shortcut_paths_batch), smoothBSpline between the two (k_smooth_paths,
// mopa_smooth_paths_batch); behind the planner, whose multi-state validity pass the smoothing uses
#include "mopa_k9.inc"
// K3b: RRT*, the reference's other planner algorithm (k_rrt_star, mopa_plan_star_batch); the K9 kernels' shape
#include "mopa_rrtstar.inc"
// ... under the maximize-min-clearance objective (k_rrt_star_clear, mopa_plan_star_clearance_batch): a kernel of its own next to it
#include "mopa_rrtstar_clear.inc"
#include "mopa_ik.inc"
#include "mopa_paths.inc"
