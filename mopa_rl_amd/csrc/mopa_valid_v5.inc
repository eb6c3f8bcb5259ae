// mopa_valid_v5.inc -- K1, lane-per-state kernel, third generation: the broad phase runs out of LDS in FP32.
// (included by mopa_hip.hip after mopa_valid_v2.inc; shares V2BodyI/V2GeomI records, f64_sortable and geom_dist)
//
// Knock-out measurements of k_is_valid_v2 on the bench batch (1 048 576 states, 1.35 ms): forward kinematics
// 0.26 ms, cull + queue push 0.66 ms, narrow phase 0.42 ms.  The cull loop -- 250 candidate pairs per state --
// cost ~700 cycles per pair for ~15 arithmetic instructions: every iteration waited for two dependent scalar
// loads (pair word -> partner record) or for the partner's centre from the pose slab in global memory.  Here
//   phase 1  FK per lane as before; every moving geom's pose goes to the wave's slab (global, L2 resident) and its
//            CENTRE, rounded to FP32, to LDS ([geom][3][64 lanes]);
//   phase 2  per geom: all its candidate pairs are tested in one branch-free loop against an FP32 pair table
//            staged in LDS (partner centre / radius / world AABB for static partners, slot for moving ones) --
//            no stores, no dependent global loads, so the loop pipelines -- leaving a survivor bit per pair;
//            the bits are then turned into queue entries (ballot + prefix popcount).  An entry is 8 bytes
//            (lane, pair word, slots); the narrow phase gathers the two FP64 poses from the slab itself.
// The FP32 tests are conservative (radii inflated by 2e-5 m >> the rounding of metre-scale coordinates): a pair
// culled here is separated, a pair kept is evaluated by the same FP64 narrow phase as everywhere else, and both
// the verdict (dist <= threshold < 0) and the reported depth min(0, dist) are unaffected by WHICH separated pairs
// were culled -- results stay bit-identical to the CPU checker (tests/test_gpu_parity.py).

constexpr int kEntCapV5Max = 1024;  // survivor entries buffered per tile before a drain (4 bytes each); the actual
                                    // capacity h.v5_ent_cap is chosen per scene so that two workgroups fit one CU's LDS
constexpr int kBatCapV5 = 128;     // same-class batch ring
constexpr int kMprCapV5 = 128;     // per-wave ring of cylinder pairs waiting for the portal refinement (global memory)
constexpr int kMprRow = 32;        // doubles per row: geom 1 record[15], geom 2 record[15], state index, types
constexpr float kCullEps = 2.0e-5f;

// Image of a pair distance for the depth minimum (atomicMin over f64_sortable images).  A NaN distance -- a state with a non-finite
// joint value -- takes ONE image, that of the negative quiet NaN, below every number's: such a state's depth is then a NaN whatever
// sign its NaNs carry.  Left to f64_sortable a negative NaN is the smallest image and a positive one the largest, and the sign
// follows which operand of an instruction carried the NaN, which the compiler settles per instantiation: the generic and the baked
// kernel then answer differently for the same state.
MOPA_D unsigned long long v5_depth_image(double d) { return d != d ? 0x0007ffffffffffffull : f64_sortable(d); }

// Scene traits of k_is_valid_v5.  K1Generic: every scene table is read at run time (LDS / scalar loads + v_readlane
// broadcasts).  A baked scene (mopa_valid_v5_baked.inc, written by tools/bake_k1_scenes.py from the host export of a
// committed scene) carries its FP32 pair table as compile-time constants: pass A becomes straight-line compares against
// literals (no table fetch, no broadcasts, no count-driven loops) and pass B visits only the pairs some lane kept.
// mopa_scene_create launches a baked instantiation only when the scene's fingerprint (k1_fingerprint: blobs, pair table,
// header) equals the baked one -- the same bytes the constants were taken from.
struct K1Generic {
    static constexpr bool kBaked = false;
    static constexpr int n_ax = 0;
    static constexpr int kTilesPerDrain = 1;
};
#include "mopa_valid_v5_baked.inc"

// Pair drain (TR::kTilesPerDrain = 2): a wave pulls two consecutive tiles, runs walk, resident fold, pass A and pass B on each
// in turn (the "halves") and evaluates the entries of both in ONE drain -- a class batch costs the same for 3 busy lanes as for
// 64 and runs once per class present, so two tiles sharing a drain fill the batches better.  Nothing moves: the entries stay
// 4-byte words in the same buffer with their half in bit 31, the poses stay in the slab (one region per half, so the first
// half's survive until the drain), and the verdict word / depth words exist once per half.  The FP32 centre table and the axis
// words are the second half's once it has walked: v5_flush and the MPR ring read slab rows and scene tables only.
// The extra LDS words come out of the entry capacity (k1_pair_words; mopa_valid_launch.inc: k1_plan), as the axis table's do.
// MOPA_V5_TILES_PER_DRAIN=1: every scene drains tile by tile (the knock-out build of tools/k1_knock.sh).
// The depth-reporting instantiations stay at one tile per drain: 64 more depth words per wave on top of the verdict word would
// leave Push 192 entries, under the 256 the launch plan asks of a baked kernel.
#ifdef MOPA_V5_TILES_PER_DRAIN
template <class TR, bool WANT_MD> constexpr int k1_tiles_per_drain = TR::kBaked && !WANT_MD ? MOPA_V5_TILES_PER_DRAIN : 1;
#else
template <class TR, bool WANT_MD> constexpr int k1_tiles_per_drain = WANT_MD ? 1 : TR::kTilesPerDrain;
#endif
constexpr unsigned kEntHalfBit = 31;        // entry bit: the half; the table index keeps bits 16..30
// LDS words per wave that the second half's verdict word (and depth words) take out of the entry buffer: a multiple of 64
template <class TR, bool WANT_MD>
constexpr int k1_pair_words_of() {
    constexpr int T = k1_tiles_per_drain<TR, WANT_MD>;
    return T > 1 ? (((T - 1) * (2 + (WANT_MD ? 128 : 0)) + 63) & ~63) : 0;
}
template <class TR, bool WANT_MD> constexpr int k1_pair_words = k1_pair_words_of<TR, WANT_MD>();

// Resident pairs of a baked scene (TR::res, chosen by tools/bake_k1_scenes.py): moving-moving pairs of a closed-form class that
// pass A keeps in most states.  Both poses are in the owning lane's registers during the walk, so the lane evaluates the pair
// there, on full lanes, with the operands and the routine v5_flush would use (same bits) -- instead of survivor bit, entry,
// compaction, slab gather and a batch that costs the same for 3 lanes as for 64.  Pass A skips the pair's table entry.
// MOPA_V5_NO_RESIDENT: no pair is resident (the knock-out build of tools/k1_knock.sh).
constexpr int kResMax = 2;
#ifdef MOPA_V5_NO_RESIDENT
template <class TR> constexpr int k1_n_res = 0;
#else
template <class TR> constexpr int k1_n_res = TR::n_res;
#endif
template <class TR>
MOPA_HD constexpr bool k1_is_resident(int M, int K) {
    for (int r = 0; r < k1_n_res<TR>; r++)
        if (TR::res[r][0] == M && TR::res[r][1] == K) return true;
    return false;
}

// Axis extents of a baked scene (TR::ax_*, written by tools/bake_k1_scenes.py).  Pass A tests a static partner's world AABB
// against the owner's bounding radius r + hl -- a ball, where a capsule or cylinder is long and thin.  Along world axis i such
// an owner reaches r + hl |a_i| from its centre (a: its axis, the third column of its rotation; exact for a capsule, encloses
// a cylinder), so for these owners the three box tests become |d_i| > c_i' + hl a_i, c_i' = partner half extent + r + kCullEps
// (the three products once per owner, then one addition of a literal per pair and axis: gfx950 has no FMA form that takes
// two scalar constants, and constants kept in registers across the tile loop were what the allocator spilled).
// The walk forms |a_i| in FP32 from the geom quaternion and leaves it in LDS as ONE word per owner and lane, three
// magnitudes of 10 bits each (k1_axis_word), next to the centre table; pass A unpacks it once per owner.
// Conservative by construction -- the unpacked value is never below the FP64 |a_i|:
//   * a_f, the FP32 value: the quaternion rounded to FP32 (4 x 2^-24 relative), three roundings per product term, the
//     terms' magnitudes sum to <= 1  =>  |a_f - |a_i|| < 1e-6;
//   * the word holds u = ceil(1023 a_f + kAxisBias) (one FMA: t >= 1023 a_f + 0.02 - 6.2e-5), so u / 1023 >= a_f + 1.9e-5
//     > |a_i|; clipped at 1023, where u / 1023 = 1;
//   * unpacking multiplies by kAxisStep, the FP32 number just ABOVE 1/1023: u kAxisStep rounded to nearest is >= u / 1023.
// It exceeds |a_i| by less than kAxisSlack = 1e-3 (1.02 / 1023 + the 1e-6 above + two roundings): the bound is looser than
// the exact extent by at most hl kAxisSlack.  What is left for kCullEps (2e-5) is what it covers in every other test: the centres' and the
// half extents' rounding to FP32 (~1e-7 at metre scale) and the roundings of the product and the sum.  The unpacked value is
// then clamped to TR::ax_max[M], the largest FP32 a for which c_i' + hl a, in the kernel's FP32 arithmetic, stays <= the
// bounding-radius constant c_i for every static pair and axis of the owner (found by the bake script in that arithmetic;
// both operations are monotone in a): the new bound never exceeds the bounding-radius one, which stays valid on its own
// (a cylinder's bounding radius hypot(r, hl) is below r + hl), so the survivors are a subset of that rule's.
// MOPA_V5_NO_AXIS_CULL: the bounding-radius constants for every static pair, no axis table (the knock-out build of tools/k1_knock.sh).
constexpr float kAxisBias = 0.02f;
constexpr float kAxisStep = __builtin_bit_cast(float, 0x3a802009u);     // nextafter(1.0f / 1023.0f, 1.0f)
constexpr float kAxisSlack = 1.0e-3f;
#ifdef MOPA_V5_NO_AXIS_CULL
template <class TR> constexpr bool k1_axis_on = false;
#else
template <class TR> constexpr bool k1_axis_on = TR::n_ax > 0;
#endif
// moving geom slot M is a capsule or cylinder with static non-plane partners: it owns a word of the axis table
template <class TR>
MOPA_HD constexpr bool k1_axis_owner(int M) {
    if constexpr (k1_axis_on<TR>) return TR::ax_slot[M] >= 0;
    else return false;
}
// LDS words per wave of the axis table ([n_ax][64]); they are taken out of the entry buffer (mopa_valid_launch.inc: k1_plan)
template <class TR>
constexpr int k1_axis_words_of() {
    if constexpr (k1_axis_on<TR>) return TR::n_ax * 64;
    else return 0;
}
template <class TR> constexpr int k1_axis_words = k1_axis_words_of<TR>();
MOPA_HD unsigned k1_axis_q10(float a) {
    const float t = ceilf(fmaf(fabsf(a), 1023.0f, kAxisBias));
    return t < 1023.0f ? (unsigned)t : 1023u;
}
MOPA_HD unsigned k1_axis_word(const Q4 &q) {
    const float w = (float)q.w, x = (float)q.x, y = (float)q.y, z = (float)q.z;
    const float ax = 2.0f * (x * z + w * y), ay = 2.0f * (y * z - w * x), az = ((w * w - x * x) - y * y) + z * z;   // quat2mat: M[2], M[5], M[8]
    return k1_axis_q10(ax) | (k1_axis_q10(ay) << 10) | (k1_axis_q10(az) << 20);
}
MOPA_HD void k1_axis_unpack(unsigned word, float &ax, float &ay, float &az) {
    ax = (float)(word & 1023u) * kAxisStep; ay = (float)((word >> 10) & 1023u) * kAxisStep; az = (float)(word >> 20) * kAxisStep;
}
// what pass A uses of owner M's word: hl |a_i|, with the unpacked magnitudes clamped to TR::ax_max[M]
template <class TR, int M>
MOPA_HD void k1_axis_reach(unsigned word, float &hx, float &hy, float &hz) {
    constexpr float amax = __builtin_bit_cast(float, TR::ax_max[M]), hl = __builtin_bit_cast(float, TR::ax_hl[M]);
    k1_axis_unpack(word, hx, hy, hz);
    hx = hl * fminf(hx, amax); hy = hl * fminf(hy, amax); hz = hl * fminf(hz, amax);
}
// pass A's test of one static non-plane partner (entry padr[M] + K): sphere, then the partner's world AABB against the owner's
// bounding radius -- or, AXIS and the owner has an axis, against its per-axis reach ((hx, hy, hz): k1_axis_reach)
template <class TR, int M, int K, bool AXIS>
MOPA_HD bool k1_static_keep(float cx, float cy, float cz, float hx, float hy, float hz) {
    constexpr int e = TR::padr[M] + K;
    constexpr float c0 = __builtin_bit_cast(float, TR::tab[8 * e + 0]), c1 = __builtin_bit_cast(float, TR::tab[8 * e + 1]);
    constexpr float c2 = __builtin_bit_cast(float, TR::tab[8 * e + 2]), c3 = __builtin_bit_cast(float, TR::tab[8 * e + 3]);
    const float dx = cx - c0, dy = cy - c1, dz = cz - c2;
    if constexpr (AXIS && k1_axis_owner<TR>(M)) {
        constexpr float e4 = __builtin_bit_cast(float, TR::ax_tab[3 * e + 0]), e5 = __builtin_bit_cast(float, TR::ax_tab[3 * e + 1]);
        constexpr float e6 = __builtin_bit_cast(float, TR::ax_tab[3 * e + 2]);
        return !((fmaf(dz, dz, fmaf(dy, dy, dx * dx)) > c3) | (fabsf(dx) > e4 + hx) | (fabsf(dy) > e5 + hy) | (fabsf(dz) > e6 + hz));
    } else {
        constexpr float c4 = __builtin_bit_cast(float, TR::tab[8 * e + 4]), c5 = __builtin_bit_cast(float, TR::tab[8 * e + 5]);
        constexpr float c6 = __builtin_bit_cast(float, TR::tab[8 * e + 6]);
        return !((fmaf(dz, dz, fmaf(dy, dy, dx * dx)) > c3) | (fabsf(dx) > c4) | (fabsf(dy) > c5) | (fabsf(dz) > c6));
    }
}

// pass A of a baked scene, one candidate pair (entry padr[M] + K of the table): the same FP32 arithmetic and compares as
// the generic loops of k_is_valid_v5, with the table values as literals.  An inscribed-ball bound of 0 (no bound) is
// never exceeded (d2 >= 0 or NaN), so its test is left out.
template <class TR, int M, bool WANT_MD, int K>
MOPA_D void v5_cull_baked(float cx, float cy, float cz, const float *cen_lane, float hx, float hy, float hz, unsigned &surv_lo, unsigned &surv_hi,
                          unsigned long long &deep_mask, unsigned long long &any_kept) {
    if constexpr (!k1_is_resident<TR>(M, K)) {      // (a resident pair is decided by the walk: no bit, no inscribed-ball test)
    constexpr int e = TR::padr[M] + K;
    constexpr float c0 = __builtin_bit_cast(float, TR::tab[8 * e + 0]), c1 = __builtin_bit_cast(float, TR::tab[8 * e + 1]);
    constexpr float c2 = __builtin_bit_cast(float, TR::tab[8 * e + 2]), c3 = __builtin_bit_cast(float, TR::tab[8 * e + 3]);
    constexpr float c4 = __builtin_bit_cast(float, TR::tab[8 * e + 4]), c5 = __builtin_bit_cast(float, TR::tab[8 * e + 5]);
    constexpr float c6 = __builtin_bit_cast(float, TR::tab[8 * e + 6]);
    bool keep;
    if constexpr (K < TR::nmov[M]) {          // moving partner: its centre from the tile's table
        const float *pc = cen_lane + ((TR::tab[8 * e + 7] >> 14) & 0xff) * 3 * 64;
        const float dx = cx - pc[0], dy = cy - pc[64], dz = cz - pc[128];
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        if constexpr (!WANT_MD && TR::tab[8 * e + 0] != 0u) deep_mask |= __ballot(d2 < c0);
        keep = !(d2 > c3);
    } else if constexpr (K < TR::nmov[M] + TR::nstat[M]) {   // static partner: sphere, then world AABB
        keep = k1_static_keep<TR, M, K, k1_axis_on<TR>>(cx, cy, cz, hx, hy, hz);
    } else {                                  // plane: (c4, c5, c6) is the normal
        const float dx = cx - c0, dy = cy - c1, dz = cz - c2;
        keep = !(fmaf(dz, c6, fmaf(dy, c5, dx * c4)) > c3);
    }
    if constexpr (K < 32) surv_lo |= keep ? (1u << K) : 0u;
    else surv_hi |= keep ? (1u << (K - 32)) : 0u;
    any_kept |= __ballot(keep) ? (1ull << K) : 0ull;
    }
}
template <class TR, int M, bool WANT_MD, int... K>
MOPA_D void v5_pass_a_baked(float cx, float cy, float cz, const float *cen_lane, unsigned &surv_lo, unsigned &surv_hi,
                            unsigned long long &deep_mask, unsigned long long &any_kept, std::integer_sequence<int, K...>) {
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;
    if constexpr (k1_axis_owner<TR>(M))         // its word follows the centre table; unpacked once for all its static partners
        k1_axis_reach<TR, M>(reinterpret_cast<const unsigned *>(cen_lane)[(3 * TR::nmg + TR::ax_slot[M]) * 64], hx, hy, hz);
    (v5_cull_baked<TR, M, WANT_MD, K>(cx, cy, cz, cen_lane, hx, hy, hz, surv_lo, surv_hi, deep_mask, any_kept), ...);
}
// geom slot m (wave-uniform) -> its straight-line pass A
template <class TR, bool WANT_MD, int... M>
MOPA_D void v5_pass_a_dispatch(int m, float cx, float cy, float cz, const float *cen_lane, unsigned &surv_lo, unsigned &surv_hi,
                               unsigned long long &deep_mask, unsigned long long &any_kept, std::integer_sequence<int, M...>) {
    (void)((m == M ? (v5_pass_a_baked<TR, M, WANT_MD>(cx, cy, cz, cen_lane, surv_lo, surv_hi, deep_mask, any_kept,
                                                     std::make_integer_sequence<int, TR::pnum[M]>{}), true)
                   : false) || ...);
}

// Phase 1 of a baked scene: the moving-body program of the generic walk (k_is_valid_v5, phase 1) expanded body by body at
// compile time.  Every body runs the generic walk's FP64 operations on the same operands in the same order -- only the scene
// values are literals (bit patterns of the exported blobs), the branches on joint type / load slot / anchor are resolved by
// the compiler, each joint takes its own sine / cosine (no select chain) and the DFS save slots stay in registers.  All
// inputs (active values, passive coordinates) are read before the first pose leaves, so the pose stores drain under the
// rest of the walk and pass A.  `sink(m, pos, quat)` receives moving geom m's world pose.
MOPA_HD constexpr double k1_bits(unsigned long long b) { return __builtin_bit_cast(double, b); }

// Sparse form of the walk (bodies marked in TR::fk_sparse by tools/bake_k1_scenes.py).  The scene's literals are full of exact zeros
// and ones -- identity geom quaternions, local positions (0, 0, z), hinge axes (0, 0, 1), slide axes (0, -+1, 0) -- but the compiler
// may not fold x * 0.0 or fma(x, 0.0, acc) under IEEE rules, so the dense walk multiplies by them.  The sparse form drops every
// product whose constant factor is an exact zero (a literal, or the hinge quaternion's 0 * sn), turns x * (+-1) into +-x, and keeps
// the order and the fma / mul / add structure of the terms that remain.
// Lemma (finite operands, no overflow): every intermediate and every result of the sparse walk is bit-equal to the dense walk's, or
// a zero in both (possibly of different sign).  Induction over the operations: a * 0 = +-0 exactly; acc + (+-0) = acc for acc != 0
// and a zero otherwise; fma(a, b, +-0) = round(a b) whichever zero, unless a b is itself a zero; fma(a, +-1, acc) = round(acc +- a);
// products and sums of equal-or-both-zero operands are again equal-or-both-zero; quat_normalize's comparisons do not see a zero's sign.
// So a sparse result that is nonzero has the dense walk's bits, and only the sign of an exact zero is in doubt.  The guard, one flag per lane:
//   1. an active or passive input fails |x| <= 2^20 (written so that NaN fails).  Under the bound nothing overflows: every quaternion
//      the walk holds is a product of normalised ones (components <= 1 + 1e-15), matrices have entries <= 3, positions are sums of at
//      most nmb literal offsets (metres) and slide travels |dq| <= 2^20 times such entries, mopa_sincos reduces |x| <= 2^19 with
//      k <= 2^19 exactly, and the free joint's norm^2 <= 2^42: all below 2^64, far from 2^1024;
//   2. a stored pose component (3 position, 4 quaternion) of a marked body's geom is an exact zero (one compare each).
// If any lane of the wave raises its flag, the wave runs the dense walk for the tile, which overwrites everything the sparse one left
// (slab rows, FP32 centres, axis words, resident distances).  Without a flag those are the dense walk's bits already: they are
// functions of the stored poses.  The marks affect speed only (a body whose geoms have structural zeros would trip in every tile):
// the bake script marks a body only if no stored component of it or of a body below it was zero on a seeded sample, never a
// free-jointed one, and only with every body below it.  MOPA_V5_NO_SPARSE_FK: dense walk only (the knock-out build of tools/k1_knock.sh).
#ifdef MOPA_V5_NO_SPARSE_FK
template <class TR> constexpr bool k1_sparse_on = false;
#else
template <class TR> constexpr bool k1_sparse_on = true;
#endif
template <class TR>
MOPA_HD constexpr bool k1_body_sparse(int B) {
    if constexpr (k1_sparse_on<TR>) return TR::fk_sparse[B];
    else return false;
}
constexpr double kSparseInMax = 0x1p20;     // guard 1: bound on the inputs' magnitude
enum K1Term : int { KT_ZERO = 0, KT_ONE, KT_NEG, KT_GEN };   // a constant factor: +-0, 1, -1, anything else
MOPA_HD constexpr int k1_kind(unsigned long long b) {
    return (b << 1) == 0ull ? KT_ZERO : b == 0x3ff0000000000000ull ? KT_ONE : b == 0xbff0000000000000ull ? KT_NEG : KT_GEN;
}
// acc <- fma(a, b, acc) for a factor b of kind KIND; FIRST: every term before this one was dropped (the dense code's accumulator is a zero)
template <int KIND, bool FIRST>
MOPA_HD double k1_term(double acc, double a, double b) {
    if constexpr (KIND == KT_ZERO) return acc;
    else if constexpr (FIRST) return KIND == KT_ONE ? a : KIND == KT_NEG ? -a : a * b;
    else return KIND == KT_ONE ? acc + a : KIND == KT_NEG ? acc - a : fma(a, b, acc);
}
// fma(a2, b2, fma(a1, b1, a0 * b0)) / fma(a3, b3, ...) without the dropped terms (all dropped: 0)
template <int K0, int K1, int K2>
MOPA_HD double k1_chain3(double a0, double b0, double a1, double b1, double a2, double b2) {
    double acc = 0.0;
    acc = k1_term<K0, true>(acc, a0, b0);
    acc = k1_term<K1, K0 == KT_ZERO>(acc, a1, b1);
    acc = k1_term<K2, K0 == KT_ZERO && K1 == KT_ZERO>(acc, a2, b2);
    return acc;
}
template <int K0, int K1, int K2, int K3>
MOPA_HD double k1_chain4(double a0, double b0, double a1, double b1, double a2, double b2, double a3, double b3) {
    double acc = k1_chain3<K0, K1, K2>(a0, b0, a1, b1, a2, b2);
    return k1_term<K3, K0 == KT_ZERO && K1 == KT_ZERO && K2 == KT_ZERO>(acc, a3, b3);
}
// quat_mul(a, b), b's components of kinds KW KX KY KZ: the terms of quat_mul in its order
template <int KW, int KX, int KY, int KZ>
MOPA_HD Q4 k1_quat_mul_s(Q4 a, Q4 b) {
    Q4 r;
    r.w = k1_chain4<KW, KX, KY, KZ>(a.w, b.w, -a.x, b.x, -a.y, b.y, -a.z, b.z);
    r.x = k1_chain4<KX, KW, KZ, KY>(a.w, b.x, a.x, b.w, a.y, b.z, -a.z, b.y);
    r.y = k1_chain4<KY, KZ, KW, KX>(a.w, b.y, -a.x, b.z, a.y, b.w, a.z, b.x);
    r.z = k1_chain4<KZ, KY, KX, KW>(a.w, b.z, a.x, b.y, -a.y, b.x, a.z, b.w);
    return r;
}
// mat_vec(M, v), v's components of kinds KX KY KZ; matrix entries that only meet dropped terms are never read
template <int KX, int KY, int KZ>
MOPA_HD V3 k1_mat_vec_s(const double *M, V3 v) {
    return V3{k1_chain3<KX, KY, KZ>(M[0], v.x, M[1], v.y, M[2], v.z), k1_chain3<KX, KY, KZ>(M[3], v.x, M[4], v.y, M[5], v.z),
              k1_chain3<KX, KY, KZ>(M[6], v.x, M[7], v.y, M[8], v.z)};
}
// add3(p, mat_vec(M, v)); all three terms dropped: p + (+-0), a copy
template <int KX, int KY, int KZ>
MOPA_HD V3 k1_offset_s(V3 p, const double *M, V3 v) {
    if constexpr (KX == KT_ZERO && KY == KT_ZERO && KZ == KT_ZERO) return p;
    else return add3(p, k1_mat_vec_s<KX, KY, KZ>(M, v));
}
// guard 2: an exact zero among the seven stored components of a pose
MOPA_HD bool k1_zero7(const V3 &p, const Q4 &q) {
    return (p.x == 0.0) | (p.y == 0.0) | (p.z == 0.0) | (q.w == 0.0) | (q.x == 0.0) | (q.y == 0.0) | (q.z == 0.0);
}
// the flag is folded geom by geom: left to itself the compiler gathers the 63 compares at the end of the walk and keeps every pose
// they read in registers until then (256 VGPRs and spills where the walk needs 238)
MOPA_HD void k1_pin(unsigned &w) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(w));
#else
    (void)w;
#endif
}

template <class TR>
struct K1FkRegs {
    V3 pos;
    Q4 quat;
    double mat[9];
    unsigned trip;             // sparse walk: the lane's guard flag (0 / 1)
    V3 save_pos[TR::n_save];
    Q4 save_quat[TR::n_save];
    V3 res_pos[kResMax];       // resident pair r: what its routine needs of the geom posed first -- the centre,
    Q4 res_quat[kResMax];      // and for a capsule the quaternion
};
// posed record of one geom of a resident pair, as v5_load_rec2 builds it from the slab: position, quat2mat of the geom
// quaternion, sizes.  (A sphere's matrix is read by none of the resident classes' routines: left zero, its quaternion is not kept.)
template <int TYPE>
MOPA_HD void k1_res_rec(double (&R)[15], const V3 &p, const Q4 &q, const unsigned long long *size) {
    R[GO_POS] = p.x; R[GO_POS + 1] = p.y; R[GO_POS + 2] = p.z;
    if constexpr (TYPE != G_SPHERE) {
        quat2mat(R + GO_MAT, q);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) R[GO_MAT + i] = 0.0;
    }
    R[GO_SIZE] = k1_bits(size[0]); R[GO_SIZE + 1] = k1_bits(size[1]); R[GO_SIZE + 2] = k1_bits(size[2]);
}
// moving geom M has its pose: the first geom of resident pair R is kept, the second one completes the pair -> `sink.resident(R, dist)`
template <class TR, int M, int R, class Sink>
MOPA_HD void k1_fk_resident(K1FkRegs<TR> &r, const V3 &gp, const Q4 &gq, Sink &sink) {
    constexpr int sa = TR::res[R][2], sb = TR::res[R][3], code = TR::res[R][4], ta = TR::res[R][5], tb = TR::res[R][6];
    static_assert(sa != sb && ta <= tb && (code == PC_SPHERE_SPHERE || code == PC_SPHERE_CAPSULE || code == PC_CAPSULE_CAPSULE),
                  "resident pair: two geoms in routine order, closed-form class");
    constexpr bool a_first = sa < sb;           // (the walk poses the moving geoms in slot order)
    if constexpr (M == (a_first ? sa : sb)) {
        r.res_pos[R] = gp;
        if constexpr ((a_first ? ta : tb) != G_SPHERE) r.res_quat[R] = gq;
        else r.res_quat[R] = Q4{1.0, 0.0, 0.0, 0.0};
    } else if constexpr (M == (a_first ? sb : sa)) {
        double R1[15], R2[15];
        k1_res_rec<ta>(R1, a_first ? r.res_pos[R] : gp, a_first ? r.res_quat[R] : gq, TR::res_size[R]);
        k1_res_rec<tb>(R2, a_first ? gp : r.res_pos[R], a_first ? gq : r.res_quat[R], TR::res_size[R] + 3);
        sink.resident(R, geom_dist<false>(code, R1, ta, R2, tb));
    }
}
template <class TR, int M, class Sink, int... R>
MOPA_HD void k1_fk_residents(K1FkRegs<TR> &r, const V3 &gp, const Q4 &gq, Sink &sink, std::integer_sequence<int, R...>) {
    (k1_fk_resident<TR, M, R>(r, gp, gq, sink), ...);
}
// SP: the sparse form (its body is marked and the walk is the sparse one)
template <class TR, int M, bool SP, class Sink>
MOPA_HD void k1_fk_geom(K1FkRegs<TR> &r, Sink &sink) {
    constexpr const unsigned long long *gd = TR::fk_gd[M];   // lpos[3] lquat[4]
    const V3 lp{k1_bits(gd[0]), k1_bits(gd[1]), k1_bits(gd[2])};
    const Q4 lq{k1_bits(gd[3]), k1_bits(gd[4]), k1_bits(gd[5]), k1_bits(gd[6])};
    V3 gp;
    Q4 gq;
    if constexpr (SP) {
        gp = k1_offset_s<k1_kind(gd[0]), k1_kind(gd[1]), k1_kind(gd[2])>(r.pos, r.mat, lp);
        gq = k1_quat_mul_s<k1_kind(gd[3]), k1_kind(gd[4]), k1_kind(gd[5]), k1_kind(gd[6])>(r.quat, lq);
        r.trip |= k1_zero7(gp, gq) ? 1u : 0u;
        k1_pin(r.trip);
    } else {
        gp = add3(r.pos, mat_vec(r.mat, lp));
        gq = quat_mul(r.quat, lq);
    }
    sink(M, gp, gq);
    if constexpr (k1_axis_owner<TR>(M)) sink.axis(TR::ax_slot[M], k1_axis_word(gq));
    k1_fk_residents<TR, M>(r, gp, gq, sink, std::make_integer_sequence<int, k1_n_res<TR>>{});
}
template <class TR, int B, bool SPARSE, class Sink, int... G>
MOPA_HD void k1_fk_body(K1FkRegs<TR> &r, const double *qact, const double *sn, const double *cs, const double *pv, Sink &sink,
                        std::integer_sequence<int, G...>) {
    constexpr const int *bi = TR::fk_body[B];                // load, static frame, save, first geom, geoms, joints, type, anchor 0, value slot
    constexpr int load = bi[0], sf = bi[1], save = bi[2], mgadr = bi[3], jn = bi[5], jt = bi[6], src = bi[8];
    constexpr bool jp0 = bi[7] != 0;
    constexpr const unsigned long long *bd = TR::fk_bd[B];   // pos[3] quat[4] axis[3] jpos[3] ref
    static_assert(jn <= 1 && sizeof...(G) == bi[4], "baked walk: one joint per body at most");
    constexpr bool SP = SPARSE && k1_body_sparse<TR>(B) && !(jn == 1 && jt == J_FREE);
    if constexpr (jn == 1 && jt == J_FREE) {
        fk_free_step(pv + (src - TR::na), r.pos, r.quat);
    } else {
        V3 ppos;
        Q4 pquat;
        if constexpr (load == -2) {
            constexpr const unsigned long long *f = TR::fk_sf[sf];   // pos[3] quat[4] mat[9]
            ppos = V3{k1_bits(f[0]), k1_bits(f[1]), k1_bits(f[2])};
            pquat = Q4{k1_bits(f[3]), k1_bits(f[4]), k1_bits(f[5]), k1_bits(f[6])};
#pragma unroll
            for (int i = 0; i < 9; i++) r.mat[i] = k1_bits(f[7 + i]);
        } else if constexpr (load >= 0) {
            ppos = r.save_pos[load];
            pquat = r.save_quat[load];
            quat2mat(r.mat, pquat);
        } else {
            ppos = r.pos;
            pquat = r.quat;
        }
        const V3 bp{k1_bits(bd[0]), k1_bits(bd[1]), k1_bits(bd[2])};
        const Q4 bq{k1_bits(bd[3]), k1_bits(bd[4]), k1_bits(bd[5]), k1_bits(bd[6])};
        if constexpr (SP) {
            r.pos = k1_offset_s<k1_kind(bd[0]), k1_kind(bd[1]), k1_kind(bd[2])>(ppos, r.mat, bp);
            r.quat = k1_quat_mul_s<k1_kind(bd[3]), k1_kind(bd[4]), k1_kind(bd[5]), k1_kind(bd[6])>(pquat, bq);
        } else {
            r.pos = add3(ppos, mat_vec(r.mat, bp));
            r.quat = quat_mul(pquat, bq);
        }
        if constexpr (jn == 1) {
            const V3 ax{k1_bits(bd[7]), k1_bits(bd[8]), k1_bits(bd[9])}, jp{k1_bits(bd[10]), k1_bits(bd[11]), k1_bits(bd[12])};
            constexpr double ref = k1_bits(bd[13]);
            constexpr int kax = k1_kind(bd[7]), kay = k1_kind(bd[8]), kaz = k1_kind(bd[9]);
            if constexpr (SP && jt == J_HINGE && jp0 && kax == KT_ZERO && kay == KT_ZERO && kaz == KT_ONE) {
                // axis (0, 0, 1): apply_joint_sc's ql = (cs, 0 sn, 0 sn, 1 sn) = (cs, +-0, +-0, sn)
                double s1, c1;
                if constexpr (src < TR::na) { s1 = sn[src]; c1 = cs[src]; }
                else mopa_sincos(0.5 * (pv[src - TR::na] - ref), s1, c1);
                r.quat = k1_quat_mul_s<KT_GEN, KT_ZERO, KT_ZERO, KT_GEN>(r.quat, Q4{c1, 0.0, 0.0, s1});
            } else if constexpr (SP && jt == J_SLIDE) {
                // apply_joint_sc's slide: with an axis-aligned axis one column of the matrix survives
                double dq;
                if constexpr (src < TR::na) dq = qact[src] - ref;
                else dq = pv[src - TR::na] - ref;
                double jm[9];
                quat2mat(jm, r.quat);
                r.pos = addscl3(r.pos, k1_mat_vec_s<kax, kay, kaz>(jm, ax), dq);
            } else {
                if constexpr (src < TR::na) apply_joint_sc(jt, ax, jp, jp0, qact[src] - ref, sn[src], cs[src], r.pos, r.quat);
                else apply_joint(jt, ax, jp, jp0, pv[src - TR::na] - ref, r.pos, r.quat);
            }
        }
        r.quat = quat_normalize(r.quat);
    }
    quat2mat(r.mat, r.quat);
    if constexpr (save >= 0) {
        r.save_pos[save] = r.pos;
        r.save_quat[save] = r.quat;
    }
    (k1_fk_geom<TR, mgadr + G, SP>(r, sink), ...);
}
// SPARSE: marked bodies take their sparse form; returns the lane's guard flag (the caller re-runs the dense walk, SPARSE = false,
// when it is set; the dense walk returns false)
// QP: pointer to the input rows (const double *; the kernel's cold walk passes its laundered rows typed as global memory)
template <class TR, bool SPARSE = false, class QP, class Sink, int... B>
MOPA_HD bool k1_fk_baked(QP qa_row, QP env_row, Sink &sink, std::integer_sequence<int, B...>) {
    static_assert(TR::na <= 8 && TR::n_pq >= 1 && TR::n_save >= 1, "baked walk: at most 8 active values; array sizes padded to 1");
    static_assert(TR::n_res <= kResMax, "baked walk: at most kResMax resident pairs");
    double qact[TR::na], pv[TR::n_pq], sn[TR::na], cs[TR::na];
#pragma unroll
    for (int a = 0; a < TR::na; a++) qact[a] = qa_row[a];
#pragma unroll
    for (int k = 0; k < TR::n_pq; k++) pv[k] = env_row[TR::fk_pq_adr[k]];
    // half-angle sine / cosine of every active value up front, as in the generic walk (same function, same argument)
#pragma unroll
    for (int a = 0; a < TR::na; a++) mopa_sincos(0.5 * (qact[a] - k1_bits(TR::fk_act_ref[a])), sn[a], cs[a]);
    K1FkRegs<TR> r;
    r.pos = V3{0.0, 0.0, 0.0};
    r.quat = Q4{1.0, 0.0, 0.0, 0.0};
    r.trip = 0u;
    if constexpr (SPARSE) {
#pragma unroll
        for (int a = 0; a < TR::na; a++) r.trip |= !(fabs(qact[a]) <= kSparseInMax) ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < TR::n_pq; k++) r.trip |= !(fabs(pv[k]) <= kSparseInMax) ? 1u : 0u;
        k1_pin(r.trip);
    }
    (k1_fk_body<TR, B, SPARSE>(r, qact, sn, cs, pv, sink, std::make_integer_sequence<int, TR::fk_body[B][4]>{}), ...);
    return r.trip != 0u;
}
// the kernel's sink: pose -> the geom's slab row, FP32 centre -> the tile's centre table in LDS (what pass A, v5_flush and the
// MPR ring read, exactly as the generic walk writes them)
// COLD: the dense walk behind the sparse one's guard.  Each geom's slab address passes through an empty asm: in that rarely run
// block the compiler otherwise forms all the rows' addresses up front and spills VGPRs to hold them.
// The slab pointer is typed as global memory: an empty asm hides where a pointer came from, and through a generic pointer every pose
// store is a FLAT instruction -- issued to the LDS queue as well, counted in lgkmcnt, and every LDS wait behind one becomes
// lgkmcnt(0).  The type survives the asm, so the 98 stores of a walk are global_store and pass A's first centre read waits for LDS only.
#ifdef MOPA_V5_FLAT_SLAB      // knock-out (tools/k1_knock.sh flatslab): generic pointers, as before
typedef double k1_gdouble;
typedef const double k1_gcdouble;
#else
typedef __attribute__((address_space(1))) double k1_gdouble;
typedef const __attribute__((address_space(1))) double k1_gcdouble;
#endif
template <bool COLD>
struct V5FkSinkT {
    k1_gdouble *slab;   // this lane's place in the wave's slab
    float *cen;     // this lane's place in the centre table
    MOPA_D void operator()(int m, V3 gp, Q4 gq) {
        k1_gdouble *sp = slab + (size_t)m * kSlabStride;
        if constexpr (COLD) asm volatile("" : "+v"(sp));
        // (pose7_st<64>, through the typed pointer)
        sp[0] = gp.x; sp[64] = gp.y; sp[2 * 64] = gp.z;
        sp[3 * 64] = gq.w; sp[4 * 64] = gq.x; sp[5 * 64] = gq.y; sp[6 * 64] = gq.z;
        float *cp = cen + (size_t)m * 3 * 64;
        cp[0] = (float)gp.x; cp[64] = (float)gp.y; cp[128] = (float)gp.z;
    }
    double res_d[kResMax];   // distances of the resident pairs of this lane's state
    MOPA_D void resident(int r, double d) { res_d[r] = d; }
    int ax_row;     // first row of the axis table, in rows of the centre table (3 nmg: it follows the centres)
    MOPA_D void axis(int slot, unsigned word) { reinterpret_cast<unsigned *>(cen)[(ax_row + slot) * 64] = word; }
};
using V5FkSink = V5FkSinkT<false>;

struct V5Lds {
    float *cen;                 // [nmg][3][64]   geom centres of this tile, FP32; baked scenes: then [n_ax][64] packed |axis| words of
                                //                the capsule / cylinder owners (k1_axis_word)
    unsigned *ent;              // [h.v5_ent_cap]    lane | owner slot << 6 | pair class << 12 | table index << 16
    unsigned *bat;              // [kBatCapV5]    entries of ONE pair class, compacted for the narrow phase
    unsigned *bat2;             // [kBatCapV5]    cylinder pairs that failed the capsule pre-test: dense batches for MPR
    unsigned long long *bad;    // [T]       one verdict word per tile of a drain (T: k1_tiles_per_drain, 1 but for a pair-drain scene)
    unsigned long long *md;     // [T][64]
    bool tp;                    // this tile's states share one env row and the scene has tile-posed geoms: their slab rows hold ONE pose, in lane 0's place
};
// (the 64 depth words `md` exist only in the instantiations that report depths: the verdict-only kernels give that LDS to `ent`)
// (a baked scene's axis table counts as entries: k_is_valid_v5 passes h.v5_ent_cap + k1_axis_words<TR>, the capacity the scene compiler sized)
MOPA_HD int v5_lds_per_wave(int nmg, int ent_cap, bool want_md) { return ((nmg * 3 * 64 * 4) + ent_cap * 4 + 2 * kBatCapV5 * 4 + (want_md ? 64 * 8 : 0) + 8 + 15) & ~15; }

// posed record (pos, mat, size) of geom g for the state of lane `sl` of the tile: moving geoms from the pose slab,
// static ones from the scene blob
// Both posed records of a pair.  Every load is issued before the first result is used: the static records (and the
// sizes of the moving ones) come from LDS unconditionally, position + quaternion of a moving geom from the tile's slab
// into temporaries, and only then the rotation matrices are formed -- written as two loads of one routine each, the
// compiler had chained them (slab quaternion -> wait -> matrix -> positions through a merged flat pointer -> next record).
MOPA_D void v5_load_rec2(double (&R1)[15], double (&R2)[15], const SceneHdr &h, const double *D, const double *slab_tile,
                         int gA, int movA, int slotA, int gB, int movB, int slotB, int slA, int slB) {
    const double *sA = D + h.o_g_rec + gA * kGeomStride, *sB = D + h.o_g_rec + gB * kGeomStride;
    double a[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, b[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (movA) {
        const double *sp = slab_tile + (size_t)slotA * kSlabStride + slA;
#pragma unroll
        for (int k = 0; k < 7; k++) a[k] = sp[64 * k];
    }
    if (movB) {
        const double *sp = slab_tile + (size_t)slotB * kSlabStride + slB;
#pragma unroll
        for (int k = 0; k < 7; k++) b[k] = sp[64 * k];
    }
#pragma unroll
    for (int i = 0; i < 15; i++) { R1[i] = sA[i]; R2[i] = sB[i]; }
    if (movA) {
        R1[0] = a[0]; R1[1] = a[1]; R1[2] = a[2];
        quat2mat(R1 + GO_MAT, Q4{a[3], a[4], a[5], a[6]});
    }
    if (movB) {
        R2[0] = b[0]; R2[1] = b[1]; R2[2] = b[2];
        quat2mat(R2 + GO_MAT, Q4{b[3], b[4], b[5], b[6]});
    }
}

// narrow phase on `n` (<= 64) entries of pair class `code` (wave-uniform: one routine runs, on full lanes)
// stage: 0 = the class routine; 1 = cylinder pairs, closed-form pre-test on the enclosing capsules only -- entries that are
// not proven disjoint are appended to the second ring (returns their number); 2 = cylinder pairs, portal refinement only
// T > 1 (pair drain): bit 31 of an entry is its half -- which slab region, verdict word, depth words and tile it belongs to
template <bool WANT_MD, int T = 1>
MOPA_D int v5_flush(const SceneHdr &h, const LdsView &v, const V5Lds &q, const int *s_tab, const double *slab_tile, int lane,
                    int head, int n, int code, int stage = 0, int head2 = 0, int count2 = 0, double *mpr_ring = nullptr,
                    int mpr_head = 0, int *mpr_count = nullptr, long long tile_base = 0) {
    bool to_mpr = false;
    unsigned e = 0;
    double R1s[15], R2s[15];
    int t1s = 0, t2s = 0;
    if (lane < n) {
        e = (stage == 2 ? q.bat2 : q.bat)[(head + lane) & (kBatCapV5 - 1)];
        const int sl = e & 63, m = (e >> 6) & 63, hf = T > 1 ? (int)(e >> kEntHalfBit) : 0;
        const int fl = s_tab[8 * (T > 1 ? (e >> 16) & 0x7fffu : e >> 16) + 7];
        if constexpr (T > 1) slab_tile += (size_t)hf * (size_t)(h.nmg + h.n_save) * kSlabStride;
        const int pg = fl & 0xff, cur_is_g2 = (fl >> 12) & 1, pmov = (fl >> 13) & 1, pslot = (fl >> 14) & 0xff;
        const double *D = v.dbl;
        const int *I = v.ints;
        const int cg = I[h.o_mg_geom + m];
        // geom 1 / geom 2 of the pair in the order the pair routines expect (type1 <= type2): the records are loaded
        // straight into place -- selecting 2 x 15 doubles afterwards cost more than the routine of a cheap class
        const int gA = cur_is_g2 ? pg : cg, gB = cur_is_g2 ? cg : pg;
        const int movA = cur_is_g2 ? pmov : 1, movB = cur_is_g2 ? 1 : pmov;
        const int slotA = cur_is_g2 ? pslot : m, slotB = cur_is_g2 ? m : pslot;
        double R1[15], R2[15];
        // (a tile-posed geom -- a body no active coordinate reaches, in a tile whose states share their env row -- has ONE pose per tile,
        //  kept in lane 0's place of its slab row: 64 lanes no longer store 64 copies of it)
        const int slA = (q.tp && movA && I[h.o_mg_pas + slotA] >= 0) ? 0 : sl, slB = (q.tp && movB && I[h.o_mg_pas + slotB] >= 0) ? 0 : sl;
        v5_load_rec2(R1, R2, h, D, slab_tile, gA, movA, slotA, gB, movB, slotB, slA, slB);
        const int t1 = I[h.o_g_type + gA], t2 = I[h.o_g_type + gB];
        double d;
        if (stage == 1) {
            const double pre = (t2 == G_BOX) ? d_capsule_box(R1, R2) : d_capsule_capsule(R1, R2);
            to_mpr = !(pre > 1e-9) && !convex_axes_separate(R1, t1, R2, t2);
            d = kFar;
            // verdict only: a pair that overlaps deeper than the threshold is decided without the refinement
            if (!WANT_MD && to_mpr && convex_overlap_deeper_than(R1, t1, R2, t2, convex_deep_delta(h.thr))) { to_mpr = false; d = h.thr; }
#pragma unroll
            for (int i = 0; i < 15; i++) { R1s[i] = R1[i]; R2s[i] = R2[i]; }
            t1s = t1; t2s = t2;
        } else if (stage == 2) {
            d = d_convex<false>(R1, t1, R2, t2);
        } else {
            d = geom_dist<false>(code, R1, t1, R2, t2, D);
        }
        if (d <= h.thr) atomicOr(q.bad + hf, 1ull << sl);
        if (WANT_MD) atomicMin(q.md + 64 * hf + sl, v5_depth_image(d));
    }
    int added = 0;
    if (stage == 1) {
        const unsigned long long mask = __ballot(to_mpr);
        const int nadd = __popcll(mask);
        if (mpr_ring && *mpr_count + nadd <= kMprCapV5) {
            // deferred: a tile yields ~20 such pairs, the refinement costs the same for 20 lanes as for 64 -- they wait in
            // the wave's ring (complete records, so they outlive the tile's slab) until a full batch has gathered
            if (to_mpr) {
                double *row = mpr_ring + (size_t)((mpr_head + *mpr_count + __popcll(mask & ((1ull << lane) - 1ull))) & (kMprCapV5 - 1)) * kMprRow;
#pragma unroll
                for (int i = 0; i < 15; i++) { row[i] = R1s[i]; row[15 + i] = R2s[i]; }
                row[30] = __longlong_as_double(tile_base + (long long)(T > 1 ? ((e >> kEntHalfBit) << 6) | (e & 63) : e & 63));
                row[31] = __longlong_as_double((long long)(t1s | (t2s << 8)));
            }
            *mpr_count += nadd;
        } else {
            if (to_mpr) q.bat2[(head2 + count2 + __popcll(mask & ((1ull << lane) - 1ull))) & (kBatCapV5 - 1)] = e;
            added = nadd;
        }
    }
    wave_sync();
    return added;
}

// Portal refinement for `n` (<= 64) rows of the wave's deferred ring.  Rows carry complete posed records and the index of
// the state they belong to; those states' tiles are finished (their verdicts are in global memory), so the result is folded
// straight into the outputs -- only this wave ever touches them.
template <bool WANT_MD>
MOPA_D void v5_mpr_rows(const SceneHdr &h, const double *ring, int head, int n, int lane, unsigned char *valid, double *min_dist) {
    if (lane < n) {
        const double *row = ring + (size_t)((head + lane) & (kMprCapV5 - 1)) * kMprRow;
        double R1[15], R2[15];
#pragma unroll
        for (int i = 0; i < 15; i++) { R1[i] = row[i]; R2[i] = row[15 + i]; }
        const long long s = __double_as_longlong(row[30]);
        const int tt = (int)__double_as_longlong(row[31]);
        const double d = d_convex<false>(R1, tt & 0xff, R2, (tt >> 8) & 0xff);
        if (d <= h.thr) valid[s] = 0;
        // depth = min(0, dist): several rows of a batch may belong to one state -> atomic; for negative doubles the more
        // negative value has the larger bit pattern, and the stored depth is <= 0, so an unsigned max is the minimum
        if (WANT_MD && d < 0.0) atomicMax(reinterpret_cast<unsigned long long *>(min_dist + s), (unsigned long long)__double_as_longlong(d));
    }
    wave_sync();
}

// All buffered survivor entries of the tile, class by class (cheapest first): entries of class c are compacted into
// the batch ring and evaluated 64 at a time.  Without WANT_MD, entries of states that are already invalid are
// dropped at compaction time (the per-state early-out).
template <bool WANT_MD, int T = 1>
MOPA_D void v5_drain(const SceneHdr &h, const LdsView &v, const V5Lds &q, const int *s_tab, const double *slab_tile, int lane,
                     int n_ent, unsigned present, double *mpr_ring, int mpr_head, int *mpr_count, long long tile_base) {
    wave_sync();
    for (int code = 0; code < PC_COUNT; code++) {
        if (!((present >> code) & 1u)) continue;
        int head = 0, count = 0, head2 = 0, count2 = 0;
        for (int base = 0; base < n_ent; base += 64) {
            const int i = base + lane;
            bool take = false;
            unsigned e = 0;
            if (i < n_ent) {
                e = q.ent[i];
                take = (int)((e >> 12) & 0xf) == code;      // the class travels in the entry: no dependent table read
                if (!WANT_MD) take = take && !((q.bad[T > 1 ? e >> kEntHalfBit : 0u] >> (e & 63)) & 1ull);
            }
            const unsigned long long mask = __ballot(take);
            if (!mask) continue;
            if (take) q.bat[(head + count + __popcll(mask & ((1ull << lane) - 1ull))) & (kBatCapV5 - 1)] = e;
            count += __popcll(mask);
            if (count >= 64) {
                wave_sync();
                if (code == PC_CONVEX) {
                    count2 += v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head, 64, code, 1, head2, count2, mpr_ring, mpr_head, mpr_count, tile_base);
                    if (count2 >= 64) {
                        v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head2, 64, code, 2);
                        head2 = (head2 + 64) & (kBatCapV5 - 1);
                        count2 -= 64;
                    }
                } else {
                    v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head, 64, code);
                }
                head = (head + 64) & (kBatCapV5 - 1);
                count -= 64;
            }
        }
        if (count > 0) {
            wave_sync();
            if (code == PC_CONVEX) count2 += v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head, count, code, 1, head2, count2, mpr_ring, mpr_head, mpr_count, tile_base);
            else v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head, count, code);
        }
        if (code == PC_CONVEX) {
            while (count2 > 0) {      // the cylinder pairs the capsule test could not separate: dense MPR batches
                const int nb = count2 < 64 ? count2 : 64;
                v5_flush<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, head2, nb, code, 2);
                head2 = (head2 + nb) & (kBatCapV5 - 1);
                count2 -= nb;
            }
        }
    }
}

// MOPA_V5_TIMELINE: the diagnostic build of tools/k1_wave_timeline.py (never the production library).  Every wave stamps the constant
// 100 MHz clock (s_memrealtime) where its life changes phase, into its own row of kTlRow words behind the launch's pose slabs (lane 0,
// plain vector stores; launch_is_valid sizes and zeroes the rows, mopa_k1_timeline_read copies them out).  Row: [0] kernel entry,
// [1] staged, [2] pulls (the one that found no tile included), [3] the last pull that got a tile, [4] the pull that found none = in
// front of the final portal flush, [5] behind that flush, [6] exit, [7] rows in that flush, [8] tiles, [9] HW_ID, [10 ..] every pull.
constexpr int kTlRow = 64, kTlPulls = kTlRow - 10;
#ifdef MOPA_V5_TIMELINE
#define V5_TL_DECL const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
#define V5_TL_STAGED const unsigned long long tl_t1 = __builtin_amdgcn_s_memrealtime();
#define V5_TL_ROW(tail_, w_)                                                                                  \
    unsigned long long *const tl_row = reinterpret_cast<unsigned long long *>(tail_) + (w_) * (size_t)kTlRow; \
    unsigned tl_pulls = 0u, tl_tiles = 0u;                                                                    \
    if (lane == 0) { tl_row[0] = tl_t0; tl_row[1] = tl_t1; tl_row[9] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (3 << 11)) << 32); }   /* HW_ID | XCC_ID << 32 */
#define V5_TL_PULL(fin_)                                                                  \
    {                                                                                     \
        const unsigned long long tl_t = __builtin_amdgcn_s_memrealtime();                 \
        if (lane == 0) {                                                                  \
            if (tl_pulls < (unsigned)kTlPulls) tl_row[10 + tl_pulls] = tl_t;              \
            tl_row[(fin_) ? 4 : 3] = tl_t;                                                \
        }                                                                                 \
        tl_pulls++;                                                                       \
    }
#define V5_TL_TILE tl_tiles++;
#define V5_TL_MPR0(fin_, n_) if ((fin_) && lane == 0) tl_row[7] = (unsigned long long)(n_);
#define V5_TL_MPR1(fin_) if ((fin_) && lane == 0) tl_row[5] = __builtin_amdgcn_s_memrealtime();
#define V5_TL_EXIT if (lane == 0) { tl_row[2] = tl_pulls; tl_row[8] = tl_tiles; tl_row[6] = __builtin_amdgcn_s_memrealtime(); }
#else
#define V5_TL_DECL
#define V5_TL_STAGED
#define V5_TL_ROW(tail_, w_)
#define V5_TL_PULL(fin_)
#define V5_TL_TILE
#define V5_TL_MPR0(fin_, n_)
#define V5_TL_MPR1(fin_)
#define V5_TL_EXIT
#endif

// CEN_LDS: the FP32 centre table of the tile lives in LDS (3 x 256 B per moving geom and wave).  Scenes with many moving
// geoms (Assembly 34, Lift 19) then get one workgroup per CU; with CEN_LDS = false the table of each wave lives in global
// memory instead (same FP32 values => the same survivors; 26 KB per wave for Assembly, a fifth of its pose slab, and the
// cull issues its loads four partners ahead) and two workgroups fit again.
// GATE: the scene has mesh pairs; they take part in the FP32 broad phase only, and the states in which one survives are
// appended to the work list of the second (mesh) pass.
// TR: scene traits (K1Generic, or a baked scene of mopa_valid_v5_baked.inc: CEN_LDS, no GATE).  A baked instantiation asks for
// two workgroups per CU: left to itself the allocator spends the straight-line pass A's freedom on 256 VGPRs + AGPRs (one
// wave per SIMD); held to 256 it needs 245 and spills no VGPR.  (The generic ones keep the default: measured slower with it.)
template <bool WANT_MD, bool CEN_LDS, bool GATE, class TR = K1Generic>
__global__ __launch_bounds__(kBlock, TR::kBaked ? 2 : 1) void k_is_valid_v5(SceneHdr h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                                         const int32_t *__restrict__ g_tab, const double *__restrict__ q_active,
                                                         const double *__restrict__ qpos_env, long long N, long long samples_per_env,
                                                         unsigned char *__restrict__ valid, double *__restrict__ min_dist,
                                                         double *__restrict__ slab_all, const int *__restrict__ env_idx /* nullable */, double *__restrict__ mpr_all,
                                                         long long *__restrict__ mesh_list /* nullable; scenes with mesh pairs: [0] = count, then the states */,
                                                         float *__restrict__ cen_all /* !CEN_LDS: per-wave FP32 centre tables [nmg][3][64] in global memory */,
                                                         const long long *__restrict__ n_dev /* nullable: the state count lives on the device (<= N) */, unsigned long long *__restrict__ tile_ctr,
                                                         double *__restrict__ mesh_rows /* nullable; GATE: [cap][kMprRow] complete records of the mesh pairs within reach (k_mesh_rows evaluates them) */,
                                                         long long mesh_rows_cap, unsigned long long *__restrict__ mesh_rows_cnt,
                                                         long long n_small /* with n_dev: counts below it are served by the wave-per-state launch in front of this one */,
                                                         long long pair_tiles /* pair drain: the leading tiles (an even number) that are pulled two at a time */) {
    constexpr int T = k1_tiles_per_drain<TR, WANT_MD>;        // tiles per drain ("Pair drain" above)
    static_assert(T == 1 || (T == 2 && TR::kBaked), "pair drain: two tiles, baked scenes only (the generic phase 0 borrows the entry buffer)");
    if constexpr (T > 1) static_assert(TR::padr[TR::nmg - 1] + TR::pnum[TR::nmg - 1] < (1 << 15), "pair drain: the entry's table index leaves bit 31 to the half");
    if (n_dev) {
        const long long nd = *n_dev;
        if (nd < N) N = nd;
        if (nd < n_small) N = 0;
    }
    V5_TL_DECL
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *s_dbl = reinterpret_cast<double *>(smem);
    int *s_int = reinterpret_cast<int *>(s_dbl + h.n_dbl);
    int *s_tab = s_int + ((h.n_int + 3) & ~3);                       // [n_gp][8] FP32 pair table
    constexpr int kTail = GATE ? 3 : 1;     // per geom after the entries: group counts [, first entry, count]
    // (MOPA_V5_FULL_STAGING: the knock-out of the baked scenes' lean staging, tools/k1_knock.sh fullstage)
#ifndef MOPA_V5_FULL_STAGING
    if constexpr (TR::kBaked) {
        stage_scene_k1_baked(h, g_dbl, g_int, g_tab, s_dbl, s_int, s_tab);   // ends with __syncthreads()
    } else
#endif
    {
        for (int i = threadIdx.x; i < 8 * h.n_gp + kTail * h.nmg; i += blockDim.x) s_tab[i] = g_tab[i];
        stage_scene(h, g_dbl, g_int, s_dbl, s_int);                      // ends with __syncthreads()
    }
    V5_TL_STAGED
    LdsView v;
    v.dbl = s_dbl; v.ints = s_int; v.grec = nullptr; v.qbuf = nullptr; v.sc = nullptr; v.wl = nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V5Lds q;
    {
        const int n_cen = CEN_LDS ? h.nmg : 0;
        int ent_words = h.v5_ent_cap;
        if constexpr (k1_axis_words<TR> > 0) ent_words += k1_axis_words<TR>;
        if constexpr (T > 1) ent_words += k1_pair_words<TR, WANT_MD>;    // (the second half's verdict / depth words, behind the first's)
        unsigned char *base = reinterpret_cast<unsigned char *>(s_tab + ((8 * h.n_gp + kTail * h.nmg + 3) & ~3)) + wave * v5_lds_per_wave(n_cen, ent_words, WANT_MD);
        q.cen = reinterpret_cast<float *>(base);
        // (a baked scene's axis table, [n_ax][64] words, sits between the centre table and the entries: a constant offset from the
        //  centres, so neither the walk nor pass A holds an address for it)
        q.ent = reinterpret_cast<unsigned *>(q.cen + n_cen * 3 * 64);
        if constexpr (k1_axis_words<TR> > 0) q.ent += k1_axis_words<TR>;
        q.bat = q.ent + h.v5_ent_cap;
        q.bat2 = q.bat + kBatCapV5;
        q.md = reinterpret_cast<unsigned long long *>(q.bat2 + kBatCapV5);
        q.bad = WANT_MD ? q.md + 64 * T : q.md;
        q.tp = false;
    }
    const double *__restrict__ GD = g_dbl;
    const int32_t *__restrict__ GI = g_int;
    const int nslab = h.nmg + h.n_save;
    // (pair drain: T slab regions per wave, one per half)
    double *slab = slab_all + ((size_t)blockIdx.x * kWavesPerBlock + wave) * (size_t)(T * nslab) * kSlabStride + lane;
    const double *slab_tile = slab - lane;
    double *mpr_ring = mpr_all + ((size_t)blockIdx.x * kWavesPerBlock + wave) * (size_t)kMprCapV5 * kMprRow;
    float *gcen = CEN_LDS ? nullptr : cen_all + ((size_t)blockIdx.x * kWavesPerBlock + wave) * (size_t)h.nmg * 3 * 64 + lane;
    int mpr_head = 0, mpr_count = 0;      // deferred cylinder pairs of this wave (persist across tiles)
    const long long n_tiles = (N + 63) >> 6;
    V5_TL_ROW(slab_all + (size_t)gridDim.x * kWavesPerBlock * (size_t)(T * nslab) * kSlabStride, (size_t)blockIdx.x * kWavesPerBlock + wave)
    // tile counter [0] + count of waves that have run out of tiles [1]: zero between launches -- the last wave to leave resets both
    // (tile_ctr_release), so no launch has to zero them first
    for (;;) {
        long long tile = 0;
        if (lane == 0) tile = (long long)atomicAdd(tile_ctr, (unsigned long long)T);
        tile = __shfl(tile, 0, 64);
        // pair drain: every pull adds 2.  Below pair_tiles a pull is the pair (tile, tile + 1); from there on it stands for ONE tile
        // (pulls pair_tiles, pair_tiles + 2, ... are the tiles pair_tiles, pair_tiles + 1, ...): the last tiles of a launch go out one
        // at a time, so the waves finish within one tile of each other as they did, not within two -- and a batch of fewer tiles than
        // the launch has waves still keeps every wave busy (k1_plan sets pair_tiles)
        bool single = false;
        if constexpr (T > 1) {
            if (tile >= pair_tiles) {
                tile = pair_tiles + ((tile - pair_tiles) >> 1);
                single = true;
            }
        }
        const bool fin = tile >= n_tiles;      // (pair drain: decided on the first tile of the pair)
        V5_TL_PULL(fin)
        if (!fin) {
        int n_ent;                 // survivor entries in the buffer and the pair classes among them: zeroed by the first half, and
        unsigned present;          // by every drain
        long long s;
        bool act, need_mesh;
        // pair drain: the halves, tile and tile + 1, one after the other through the same code (not unrolled); the entries of both wait
        // in the buffer for the drain behind the loop.  Nothing per lane lives across halves but what is in LDS and the slab.
        // (a do-while on a compile-time condition: with T == 1 there is no loop at all, and the kernel is the one it was)
        int hf = 0;
#pragma unroll 1
        do {
        if (T > 1 && hf > 0 && (single || tile + hf >= n_tiles)) break;       // no second tile (a single pull; an odd tile count or a device-side count that ends in the pair)
        V5_TL_TILE
        s = (tile + hf) * 64 + lane;
        act = s < N;
        if (!act) s = N - 1;
        const double *qa_row = q_active + s * h.na;
        const double *env_row = qpos_env + (env_idx ? (long long)env_idx[s] : s / samples_per_env) * h.nq;
        if (lane == 0) q.bad[hf] = 0ull;
        if (WANT_MD) q.md[64 * hf + lane] = f64_sortable(0.0);

        // ================= phase 1: forward kinematics, poses -> slab, FP32 centres -> LDS =================
        // (MOPA_V5_FK_REPS / _CULL_REPS / _KO_PASSB / _KO_DRAIN: knock-in / knock-out builds of tools/k1_knock.sh -- a phase run N
        //  times, or left out, and the kernel timed: per-phase cycle counters mislead when two waves share a SIMD)
        double res_d[kResMax] = {};      // baked scenes: the resident pairs' distances for this lane's state
#ifdef MOPA_V5_FK_REPS
        for (int fk_rep = 0; fk_rep < MOPA_V5_FK_REPS; fk_rep++)
#endif
        if constexpr (TR::kBaked) {       // (the baked scenes have no tile-posed bodies: q.tp stays false)
            // (the slab pointer passes through an empty asm once per tile: otherwise the 98 loop-invariant store addresses of the
            //  straight-line walk are hoisted out of the tile loop and held in VGPR pairs for the whole kernel)
            double *fk_slab = T > 1 ? slab + (size_t)hf * (size_t)nslab * kSlabStride : slab;
            asm volatile("" : "+v"(fk_slab));
            k1_gdouble *const fk_slab_g = (k1_gdouble *)fk_slab;      // (the asm erased what the kernel argument said: global memory)
            V5FkSink sink{fk_slab_g, q.cen + lane, {}, 3 * TR::nmg};
            // the sparse walk; a guard flag anywhere in the wave (rare: an exact zero in a stored pose, an input beyond 2^20 or not
            // finite): the dense walk for the tile, over everything the sparse one stored
            if constexpr (k1_sparse_on<TR>) {
                const bool fk_trip = k1_fk_baked<TR, true>(qa_row, env_row, sink, std::make_integer_sequence<int, TR::nmb>{});
                if (__builtin_expect(__ballot(fk_trip) != 0ull, 0)) {
                    // (the cold walk reads its inputs again through pointers the compiler cannot trace, so nothing of the sparse walk --
                    //  inputs, sines, the first bodies -- has to stay in registers for it)
                    const double *qa_cold = qa_row, *env_cold = env_row;
                    asm volatile("" : "+v"(qa_cold), "+v"(env_cold) : : "memory");
                    V5FkSinkT<true> cold{fk_slab_g, q.cen + lane, {}, 3 * TR::nmg};
                    k1_fk_baked<TR>((k1_gcdouble *)qa_cold, (k1_gcdouble *)env_cold, cold, std::make_integer_sequence<int, TR::nmb>{});
#pragma unroll
                    for (int r = 0; r < kResMax; r++) sink.res_d[r] = cold.res_d[r];
                }
            } else {
                k1_fk_baked<TR>(qa_row, env_row, sink, std::make_integer_sequence<int, TR::nmb>{});
            }
#pragma unroll
            for (int r = 0; r < kResMax; r++) res_d[r] = sink.res_d[r];
#ifdef MOPA_V5_FK_REPS
            asm volatile("" ::: "memory");   // each repetition loads, computes and stores again
#endif
        } else {
            // ---- phase 0 (tiles whose states share ONE env row): the bodies no active coordinate reaches, one body per lane, level by level
            // (same arithmetic per body as the walk below); poses -> `ps` (over the entry buffer, idle until phase 2): [body | geom][7]
            double *ps = reinterpret_cast<double *>(q.ent);
            bool tile_poses = false;
            if (!GATE && h.n_pas_b > 0) {       // (not in the mesh-gate instantiation: its registers are at the two-waves-per-SIMD limit)
                const unsigned long long er = (unsigned long long)env_row;
                const unsigned long long e0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(er >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)er);
                tile_poses = __all(er == e0);
            }
            q.tp = !GATE && tile_poses;
            if (!GATE && tile_poses) {
                for (int lv = 0; lv < h.n_pas_lv; lv++) {
                    const int i = s_int[h.o_pas_lv + lv] + lane;
                    if (i < s_int[h.o_pas_lv + lv + 1]) {
                        const int b = s_int[h.o_pas_b + i];
                        const int *ri = s_int + h.o_mbr + 8 * b;
                        V2BodyI bi;        // (field by field: the LDS copy of the int blob is only 8-byte aligned)
                        bi.jn = ri[0]; bi.jntadr = ri[1]; bi.load = ri[2]; bi.sf = ri[3]; bi.save = ri[4]; bi.mgadr = ri[5]; bi.mgnum = ri[6]; bi.jt_qsrc = ri[7];
                        const double *bd = s_dbl + h.o_mbd + 16 * b;
                        const int jt0 = bi.jt_qsrc & 0x7f, qsrc0 = bi.jt_qsrc >> 8;
                        V3 pos;
                        Q4 quat;
                        if (bi.jn == 1 && jt0 == J_FREE) {
                            const double *qp = env_row + s_int[h.o_pq_adr + (qsrc0 - h.na)];
                            fk_free_step(qp, pos, quat);
                        } else {
                            V3 ppos;
                            Q4 pquat;
                            double mat[9];
                            const int par = s_int[h.o_mb_parent + b];
                            if (par < 0) {
                                sf_frame_ld(h, s_dbl, bi.sf, ppos, pquat, mat);
                            } else {
                                const double *pp = ps + 7 * (s_int[h.o_mb_pas + par] & 0xffff);
                                pose7_ld<1>(pp, ppos, pquat);
                                quat2mat(mat, pquat);
                            }
                            pos = add3(ppos, mat_vec(mat, ld3(bd)));
                            quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
                            for (int jj = 0; jj < bi.jn; jj++) {
                                V3 ax, jp;
                                double ref;
                                int jt, src;
                                bool jp0;
                                if (jj == 0) {
                                    ax = ld3(bd + 7); jp = ld3(bd + 10); ref = bd[13]; jt = jt0; src = qsrc0; jp0 = (bi.jt_qsrc & 0x80) != 0;
                                } else {
                                    const int j = bi.jntadr + jj;
                                    ax = ld3(s_dbl + h.o_mj_axis + 3 * j); jp = ld3(s_dbl + h.o_mj_pos + 3 * j); ref = s_dbl[h.o_mj_ref + j];
                                    jt = s_int[h.o_mj_type + j]; src = s_int[h.o_mj_qsrc + j]; jp0 = is_zero3(jp);
                                }
                                const double qv = env_row[s_int[h.o_pq_adr + (src - h.na)]];        // (a passive coordinate by construction)
                                apply_joint(jt, ax, jp, jp0, qv - ref, pos, quat);
                            }
                            quat = quat_normalize(quat);
                        }
                        double *pp = ps + 7 * i;
                        pose7_st<1>(pp, pos, quat);
                    }
                    wave_sync();
                }
                if (lane < h.n_pas_g) {
                    const int m = s_int[h.o_pas_g + lane];
                    const double *pp = ps + 7 * (s_int[h.o_mb_pas + s_int[h.o_g_mb + s_int[h.o_mg_geom + m]]] & 0xffff);
                    const Q4 bq{pp[3], pp[4], pp[5], pp[6]};
                    double mat[9];
                    quat2mat(mat, bq);
                    const double *gd = s_dbl + h.o_mgd + 8 * m;
                    const V3 gp = add3(V3{pp[0], pp[1], pp[2]}, mat_vec(mat, ld3(gd)));
                    const Q4 gq = quat_mul(bq, Q4{gd[3], gd[4], gd[5], gd[6]});
                    double *gpp = ps + 7 * (h.n_pas_b + lane);
                    pose7_st<1>(gpp, gp, gq);
                }
                wave_sync();
            }
            V3 pos{0.0, 0.0, 0.0};
            Q4 quat{1.0, 0.0, 0.0, 0.0};
            double mat[9];
            double qact[8];
#pragma unroll
            for (int a = 0; a < 8; a++) qact[a] = (a < h.na) ? qa_row[a] : 0.0;
            // half-angle sine / cosine of every active joint value up front: eight independent evaluations that overlap,
            // instead of one at a time inside the serial walk down the chain (same function, same argument => same bits)
            double sn8[8], cs8[8];
#pragma unroll
            for (int a = 0; a < 8; a++) mopa_sincos(0.5 * (qact[a] - s_dbl[h.o_act_ref + a]), sn8[a], cs8[a]);
            for (int b = 0; b < h.nmb; b++) {
                const V2BodyI bi = *reinterpret_cast<const V2BodyI *>(GI + h.o_mbr + 8 * b);
                const double *bd = s_dbl + h.o_mbd + 16 * b;   // pos[3] quat[4] axis[3] jpos[3] ref
                const int jt0 = bi.jt_qsrc & 0x7f, qsrc0 = bi.jt_qsrc >> 8;
                const bool jp00 = (bi.jt_qsrc & 0x80) != 0;
                if (!GATE && tile_poses) {
                    const int pw = GI[h.o_mb_pas + b];
                    if (pw >= 0) {          // posed by the tile: the pose, its save slot, its geoms -- copied, not computed
                        const double *pp = ps + 7 * (pw & 0xffff);
                        pose7_ld<1>(pp, pos, quat);
                        if (!(pw & (1 << 16))) {
                            quat2mat(mat, quat);
                            if (bi.save >= 0) {
                                double *sp = slab + (size_t)(h.nmg + bi.save) * kSlabStride;
                                pose7_st<64>(sp, pos, quat);
                            }
                        }
                        for (int m = bi.mgadr; m < bi.mgadr + bi.mgnum; m++) {
                            const double *gp = ps + 7 * (h.n_pas_b + GI[h.o_mg_pas + m]);
                            // one pose for the tile (v5_flush reads lane 0's place for these geoms)
                            if (lane == 0) pose7_st<64>(slab + (size_t)m * kSlabStride, ld3(gp), Q4{gp[3], gp[4], gp[5], gp[6]});
                            float *cp = CEN_LDS ? q.cen + (size_t)m * 3 * 64 + lane : gcen + (size_t)m * 3 * 64;
                            cp[0] = (float)gp[0]; cp[64] = (float)gp[1]; cp[128] = (float)gp[2];
                        }
                        continue;
                    }
                }
                if (bi.jn == 1 && jt0 == J_FREE) {
                    const double *qp = env_row + GI[h.o_pq_adr + (qsrc0 - h.na)];
                    fk_free_step(qp, pos, quat);
                } else {
                    V3 ppos;
                    Q4 pquat;
                    if (bi.load == -2) {
                        sf_frame_ld(h, s_dbl, bi.sf, ppos, pquat, mat);
                    } else if (bi.load >= 0) {
                        const double *sp = slab + (size_t)(h.nmg + bi.load) * kSlabStride;
                        pose7_ld<64>(sp, ppos, pquat);
                        quat2mat(mat, pquat);
                    } else {
                        ppos = pos;
                        pquat = quat;
                    }
                    if (jt0 == J_GLUE) {        // the carried body of a glued scene: local pose out of the env row's free-joint slots
                        const double *qp = env_row + GI[h.o_pq_adr + (qsrc0 - h.na)];
                        fk_glue_step(ppos, pquat, mat, qp, pos, quat);
                    } else {
                        pos = add3(ppos, mat_vec(mat, ld3(bd)));
                        quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
                    }
                    for (int jj = 0; jj < bi.jn; jj++) {
                        V3 ax, jp;
                        double ref;
                        int jt, src;
                        bool jp0;
                        if (jj == 0) {
                            ax = ld3(bd + 7); jp = ld3(bd + 10); ref = bd[13]; jt = jt0; src = qsrc0; jp0 = jp00;
                        } else {
                            const int j = bi.jntadr + jj;
                            ax = ld3(GD + h.o_mj_axis + 3 * j); jp = ld3(GD + h.o_mj_pos + 3 * j); ref = GD[h.o_mj_ref + j];
                            jt = GI[h.o_mj_type + j]; src = GI[h.o_mj_qsrc + j]; jp0 = is_zero3(jp);
                        }
                        if (src < h.na && h.na <= 8) {
                            double qv = qact[0], sn = sn8[0], cs = cs8[0];
#pragma unroll
                            for (int a = 1; a < 8; a++) {
                                qv = (src == a) ? qact[a] : qv;
                                sn = (src == a) ? sn8[a] : sn;
                                cs = (src == a) ? cs8[a] : cs;
                            }
                            apply_joint_sc(jt, ax, jp, jp0, qv - ref, sn, cs, pos, quat);
                        } else {
                            const double qv = (src < h.na) ? qa_row[src] : env_row[GI[h.o_pq_adr + (src - h.na)]];
                            apply_joint(jt, ax, jp, jp0, qv - ref, pos, quat);
                        }
                    }
                    quat = quat_normalize(quat);
                }
                quat2mat(mat, quat);
                if (bi.save >= 0) {
                    double *sp = slab + (size_t)(h.nmg + bi.save) * kSlabStride;
                    pose7_st<64>(sp, pos, quat);
                }
                for (int m = bi.mgadr; m < bi.mgadr + bi.mgnum; m++) {
                    const double *gd = s_dbl + h.o_mgd + 8 * m;   // lpos[3] lquat[4] rbound
                    const V3 gp = add3(pos, mat_vec(mat, ld3(gd)));
                    const Q4 gq = quat_mul(quat, Q4{gd[3], gd[4], gd[5], gd[6]});
                    double *sp = slab + (size_t)m * kSlabStride;
                    pose7_st<64>(sp, gp, gq);
                    float *cp = CEN_LDS ? q.cen + (size_t)m * 3 * 64 + lane : gcen + (size_t)m * 3 * 64;
                    cp[0] = (float)gp.x; cp[64] = (float)gp.y; cp[128] = (float)gp.z;
                }
            }
        }
        wave_sync();

        // ================= phase 2: FP32 broad phase out of LDS, queue, FP64 narrow phase =================
        bool dead = !act;
        need_mesh = false;
        if constexpr (TR::kBaked) {
            if constexpr (k1_n_res<TR> > 0) {
                // the resident pairs are decided: the verdict as v5_flush folds it (d <= thr), the depth through the same
                // order-preserving image; a verdict-only lane that is invalid builds no entries (as under deep_mask below)
                bool rbad = false;
                unsigned long long rmd = f64_sortable(0.0);
#pragma unroll
                for (int r = 0; r < k1_n_res<TR>; r++) {
                    rbad = rbad || (res_d[r] <= h.thr);
                    const unsigned long long im = v5_depth_image(res_d[r]);
                    rmd = im < rmd ? im : rmd;
                }
                rbad = rbad && act;
                const unsigned long long rmask = __ballot(rbad);
                if (lane == 0 && rmask) q.bad[hf] |= rmask;
                if (WANT_MD) q.md[64 * hf + lane] = rmd;
                else dead = dead || rbad;
            }
        }
        if (T == 1 || hf == 0) {
            n_ent = 0;
            present = 0u;
        }
        for (int m = 0; m < h.nmg; m++) {
            int p0, pn;
            if (GATE) {          // the table of a scene with mesh pairs lists them too: its own (first entry, count) per geom
                p0 = g_tab[8 * h.n_gp + h.nmg + 2 * m]; pn = g_tab[8 * h.n_gp + h.nmg + 2 * m + 1];
            } else {
                const V2GeomI gi = *reinterpret_cast<const V2GeomI *>(GI + h.o_mgr + 4 * m);
                p0 = gi.padr; pn = gi.pnum;
            }
            if (pn == 0) continue;
            float cx, cy, cz;
            if (CEN_LDS) {
                const float *cp = q.cen + (size_t)m * 3 * 64 + lane;
                cx = cp[0]; cy = cp[64]; cz = cp[128];
            } else {
                const float *cp = gcen + (size_t)m * 3 * 64;
                cx = cp[0]; cy = cp[64]; cz = cp[128];
            }
            // ---- pass A: survivor bit per candidate pair.  The pair table of this geom is fetched ONCE, one entry per
            //      lane, and broadcast pair by pair with v_readlane (no memory latency inside the loops); the entries
            //      are grouped [moving | static | plane] so each loop is branch-free FP32 arithmetic against constants
            //      that already include this geom's inflated radius.  Every test is a compare into a scalar lane mask
            //      (ballot), the masks are combined on the scalar unit and come back as the per-lane predicate
            //      (inverse ballot): two vector instructions per pair for the bookkeeping ----
            unsigned surv_lo = 0u, surv_hi = 0u;
            unsigned long long deep_mask = 0ull;   // lanes whose state this geom's moving partners prove invalid
            int t7 = 0;        // flags word of table entry p0 + lane (pass B broadcasts it again)
            unsigned long long any_kept = 0ull;   // baked scenes: the pairs some lane kept (pass B visits only these)
            if constexpr (TR::kBaked) {
                static_assert(CEN_LDS && !GATE, "baked scenes: centre table in LDS, no mesh gate");
                if (lane < pn) t7 = s_tab[8 * (p0 + lane) + 7];
#ifdef MOPA_V5_CULL_REPS
                for (int cull_rep = 1; cull_rep < MOPA_V5_CULL_REPS; cull_rep++) {
                    v5_pass_a_dispatch<TR, WANT_MD>(m, cx, cy, cz, q.cen + lane, surv_lo, surv_hi, deep_mask, any_kept, std::make_integer_sequence<int, TR::nmg>{});
                    asm volatile("" : "+v"(surv_lo), "+v"(surv_hi));
                }
#endif
                v5_pass_a_dispatch<TR, WANT_MD>(m, cx, cy, cz, q.cen + lane, surv_lo, surv_hi, deep_mask, any_kept, std::make_integer_sequence<int, TR::nmg>{});
            } else {
                const int cnt = g_tab[8 * h.n_gp + m];
                const int n_mov = cnt & 0xff, n_stat = (cnt >> 8) & 0xff, n_pl = (cnt >> 16) & 0xff;
                int t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0, t6 = 0;
                if (lane < pn) {
                    const int4 *te = reinterpret_cast<const int4 *>(s_tab + 8 * (p0 + lane));
                    const int4 a = te[0], b = te[1];
                    t0 = a.x; t1 = a.y; t2 = a.z; t3 = a.w; t4 = b.x; t5 = b.y; t6 = b.z; t7 = b.w;
                }
#define V5_KEEP(cull_mask_)                                                                       \
                {                                                                                 \
                    const unsigned sv = __builtin_amdgcn_inverse_ballot_w64(~(cull_mask_)) ? 1u : 0u;   \
                    if (!WIDE || k < 32) surv_lo |= sv << (k & 31); else surv_hi |= sv << (k & 31);     \
                }
                // WIDE: the geom has more than 32 candidate pairs (the survivor bits then need the second word)
                auto pass_a = [&](auto wide_c) {
                constexpr bool WIDE = decltype(wide_c)::value;
                int k = 0;
                {
                    // moving partners: centre from the tile's table (LDS, or global memory for scenes whose table does not
                    // fit).  Four partners' loads are issued before the first test waits for one (the last group of a geom
                    // repeats its last partner in the unused places)
                    for (; k < n_mov; k += 4) {
                        float px[4], py[4], pz[4], rs2[4], rin2[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const int ku = (k + u < n_mov) ? k + u : n_mov - 1;
                            const int fl = __builtin_amdgcn_readlane(t7, ku);
                            const float *pc = (CEN_LDS ? q.cen + lane : gcen) + (size_t)((fl >> 14) & 0xff) * 3 * 64;
                            px[u] = pc[0]; py[u] = pc[64]; pz[u] = pc[128];
                            rs2[u] = __int_as_float(__builtin_amdgcn_readlane(t3, ku));
                            rin2[u] = __int_as_float(__builtin_amdgcn_readlane(t0, ku));
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const float dx = cx - px[u], dy = cy - py[u], dz = cz - pz[u];
                            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                            // inscribed balls overlap deeper than the threshold: the state is invalid (verdict-only kernels)
                            if (!WANT_MD) deep_mask |= __ballot(d2 < rin2[u]);
                            unsigned sv = __builtin_amdgcn_inverse_ballot_w64(~__ballot(d2 > rs2[u])) ? 1u : 0u;
                            if (k + u >= n_mov) sv = 0u;
                            if (!WIDE || k + u < 32) surv_lo |= sv << ((k + u) & 31); else surv_hi |= sv << ((k + u) & 31);
                        }
                    }
                    k = n_mov;
                }
                for (const int kend = n_mov + n_stat; k < kend; k++) {   // static partners: sphere, then world AABB
                    const float dx = cx - __int_as_float(__builtin_amdgcn_readlane(t0, k));
                    const float dy = cy - __int_as_float(__builtin_amdgcn_readlane(t1, k));
                    const float dz = cz - __int_as_float(__builtin_amdgcn_readlane(t2, k));
                    const float rs2 = __int_as_float(__builtin_amdgcn_readlane(t3, k));
                    const float hx = __int_as_float(__builtin_amdgcn_readlane(t4, k));
                    const float hy = __int_as_float(__builtin_amdgcn_readlane(t5, k));
                    const float hz = __int_as_float(__builtin_amdgcn_readlane(t6, k));
                    V5_KEEP(__ballot(fmaf(dz, dz, fmaf(dy, dy, dx * dx)) > rs2) | __ballot(fabsf(dx) > hx) |
                            __ballot(fabsf(dy) > hy) | __ballot(fabsf(dz) > hz))
                }
                for (const int kend = n_mov + n_stat + n_pl; k < kend; k++) {   // planes: (t4,t5,t6) is the normal
                    const float dx = cx - __int_as_float(__builtin_amdgcn_readlane(t0, k));
                    const float dy = cy - __int_as_float(__builtin_amdgcn_readlane(t1, k));
                    const float dz = cz - __int_as_float(__builtin_amdgcn_readlane(t2, k));
                    const float rg = __int_as_float(__builtin_amdgcn_readlane(t3, k));
                    const float hx = __int_as_float(__builtin_amdgcn_readlane(t4, k));
                    const float hy = __int_as_float(__builtin_amdgcn_readlane(t5, k));
                    const float hz = __int_as_float(__builtin_amdgcn_readlane(t6, k));
                    V5_KEEP(__ballot(fmaf(dz, hz, fmaf(dy, hy, dx * hx)) > rg))
                }
                };
#ifdef MOPA_V5_CULL_REPS
                for (int cull_rep = 1; cull_rep < MOPA_V5_CULL_REPS; cull_rep++) {
                    if (pn <= 32) pass_a(std::false_type{}); else pass_a(std::true_type{});
                    asm volatile("" : "+v"(surv_lo), "+v"(surv_hi));
                }
#endif
                if (pn <= 32) pass_a(std::false_type{}); else pass_a(std::true_type{});
#undef V5_KEEP
            }
            if (!WANT_MD && deep_mask) {       // proven invalid in the broad phase: verdict set, no entries from here on, and the
                if (lane == 0) atomicOr(q.bad + hf, deep_mask);      // ones already queued are dropped when their class is compacted
                dead = dead || ((deep_mask >> lane) & 1ull);
            }
            if (dead) { surv_lo = 0u; surv_hi = 0u; }
            // ---- pass B: survivors -> 4-byte entries in the tile's buffer ----
#ifdef MOPA_V5_KO_PASSB
            if (lane == 0 && (surv_lo | surv_hi) == 0xdeadbeefu) *q.bad = 1ull;
            continue;
#endif
            if (!__any((surv_lo | surv_hi) != 0u)) continue;
            auto pass_b_pair = [&](const int k) {
                const bool sv = (((k < 32) ? surv_lo : surv_hi) >> (k & 31)) & 1u;
                const unsigned long long mask = __ballot(sv);
                if (!mask) return;
                const unsigned pcode = ((unsigned)__builtin_amdgcn_readlane(t7, k) >> 8) & 0xfu;
                if (GATE && pcode >= (unsigned)PC_PLANE_MESH) {     // mesh pair within reach: evaluated after this kernel
                    // Its two posed records go to the launch's row list as they stand in the slab: k_mesh_rows runs the pair routine on them, a
                    // quad of lanes per row, with no forward kinematics and no cull of its own (the state-list pass needed ~115 us for ONE state:
                    // launch, scene staging, the whole chain walk, then the refinement).  A row that does not fit the list puts its state on the
                    // state list instead (the second pass of the MESH instantiation: every mesh pair of the state).
                    bool listed = sv;
                    if (mesh_rows) {
                        unsigned long long at = 0;
                        if (lane == (int)__builtin_ctzll(mask)) at = atomicAdd(mesh_rows_cnt, (unsigned long long)__popcll(mask));
                        at = __shfl(at, (int)__builtin_ctzll(mask), 64);
                        const long long slot = (long long)at + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                        if (sv && slot < mesh_rows_cap) {
                            const int fl = __builtin_amdgcn_readlane(t7, k);
                            const int pg = fl & 0xff, cur_is_g2 = (fl >> 12) & 1, pmov = (fl >> 13) & 1, pslot = (fl >> 14) & 0xff;
                            const int cg = s_int[h.o_mg_geom + m];
                            const int gA = cur_is_g2 ? pg : cg, gB = cur_is_g2 ? cg : pg;
                            double R1[15], R2[15];
                            v5_load_rec2(R1, R2, h, s_dbl, slab_tile, gA, cur_is_g2 ? pmov : 1, cur_is_g2 ? pslot : m, gB, cur_is_g2 ? 1 : pmov, cur_is_g2 ? m : pslot, lane, lane);
                            double *row = mesh_rows + (size_t)slot * kMprRow;
#pragma unroll
                            for (int i = 0; i < 15; i++) { row[i] = R1[i]; row[15 + i] = R2[i]; }
                            row[30] = __longlong_as_double(s);
                            row[31] = __longlong_as_double((long long)(s_int[h.o_g_type + gA] | (s_int[h.o_g_type + gB] << 8) | ((int)pcode << 16)));
                            listed = false;
                        }
                    }
                    need_mesh |= listed;
                    return;
                }
                if (sv) q.ent[n_ent + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] =
                            (unsigned)lane | ((unsigned)m << 6) | (pcode << 12) | ((unsigned)(p0 + k) << 16) | (T > 1 ? (unsigned)hf << kEntHalfBit : 0u);
                n_ent += __popcll(mask);
                present |= 1u << pcode;
#ifdef MOPA_V5_KO_DRAIN
                if (n_ent > h.v5_ent_cap - 64) n_ent = 0;
#endif
                if (n_ent > h.v5_ent_cap - 64) {           // buffer (almost) full: evaluate what is there (pair drain: of both halves, maybe)
                    v5_drain<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, n_ent, present, mpr_ring, mpr_head, &mpr_count, tile * 64);
                    n_ent = 0;
                    present = 0u;
                }
            };
            if constexpr (TR::kBaked) {
                for (unsigned long long bits = any_kept; bits; bits &= bits - 1ull) pass_b_pair((int)__builtin_ctzll(bits));
            } else {
                for (int k = 0; k < pn; k++) pass_b_pair(k);
            }
        }
        } while (T > 1 && ++hf < T);       // (the halves)
#ifndef MOPA_V5_KO_DRAIN
        if (n_ent > 0) v5_drain<WANT_MD, T>(h, v, q, s_tab, slab_tile, lane, n_ent, present, mpr_ring, mpr_head, &mpr_count, tile * 64);
#endif
        wave_sync();
        if constexpr (T == 1) {
            if (act) {
                valid[s] = ((*q.bad >> lane) & 1ull) ? 0 : 1;
                if (WANT_MD) min_dist[s] = f64_unsortable(q.md[lane]);
            }
        } else {
#pragma unroll
            for (int ho = 0; ho < T; ho++) {        // (a second half that was skipped: a single pull, or it lies beyond N)
                const long long so = (tile + ho) * 64 + lane;
                if (so < N && !(ho > 0 && single)) {
                    const int hf = ho;
                    valid[so] = ((q.bad[hf] >> lane) & 1ull) ? 0 : 1;
                    if (WANT_MD) min_dist[so] = f64_unsortable(q.md[64 * hf + lane]);
                }
            }
        }
        if (GATE && mesh_list) {     // states with a mesh pair within reach: appended to the second pass's work list
            const bool f = act && need_mesh;
            const unsigned long long fm = __ballot(f);
            if (fm) {
                unsigned long long at = 0;
                if (lane == 0) at = atomicAdd(reinterpret_cast<unsigned long long *>(mesh_list), (unsigned long long)__popcll(fm));
                at = __shfl(at, 0, 64);
                if (f) mesh_list[1 + at + __popcll(fm & ((1ull << lane) - 1ull))] = s;
            }
        }
        wave_sync();
        }
        // deferred cylinder pairs: full batches now, whatever is left when the wave runs out of tiles
        V5_TL_MPR0(fin, mpr_count)
        while (mpr_count >= 64 || (fin && mpr_count > 0)) {
            const int nb = mpr_count < 64 ? mpr_count : 64;
            __threadfence_block();
            v5_mpr_rows<WANT_MD>(h, mpr_ring, mpr_head, nb, lane, valid, min_dist);
            mpr_head = (mpr_head + nb) & (kMprCapV5 - 1);
            mpr_count -= nb;
        }
        V5_TL_MPR1(fin)
        if (fin) break;
    }
    tile_ctr_release(tile_ctr, lane);
    V5_TL_EXIT
}

// The mesh pairs the gate of k_is_valid_v5 found within reach, as complete records (rows: geom 1 record[15], geom 2 record[15], state
// index, types | pair class << 16): the pair routine on G lanes per row (MOPA_MESH_ROWS_G, 8 as shipped; they share the exhaustive
// vertex searches of the hull's support function: mesh_support_local<G>, 14 of the can's 106 vertices per lane), 64 / G = 8 rows per wave and round; the verdict / depth is folded straight into the first pass's outputs
// (same stream, after it).  The hull vertices are staged in LDS.  Same routine on the same records as the state-list pass => the same bits.
#ifndef MOPA_MESH_ROWS_G
#define MOPA_MESH_ROWS_G 8
#endif
template <bool WANT_MD, int G = MOPA_MESH_ROWS_G>
__global__ __launch_bounds__(kBlock) void k_mesh_rows(SceneHdr h, const double *__restrict__ g_dbl, const double *__restrict__ rows,
                                                       const unsigned long long *__restrict__ cnt, long long cap, int n_mesh_dbl,
                                                       unsigned char *__restrict__ valid, double *__restrict__ min_dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *s_mesh = reinterpret_cast<double *>(smem);
    long long n = (long long)*cnt;
    if (n > cap) n = cap;
    if (n == 0) return;
    for (int i = threadIdx.x; i < n_mesh_dbl; i += blockDim.x) s_mesh[i] = g_dbl[h.o_mesh + i];
    __syncthreads();
    const double *aux = s_mesh - h.o_mesh;
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), nw = (long long)gridDim.x * kWavesPerBlock;
    constexpr int kPer = 64 / G;          // rows per wave and round
    for (long long base = gw * kPer; base < n; base += nw * kPer) {
        const long long i = base + lane / G;
        if (i < n) {
            const double *row = rows + (size_t)i * kMprRow;
            double R1[15], R2[15];
#pragma unroll
            for (int k = 0; k < 15; k++) { R1[k] = row[k]; R2[k] = row[15 + k]; }
            const long long s = __double_as_longlong(row[30]);
            const int tt = (int)__double_as_longlong(row[31]);
            const double d = geom_dist<true, G>((tt >> 16) & 0xf, R1, tt & 0xff, R2, (tt >> 8) & 0xff, aux);
            if ((lane & (G - 1)) == 0) {
                if (d <= h.thr) valid[s] = 0;
                // (as v5_mpr_rows: the stored depth is <= 0, for negative doubles an unsigned max of the bit patterns is the minimum)
                if (WANT_MD && d < 0.0) atomicMax(reinterpret_cast<unsigned long long *>(min_dist + s), (unsigned long long)__double_as_longlong(d));
            }
        }
    }
}
