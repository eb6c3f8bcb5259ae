// mopa_k9.inc -- K9: OMPL's PathSimplifier restated, one wave per path, persistent waves.
// (included by mopa_hip.hip behind the planner, whose multi-state validity pass the smoothing calls)
//
// One kernel body, three instantiations (DESIGN.md "K9 path simplification"):
//   LEVEL 0, k_simplify_paths: reduceVertices and collapseCloseVertices.  Both only REMOVE waypoints, so the result is a subset of
//            the planner's rows (tests/simplify_ref.py).
//   LEVEL 1, k_shortcut_paths: shortcutPath in front of them (tests/shortcut_ref.py).  Two points are drawn by arc length, located
//            on the path, connected when K2's rule allows it -- and, a deviation, when the stubs between a new interior point and
//            its old neighbours pass too -- so the result has corners that are no planner rows.
//   LEVEL 2, k_smooth_paths: smoothBSpline between shortcutPath and the vertex passes of a round (tests/smooth_ref.py).  Up to
//            three steps, each of which puts a vertex into the middle of every segment and then pulls every old interior vertex
//            towards the middle of its two new neighbours when the two motions that creates pass K2's rule and the vertex moves
//            by more than a hundredth of the path's length.  Three deviations keep every segment of a result one that has itself
//            passed the motion check, so that there is nothing for checkAndRepair to do: a vertex moves only if the outer halves
//            of its two old segments pass too, a step in which nothing moves is undone, and a midpoint between two vertices that
//            stayed is kept only if both its halves pass.
// A level's result is required identical to its sequential form, new states included, hence every floating-point operation is the
// one named there: adds, one product / one division where stated, interp_dim's fma.  With the passes bits of the higher stages
// clear a level gives the bytes of the one below.
//
// The rows stay where they are: a 16-bit list maps vertex position to a row slot among the path's own max_path rows.  At LEVEL 0
// no row is ever created, a slot is the original row, the list stays ascending and the final compaction walks it once.  From
// LEVEL 1 on new points take free slots (a stack), erased ones return theirs, the cumulative distances live in LDS, and one
// in-place gather puts the rows into order at the end; no row is ever taken back once it is written.  The pairs
// collapseCloseVertices has found blocked live in the wave's LDS too.  Every decision is taken from wave-uniform values, the
// counters are scalars.  A motion check is motion_valid_ends with path row 0 as the env row; the state checks of the smoothing's
// midpoints do not depend on one another and run kMS = 4 states per validity pass (plan_states_valid_ms).  No atomics, no
// read-back.  checkAndRepair is not built.

struct K9Args {
    double *path;                       // [E, max_path, nq] in/out
    int32_t *path_len;                  // [E] in/out
    const int32_t *status;              // [E] nullable
    long long E;
    int max_path, passes, max_rounds;   // (max_rounds: LEVEL >= 1)
    unsigned long long seed, env_id_base;
    const unsigned long long *env_ids, *seeds;      // nullable, as in MopaPlanParams
    long long *info;                    // [E, k9_info_cols] nullable: motion checks, draws; LEVEL >= 1: rounds, accepted splices, capacity
                                        // skips, largest vertex count; LEVEL 2: smoothing steps, vertices moved, midpoints dropped, state checks
    int hdr_lds_off, list_lds_off, list_bytes;      // LDS: SceneHdr copy, the waves' lists, bytes of one wave's lists
};

MOPA_HD constexpr int k9_info_cols(int level) { return level == 0 ? 2 : level == 1 ? 6 : 10; }
// what one more row of max_path costs a wave: LEVEL 0 a blocked-pair word and a list entry; LEVEL 1 a cumulative distance, the
// word, the entry and a free-stack entry; LEVEL 2 a verdict byte and a moved bit on top
MOPA_HD constexpr int k9_row_bytes(int level) { return level == 0 ? 6 : level == 1 ? 16 : 18; }
// per wave behind the header copy:
//   LEVEL 0:  [2 * na doubles: the endpoints of the check][max_path words: blocked pairs][max_path halves: slot of vertex k]
//   LEVEL 1:  [4 * na doubles: the endpoints, the points A and B][nq doubles: a new row][max_path doubles: cumulative distances]
//             [max_path words: blocked pairs][max_path halves: slot of vertex k][max_path halves: free slots]
MOPA_HD int k9_list_bytes(int level, int na, int nq, int max_path) {
    return ((level == 0 ? 16 * na : 8 * (4 * na + nq)) + (level == 0 ? 6 : 16) * max_path + 15) & ~15;
}
// LEVEL 2, behind LEVEL 1's lists, every part padded to 16 bytes: [max_path bytes: verdict of segment k in bits 0-1 (0 not checked
// yet, 1 passed, 2 failed), bit 2 the midpoint in front of candidate k is valid, bit 3 midpoint k leaves][max_path bits: vertex k
// moved in this step]; the slabs of the four-state validity pass (ms_bytes_per_wave) follow
MOPA_HD int k9_verdict_bytes(int max_path) { return (max_path + 15) & ~15; }
MOPA_HD int k9_flag_bytes(int max_path) { return k9_verdict_bytes(max_path) + ((((max_path + 31) >> 5) * 4 + 15) & ~15); }

template <int LEVEL>
__device__ __forceinline__ void k9_paths_body(const SceneHdr &h, const double *__restrict__ g_dbl, const int32_t *__restrict__ g_int,
                                              const K9Args &a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsView v = make_view(h, smem);
    SceneHdr *lh = reinterpret_cast<SceneHdr *>(smem + a.hdr_lds_off);
    for (int i = threadIdx.x; i < (int)(sizeof(SceneHdr) / 4); i += blockDim.x)
        reinterpret_cast<int *>(lh)[i] = reinterpret_cast<const int *>(&h)[i];
    stage_scene(h, g_dbl, g_int, const_cast<double *>(v.dbl), const_cast<int *>(v.ints));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int na = h.na, nq = h.nq, max_path = a.max_path;
    unsigned char *lbase = smem + a.list_lds_off + wave * a.list_bytes;
    double *ends = reinterpret_cast<double *>(lbase);                                   // [2][na]
    double *ptA = nullptr, *ptB = nullptr, *rowbuf = nullptr, *D = nullptr;
    unsigned *blocked = reinterpret_cast<unsigned *>(ends + 2 * na);                    // [max_path]: slot i << 16 | slot j
    if constexpr (LEVEL >= 1) {
        ptA = ends + 2 * na, ptB = ptA + na;                                            // [na] each: the two points of a shortcut
        rowbuf = ptB + na;                                                              // [nq]: row 0, active entries overwritten per new row
        D = rowbuf + nq;                                                                // [max_path]: cumulative distance at vertex k
        blocked = reinterpret_cast<unsigned *>(D + max_path);
    }
    unsigned short *idx = reinterpret_cast<unsigned short *>(blocked + max_path);       // [max_path]: row slot of vertex k
    unsigned short *freel = LEVEL >= 1 ? idx + max_path : nullptr;                      // [max_path]: stack of the max_path - cnt free slots
    double *tst = v.qbuf + na + h.n_pq;                                                 // spare [na] doubles behind the joint-value buffer
    unsigned char *vd = LEVEL >= 2 ? lbase + k9_list_bytes(1, na, nq, max_path) : nullptr;                  // [max_path]: flags of position k
    unsigned *mvw = reinterpret_cast<unsigned *>(LEVEL >= 2 ? vd + k9_verdict_bytes(max_path) : nullptr);   // [max_path bits]: vertex k moved
    MsLds ms;
    ms.grec = reinterpret_cast<double *>(LEVEL >= 2 ? vd + k9_flag_bytes(max_path) : nullptr);
    ms.qbuf = ms.grec + kMS * h.nmg * kGeomStride;
    ms.qs = ms.qbuf + kMS * (na + h.n_pq + ms_sc_doubles(h.nmj, h.nmb));
    ms.wl = reinterpret_cast<unsigned *>(ms.qs + kMS * na);
    const int *adr = v.ints + h.o_act_adr;
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long e = (long long)blockIdx.x * kWavesPerBlock + wave; e < a.E; e += stride) {
        const int n_in = a.path_len[e];
        if ((a.status && a.status[e] != 0) || n_in < 3 || n_in > max_path) continue;         // skipped: nothing of it is touched
        double *pe = a.path + (size_t)e * max_path * nq;
        const unsigned long long key = rng_key(a.seeds ? a.seeds[e] : a.seed, a.env_ids ? a.env_ids[e] : a.env_id_base + (unsigned long long)e);
        for (int i = lane; i < n_in; i += 64) idx[i] = (unsigned short)i;
        if constexpr (LEVEL >= 1) {
            for (int i = lane; i < max_path - n_in; i += 64) freel[i] = (unsigned short)(n_in + i);
            for (int i = lane; i < nq; i += 64) rowbuf[i] = pe[i];
        }
        wave_sync();
        int cnt = n_in, max_cnt = n_in, rounds = 0;
        long long n_checks = 0, n_draws = 0, n_splices = 0, n_cap = 0;             // (the last two: LEVEL >= 1)
        long long n_steps = 0, n_moved = 0, n_dropped = 0, n_state = 0;           // (LEVEL 2)

        auto slot = [&](int k) -> int { return __builtin_amdgcn_readfirstlane((int)idx[k]); };
        auto uni = [&](bool b) -> bool { return __builtin_amdgcn_readfirstlane((int)b) != 0; };
        auto load_vertex = [&](double *dst, int k) {
            const double *r = pe + (size_t)slot(k) * nq;
            for (int i = lane; i < na; i += 64) dst[i] = r[adr[i]];
        };
        auto load_point = [&](double *dst, const double *src) {
            for (int i = lane; i < na; i += 64) dst[i] = src[i];
        };
        // K2's rule from ends[0..na) to ends[na..2 na)
        auto check_ends = [&]() -> bool {
            n_checks++;
            return motion_valid_ends(h, v, lh, lane, ends, tst, pe);
        };
        auto check = [&](int ia, int ib) -> bool {
            load_vertex(ends, ia);
            load_vertex(ends + na, ib);
            return check_ends();
        };
        // the vertices strictly between ia and ib leave: from LEVEL 1 on their slots go onto the free stack; the tail moves by
        // `delta` (< 0: up, 64 entries at a time ascending, a chunk's targets lie below the next chunk's sources; 1: down,
        // descending), and `ins` entries behind ia are left to the caller
        auto replace = [&](int ia, int ib, int ins) {
            const int gap = ib - ia - 1, delta = ins - gap;
            if constexpr (LEVEL >= 1) {
                const int top = max_path - cnt;
                for (int j = lane; j < gap; j += 64) freel[top + j] = idx[ia + 1 + j];
                wave_sync();
            }
            if (delta < 0) {
                for (int base = ib; base < cnt; base += 64) {
                    const int s = base + lane;
                    const unsigned short val = s < cnt ? idx[s] : (unsigned short)0;
                    wave_sync();
                    if (s < cnt) idx[s + delta] = val;
                    wave_sync();
                }
            }
            if constexpr (LEVEL >= 1) {
                if (delta > 0) {
                    for (int hi = cnt; hi > ib; hi -= 64) {
                        const int s = hi - 1 - lane;
                        const unsigned short val = s >= ib ? idx[s] : (unsigned short)0;
                        wave_sync();
                        if (s >= ib) idx[s + delta] = val;
                        wave_sync();
                    }
                }
            }
            cnt += delta;
        };
        auto erase = [&](int ia, int ib) { replace(ia, ib, 0); };
        auto next_uniform = [&]() -> double {
            const double u = rng_uniform_k(key, 0x8000000000000000ull + (unsigned long long)n_draws);
            n_draws++;
            return u;
        };
        auto uniform_int = [&](int lo, int hi) -> int {
            const int m = hi - lo + 1;
            const int r = (int)(next_uniform() * (double)m);
            return lo + (r < m - 1 ? r : m - 1);
        };
        auto uniform_real = [&](double lo, double hi) -> double {
            const double w = hi - lo, pr = next_uniform() * w;
            return lo + pr;
        };
        auto reduce = [&]() -> bool {
            const int n = cnt;
            if (!(a.passes & 1) || n < 3) return false;
            if (check(0, cnt - 1)) {
                erase(0, cnt - 1);
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
                // then the lanes' candidates are merged by (distance, i, j): the first minimum of the ascending scan.  A blocked
                // pair is keyed by its two slots, which no vertex changes during this call
                double best = __builtin_inf();
                unsigned best_ij = 0xffffffffu;
                for (int i = 0; i + 2 < cnt; i++) {
                    const unsigned oi = (unsigned)slot(i);
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

        // ---- shortcutPath (LEVEL >= 1; tests/shortcut_ref.py) ----
        // D[k] for k >= from (>= 1) as the ascending cumulative sum; the entries below `from` are those sums already
        auto cumulative = [&](int from) {
            for (int k = from + lane; k < cnt; k += 64) {
                const double *ra = pe + (size_t)idx[k - 1] * nq, *rb = pe + (size_t)idx[k] * nq;
                double d = 0.0;
                for (int c = 0; c < na; c++) d += dist_dim(h, v, c, ra[adr[c]], rb[adr[c]]);
                D[k] = d;
            }
            wave_sync();
            if (lane == 0) {
                double acc = D[from - 1];
                for (int k = from; k < cnt; k++) { acc = acc + D[k]; D[k] = acc; }
            }
            wave_sync();
        };
        // (p, x) of arc length d: x the vertex the point snaps to, or -1 for a point inside segment (p, p + 1)
        auto locate = [&](double d, double thr, int &p_out, int &x_out) {
            int p = cnt - 1;
            for (int base = 0; base < cnt; base += 64) {
                const int k = base + lane;
                const unsigned long long m = __ballot(k < cnt && D[k] >= d);
                if (m) { p = base + __ffsll((long long)m) - 1; break; }
            }
            p = __builtin_amdgcn_readfirstlane(p);
            int x = -1;
            if (p == 0 || uni(D[p] - d < thr)) x = p;
            else {
                while (p > 0 && uni(d < D[p])) p--;
                if (uni(d - D[p] < thr)) x = p;
            }
            if (x < 0 && p >= cnt - 1) x = p;       // (only a NaN among the rows gets here: no segment behind the last vertex)
            p_out = p;
            x_out = x;
        };
        // a new row: row 0's passive entries, the point's active ones
        auto write_row = [&](int s, const double *pt) {
            for (int i = lane; i < na; i += 64) rowbuf[adr[i]] = pt[i];
            wave_sync();
            for (int i = lane; i < nq; i += 64) pe[(size_t)s * nq + i] = rowbuf[i];
            wave_sync();
        };
        auto shortcut = [&]() -> bool {
            const int n = cnt;
            if (!(a.passes & 4) || n < 3) return false;
            if (lane == 0) D[0] = 0.0;
            cumulative(1);
            double total = D[cnt - 1];
            if (uni(total == 0.0)) return false;
            double thr = total * 0.005, rd = 0.33 * total;
            bool result = false;
            int nochange = 0;
            for (int i = 0; i < n && nochange < n; i++, nochange++) {
                double d0 = uniform_real(0.0, total);
                int p0, x0, p1, x1;
                locate(d0, thr, p0, x0);
                const double lo = d0 - rd, hi = d0 + rd;
                double d1 = uniform_real(lo > 0.0 ? lo : 0.0, total < hi ? total : hi);
                locate(d1, thr, p1, x1);
                if (p0 == p1 || x0 == p1 || x1 == p0 || p0 + 1 == x1 || p1 + 1 == x0 ||
                    (x0 >= 0 && x1 >= 0 && (x0 > x1 ? x0 - x1 : x1 - x0) < 2))
                    continue;
                if (p0 > p1) {
                    const double td = d0; d0 = d1; d1 = td;
                    int t = p0; p0 = p1; p1 = t;
                    t = x0; x0 = x1; x1 = t;
                }
                const int ia = x0 < 0 ? 1 : 0, ib = x1 < 0 ? 1 : 0;
                if (ia && ib && p0 + 1 == p1 && cnt == max_path) { n_cap++; continue; }      // one vertex would become two: no slot
                if (ia) {
                    const double t0 = (d0 - D[p0]) / (D[p0 + 1] - D[p0]);
                    const double *ra = pe + (size_t)slot(p0) * nq, *rb = pe + (size_t)slot(p0 + 1) * nq;
                    for (int c = lane; c < na; c += 64) ptA[c] = interp_dim(h, v, c, ra[adr[c]], rb[adr[c]], t0);
                } else load_vertex(ptA, x0);
                if (ib) {
                    const double t1 = (d1 - D[p1]) / (D[p1 + 1] - D[p1]);
                    const double *ra = pe + (size_t)slot(p1) * nq, *rb = pe + (size_t)slot(p1 + 1) * nq;
                    for (int c = lane; c < na; c += 64) ptB[c] = interp_dim(h, v, c, ra[adr[c]], rb[adr[c]], t1);
                } else load_vertex(ptB, x1);
                wave_sync();
                // A-B, then the stub in front of an interior A, then the stub behind an interior B
                load_point(ends, ptA);
                load_point(ends + na, ptB);
                bool ok = check_ends();
                if (ok && ia) {
                    load_vertex(ends, p0);
                    load_point(ends + na, ptA);
                    ok = check_ends();
                }
                if (ok && ib) {
                    load_point(ends, ptB);
                    load_vertex(ends + na, p1 + 1);
                    ok = check_ends();
                }
                if (!ok) continue;
                const int a_end = ia ? p0 : x0, s_start = ib ? p1 + 1 : x1;
                replace(a_end, s_start, ia + ib);              // (cnt is the new count from here on)
                // the erased vertices' slots are on the stack by now: the new rows may take them, A and B are in LDS
                const int top = max_path - cnt;               // free slots left once the new ones are taken
                const int sA = ia ? __builtin_amdgcn_readfirstlane((int)freel[top + ia + ib - 1]) : 0;
                const int sB = ib ? __builtin_amdgcn_readfirstlane((int)freel[top]) : 0;
                if (lane == 0) {
                    if (ia) idx[a_end + 1] = (unsigned short)sA;
                    if (ib) idx[a_end + 1 + ia] = (unsigned short)sB;
                }
                wave_sync();
                if (ia) write_row(sA, ptA);
                if (ib) write_row(sB, ptB);
                if (cnt > max_cnt) max_cnt = cnt;
                n_splices++;
                cumulative(a_end + 1);
                total = D[cnt - 1];
                thr = total * 0.005;
                rd = 0.33 * total;
                nochange = 0;
                result = true;
            }
            return result;
        };

        // ---- smoothBSpline (LEVEL 2; tests/smooth_ref.py) ----
        // the verdict of segment (k, k + 1) as the vertices stand: checked at most once per step
        auto seg = [&](int k) -> bool {
            int vk = __builtin_amdgcn_readfirstlane((int)vd[k]) & 3;
            if (vk == 0) {
                vk = check(k, k + 1) ? 1 : 2;
                if (lane == 0) vd[k] = (unsigned char)(vd[k] | vk);
                wave_sync();
            }
            return vk == 1;
        };
        auto smooth = [&]() {
            if (cnt < 3) return;
            if (lane == 0) D[0] = 0.0;
            cumulative(1);
            const double min_change = D[cnt - 1] / 100.0;          // of the path as it came in: not recomputed between steps
            for (int step = 0; step < 3; step++) {
                const int n0 = cnt, n = 2 * n0 - 1, top = max_path - n0;
                if (n > max_path) { n_cap++; return; }              // no slots for the midpoints: the smoothing ends here
                // subdivide: vertex k goes to position 2k (from the top down, 64 entries at a time: a chunk's targets lie
                // above every source still to be read), the midpoint behind it takes a free slot
                for (int hi = n0; hi > 1; hi -= 64) {
                    const int s = hi - 1 - lane;
                    const unsigned short val = s >= 1 ? idx[s] : (unsigned short)0;
                    wave_sync();
                    if (s >= 1) idx[2 * s] = val;
                    wave_sync();
                }
                for (int k = lane; k < n0 - 1; k += 64) idx[2 * k + 1] = freel[top - 1 - k];
                for (int k = lane; k < n; k += 64) vd[k] = 0;
                for (int k = lane; k < ((n + 31) >> 5); k += 64) mvw[k] = 0u;
                wave_sync();
                cnt = n;
                if (cnt > max_cnt) max_cnt = cnt;
                n_steps++;
                // the midpoints' rows: row 0's passive entries, then the interpolated active ones
                for (int j = lane; j < (n0 - 1) * nq; j += 64) {
                    const int k = j / nq, i = j - k * nq;
                    pe[(size_t)idx[2 * k + 1] * nq + i] = rowbuf[i];
                }
                wave_sync();
                for (int j = lane; j < (n0 - 1) * na; j += 64) {
                    const int k = j / na, c = j - k * na;
                    const double *ra = pe + (size_t)idx[2 * k] * nq, *rb = pe + (size_t)idx[2 * k + 2] * nq;
                    pe[(size_t)idx[2 * k + 1] * nq + adr[c]] = interp_dim(h, v, c, ra[adr[c]], rb[adr[c]], 0.5);
                }
                wave_sync();
                // the state check of the midpoint in front of every candidate i = 2, 4, ... < n - 1, kMS states per validity
                // pass: the candidates read odd positions and their own vertex only, so none depends on another
                const int nc = n0 - 2;
                for (int c0 = 0; c0 < nc; c0 += kMS) {
                    const int ns = nc - c0 < kMS ? nc - c0 : kMS;
                    for (int j = lane; j < ns * na; j += 64) {
                        const int s = j / na, c = j - s * na;
                        ms.qs[j] = pe[(size_t)idx[2 * (c0 + s) + 1] * nq + adr[c]];
                    }
                    wave_sync();
                    const unsigned okm = (unsigned)__builtin_amdgcn_readfirstlane(
                        (int)plan_states_valid_ms(lh, v.dbl, v.ints, ms.grec, ms.qbuf, ms.wl, ms.qs, lane, ns, pe));
                    if (lane < ns && ((okm >> lane) & 1u)) vd[2 * (c0 + lane) + 2] = 4;
                    n_state += ns;
                    wave_sync();
                }
                // the candidates in order: OMPL's two checks and the change, then -- a deviation -- the outer halves of the
                // two segments next to the vertex, whose verdicts depend on what moved before
                int u = 0;
                for (int i = 2; i < n - 1; i += 2) {
                    if (!(__builtin_amdgcn_readfirstlane((int)vd[i]) & 4)) continue;
                    const double *rm = pe + (size_t)slot(i - 1) * nq, *ri = pe + (size_t)slot(i) * nq, *rp = pe + (size_t)slot(i + 1) * nq;
                    for (int c = lane; c < na; c += 64) {
                        const double t1 = interp_dim(h, v, c, rm[adr[c]], ri[adr[c]], 0.5);
                        const double t2 = interp_dim(h, v, c, ri[adr[c]], rp[adr[c]], 0.5);
                        ptA[c] = interp_dim(h, v, c, t1, t2, 0.5);
                    }
                    wave_sync();
                    load_vertex(ends, i - 1);
                    load_point(ends + na, ptA);
                    if (!check_ends()) continue;
                    load_point(ends, ptA);
                    load_vertex(ends + na, i + 1);
                    if (!check_ends()) continue;
                    double d = 0.0;
                    for (int c = 0; c < na; c++) d += dist_dim(h, v, c, ri[adr[c]], ptA[c]);
                    if (!uni(d > min_change)) continue;
                    if (!seg(i - 2) || !seg(i + 1)) continue;
                    for (int c = lane; c < na; c += 64) pe[(size_t)slot(i) * nq + adr[c]] = ptA[c];
                    if (lane == 0) {        // the two segments at the vertex are exactly the two checks just made
                        vd[i - 1] = (unsigned char)((vd[i - 1] & ~3) | 1);
                        vd[i] = (unsigned char)((vd[i] & ~3) | 1);
                        mvw[i >> 5] |= 1u << (i & 31);
                    }
                    wave_sync();
                    u++;
                }
                if (u == 0) {           // (a deviation) nothing moved: the path as before the step, the popped slots are on the stack still
                    for (int base = 1; base < n0; base += 64) {
                        const int s = base + lane;
                        const unsigned short val = s < n0 ? idx[2 * s] : (unsigned short)0;
                        wave_sync();
                        if (s < n0) idx[s] = val;
                        wave_sync();
                    }
                    cnt = n0;
                    return;
                }
                n_moved += u;
                // (a deviation) a midpoint between two vertices that stayed is kept only if both its halves pass
                for (int k = 0; k < n0 - 1; k++) {
                    const unsigned w0 = mvw[(2 * k) >> 5], w1 = mvw[(2 * k + 2) >> 5];
                    if (uni((((w0 >> ((2 * k) & 31)) | (w1 >> ((2 * k + 2) & 31))) & 1u) != 0u)) continue;
                    if (seg(2 * k) && seg(2 * k + 1)) continue;
                    if (lane == 0) vd[2 * k + 1] |= 8;
                    n_dropped++;
                }
                wave_sync();
                // the kept positions to the front in order, the slots of the dropped midpoints back onto the stack
                int out = 0, n_out = 0;
                const int top2 = max_path - n;
                for (int base = 0; base < n; base += 64) {
                    const int k = base + lane;
                    const bool in = k < n, keep = in && !(vd[k] & 8);
                    const unsigned short val = in ? idx[k] : (unsigned short)0;
                    const unsigned long long mk = __ballot(keep), md = __ballot(in && !keep), lt = (1ull << lane) - 1ull;
                    wave_sync();
                    if (keep) idx[out + __popcll(mk & lt)] = val;
                    else if (in) freel[top2 + n_out + __popcll(md & lt)] = val;
                    out += __popcll(mk);
                    n_out += __popcll(md);
                    wave_sync();
                }
                cnt = out;
            }
        };

        // PathSimplifier::simplify's loop; from LEVEL 1 on max_rounds stands in for its wall-clock condition (the vertex passes
        // alone always come to rest)
        bool try_more = true;
        while (try_more && (LEVEL == 0 || rounds < a.max_rounds)) {
            rounds++;
            if constexpr (LEVEL >= 1) {
                if (a.passes & 4) {
                    int times = 0;
                    bool m;
                    do { m = shortcut(); } while (++times <= 5 && m);
                }
            }
            if constexpr (LEVEL >= 2) {
                if (a.passes & 8) smooth();
            }
            try_more = reduce();
            collapse();
            for (int times = 0; try_more && times < 5; times++) try_more = reduce();
        }

        if constexpr (LEVEL == 0) {
            // compaction in place, ascending (target row <= source row; row 0 never moves)
            for (int k = 1; k < cnt; k++) {
                const int src = slot(k);
                if (src != k)
                    for (int i = lane; i < nq; i += 64) pe[(size_t)k * nq + i] = pe[(size_t)src * nq + i];
            }
        } else {
            // the rows into order, in place: vertex k's row comes to row k; the row that lay there goes to the slot this frees when
            // a later vertex still needs it (row 0 never moves)
            for (int k = 1; k < cnt; k++) {
                const int src = slot(k);
                if (src == k) continue;
                int user = -1;                    // the later vertex whose row lies in slot k
                for (int base = k + 1; base < cnt; base += 64) {
                    const int j = base + lane;
                    const unsigned long long m = __ballot(j < cnt && (int)idx[j] == k);
                    if (m) { user = base + __ffsll((long long)m) - 1; break; }
                }
                user = __builtin_amdgcn_readfirstlane(user);
                for (int i = lane; i < nq; i += 64) {
                    const double mine = pe[(size_t)src * nq + i];
                    if (user >= 0) pe[(size_t)src * nq + i] = pe[(size_t)k * nq + i];
                    pe[(size_t)k * nq + i] = mine;
                }
                if (lane == 0) {
                    if (user >= 0) idx[user] = (unsigned short)src;
                    idx[k] = (unsigned short)k;
                }
                wave_sync();
            }
        }
        if (lane == 0) {
            a.path_len[e] = cnt;
            if (a.info) {
                long long *o = a.info + k9_info_cols(LEVEL) * e;
                o[0] = n_checks; o[1] = n_draws;
                if constexpr (LEVEL >= 1) { o[2] = rounds; o[3] = n_splices; o[4] = n_cap; o[5] = max_cnt; }
                if constexpr (LEVEL >= 2) { o[6] = n_steps; o[7] = n_moved; o[8] = n_dropped; o[9] = n_state; }
            }
        }
        wave_sync();
    }
}

#define MOPA_K9_KERNEL(name_, level_)                                                                                                          \
    __global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void name_(SceneHdr h, const double *__restrict__ g_dbl, \
                                                                                              const int32_t *__restrict__ g_int, K9Args a) { \
        k9_paths_body<level_>(h, g_dbl, g_int, a);                                                                                             \
    }
MOPA_K9_KERNEL(k_simplify_paths, 0)
MOPA_K9_KERNEL(k_shortcut_paths, 1)
MOPA_K9_KERNEL(k_smooth_paths, 2)
#undef MOPA_K9_KERNEL

typedef void (*K9Kernel)(SceneHdr, const double *, const int32_t *, K9Args);
static const K9Kernel kK9Kernels[3] = {k_simplify_paths, k_shortcut_paths, k_smooth_paths};

static const LdsKernels kK9Lds({(const void *)k_simplify_paths, (const void *)k_shortcut_paths, (const void *)k_smooth_paths});

// one wave's LDS behind the header copy, and the whole workgroup's
static int k9_wave_bytes(int level, const MopaScene *S, int max_path) {
    int b = k9_list_bytes(level < 1 ? 0 : 1, S->na, S->nq, max_path);
    if (level >= 2)
        b += k9_flag_bytes(max_path) + ms_bytes_per_wave(S->hdr.nmg, S->na, S->hdr.n_pq, ms_sc_doubles(S->hdr.nmj, S->hdr.nmb), S->hdr.npair);
    return b;
}
static int k9_lds_bytes(int level, const MopaScene *S, int max_path) {
    return ((S->lds_bytes + 15) & ~15) + (((int)sizeof(SceneHdr) + 15) & ~15) + kWavesPerBlock * k9_wave_bytes(level, S, max_path);
}
// the paddings of a level's lists stay below 4 rows' worth
static int k9_max_path(int level, const MopaScene *S) {
    if (!S) return -1;
    int mp = (kMaxLdsBytes - k9_lds_bytes(level, S, 0)) / (k9_row_bytes(level) * kWavesPerBlock) - 4;
    return std::max(0, std::min(mp, 65535));        // (16-bit slots)
}

static int k9_launch(int level, MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev, const int32_t *status_dev,
                     uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev, const uint64_t *seeds_dev, int32_t passes,
                     int32_t max_rounds, int64_t *info_dev, void *stream) {
    static const char *const what[3] = {"simplification", "shortcutting", "smoothing"};
    const int top = (4 << level) - 1;           // passes: 1..3, 1..7, 1..15
    if (!S || (E > 0 && (!path_dev || !path_len_dev))) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    MOPA_REFUSE_GLUED(S, std::string("path ") + what[level]);
    if (E < 0 || max_path < 2 || passes < 1 || passes > top || (level >= 1 && max_rounds < 1))
        return fail(MOPA_ERR_INVALID_ARG, "E < 0, max_path < 2" + std::string(level ? "," : " or") + " passes outside 1.." + std::to_string(top) +
                                              (level ? " or max_rounds < 1" : ""));
    if (max_path > k9_max_path(level, S) || k9_lds_bytes(level, S, max_path) > kMaxLdsBytes)
        return fail(MOPA_ERR_UNSUPPORTED, std::string("path ") + what[level] + ": max_path beyond what the per-wave LDS lists hold (" +
                                              std::to_string(k9_max_path(level, S)) + ")");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(S->device);
    K9Args a;
    a.path = path_dev; a.path_len = path_len_dev; a.status = status_dev; a.E = (long long)E; a.max_path = max_path; a.passes = passes;
    a.max_rounds = max_rounds; a.seed = seed; a.env_id_base = env_id_base;
    a.env_ids = reinterpret_cast<const unsigned long long *>(env_ids_dev); a.seeds = reinterpret_cast<const unsigned long long *>(seeds_dev);
    a.info = reinterpret_cast<long long *>(info_dev);
    a.hdr_lds_off = (S->lds_bytes + 15) & ~15;
    a.list_lds_off = a.hdr_lds_off + (((int)sizeof(SceneHdr) + 15) & ~15);
    a.list_bytes = k9_wave_bytes(level, S, max_path);
    hipLaunchKernelGGL(kK9Kernels[level], dim3(grid_for(S, E)), dim3(kBlock), k9_lds_bytes(level, S, max_path), (hipStream_t)stream, S->hdr,
                       S->d_dbl, S->d_int, a);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_simplify_paths_max_path(const MopaScene *S) { return k9_max_path(0, S); }
extern "C" int mopa_shortcut_paths_max_path(const MopaScene *S) { return k9_max_path(1, S); }
extern "C" int mopa_smooth_paths_max_path(const MopaScene *S) { return k9_max_path(2, S); }

extern "C" int mopa_simplify_paths_batch(MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev,
                                         const int32_t *status_dev, uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev,
                                         const uint64_t *seeds_dev, int32_t passes, int64_t *info_dev, void *stream) {
    return k9_launch(0, S, E, max_path, path_dev, path_len_dev, status_dev, seed, env_id_base, env_ids_dev, seeds_dev, passes, 0, info_dev, stream);
}
extern "C" int mopa_shortcut_paths_batch(MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev,
                                         const int32_t *status_dev, uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev,
                                         const uint64_t *seeds_dev, int32_t passes, int32_t max_rounds, int64_t *info_dev, void *stream) {
    return k9_launch(1, S, E, max_path, path_dev, path_len_dev, status_dev, seed, env_id_base, env_ids_dev, seeds_dev, passes, max_rounds, info_dev,
                     stream);
}
extern "C" int mopa_smooth_paths_batch(MopaScene *S, int64_t E, int32_t max_path, double *path_dev, int32_t *path_len_dev,
                                       const int32_t *status_dev, uint64_t seed, uint64_t env_id_base, const uint64_t *env_ids_dev,
                                       const uint64_t *seeds_dev, int32_t passes, int32_t max_rounds, int64_t *info_dev, void *stream) {
    return k9_launch(2, S, E, max_path, path_dev, path_len_dev, status_dev, seed, env_id_base, env_ids_dev, seeds_dev, passes, max_rounds, info_dev,
                     stream);
}
