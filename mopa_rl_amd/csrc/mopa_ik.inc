// mopa_ik.inc -- K5: batched damped-least-squares IK of a site pose (position, or position + orientation; SURVEY.md 8f row 3).
// (included by mopa_hip.hip; C ABI in include/mopa_hip.h "mopa_ik_*")
//
// Restates reference env/inverse_kinematics.py:18-135 (`qpos_from_site_pose`, target_pos [+ target_quat]) + `nullspace_method`
// :274-281 -- see the ABI comment for the iteration.  Mapping: one LANE per env, one wave per workgroup.  Every
// iteration walks the ancestor chain of the site's body (FK with the pose in registers, per-body records through
// scalar loads), parks world axis + anchor of every movable joint in LDS ([col][6][64] doubles), forms the 3 x n
// position Jacobian, the n x n normal matrix J^T J + lambda I (n <= 8, padded with identity rows so that the fully
// unrolled 8 x 8 Cholesky needs no dynamic register indexing) and applies the capped update.  Lanes whose env has
// converged (or given up) idle until the slowest env of the wave is done.  Same operation order as the CPU checker.

constexpr int kIkMaxJ = 8;

struct IkHdr {
    int nq, nb, n_save, n_joints, site_k;
    int o_bi, o_bd, o_col_type, o_col_adr, o_off, o_smat, has_smat;
    int n_pre;     // leading bodies of the site's chain without a joint (Sawyer: base, right_arm_base_link): their poses do not change over a solve
};

struct MopaIk {
    int device = 0;
    IkHdr hdr{};
    double *d_dbl = nullptr;
    int32_t *d_int = nullptr;
    ~MopaIk() {
        if (d_dbl) (void)hipFree(d_dbl);
        if (d_int) (void)hipFree(d_int);
    }
};

// per closure body: jn, load, save, jt, qadr, col (Jacobian column of its joint or -1), pad, pad
struct alignas(32) IkBodyI { int jn, load, save, jt, qadr, col, pad0, pad1; };

MOPA_D void ik_chol_solve(double (&H)[kIkMaxJ][kIkMaxJ], const double (&g)[kIkMaxJ], double (&x)[kIkMaxJ]) {
    // (one division per pivot, inv[j] = 1 / L[j][j], and products with it where 44 divisions stood -- the checker's ik_chol_solve alike)
    double y[kIkMaxJ], inv[kIkMaxJ];
#pragma unroll
    for (int j = 0; j < kIkMaxJ; j++) {       // H is overwritten by its Cholesky factor L (lower triangle)
        double d = H[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) d = fma(-H[j][k], H[j][k], d);
        H[j][j] = sqrt(d);
        inv[j] = 1.0 / H[j][j];
#pragma unroll
        for (int i = j + 1; i < kIkMaxJ; i++) {
            double s = H[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) s = fma(-H[i][k], H[j][k], s);
            H[i][j] = s * inv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < kIkMaxJ; i++) {
        double s = g[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = fma(-H[i][k], y[k], s);
        y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = kIkMaxJ - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < kIkMaxJ; k++) s = fma(-H[k][i], x[k], s);
        x[i] = s * inv[i];
    }
}

// One lane's solve: the iteration of `k_ik_solve` and of the fused position-only pre-step `k_ik_displacement_pos`.  `row` is the lane's
// qpos row (read: the joints on the chain that are not movable), `qj_io` the movable joints' values -- in: the start, out: the result --,
// `cols` / `save` the wave's LDS ([kIkMaxJ][6][64] and [n_save][7][64] doubles).  steps_io / success_io / err_norm_io as IKResult; the caller
// presets steps = max_steps - 1, success = 0, err_norm = 0.  `__any` inside: every lane of the wave calls it, idle ones with active = false.
// ROT: position + orientation target (6 x n Jacobian [jacp; jacr], inverse_kinematics.py:38-44,88-107)
template <bool ROT>
MOPA_D void ik_solve_lane(const IkHdr &h, const double *__restrict__ GD, const int32_t *__restrict__ GI, const double *__restrict__ row,
                          double (&qj_io)[kIkMaxJ], const V3 tgt, const Q4 tq, double rot_weight, int max_steps, double tol,
                          double max_update_norm, double progress_thresh, double reg, double *cols, double *save, const int lane,
                          bool active, double &err_norm_io, int &steps_io, int &success_io) {
    // (the solve works on locals of its own and hands them back at the end: updated through the caller's references, hipcc kept the joint values,
    //  the error norm and the two flags in 80 B of scratch per lane)
    double qj[kIkMaxJ];
#pragma unroll
    for (int k = 0; k < kIkMaxJ; k++) qj[k] = qj_io[k];
    double err_norm = err_norm_io;
    int steps = steps_io, success = success_io;
    for (int c = 0; c < kIkMaxJ; c++)          // columns of joints that are not on the site's chain stay zero
        for (int i = 0; i < 6; i++) cols[(c * 6 + i) * 64 + lane] = 0.0;
    V3 pos0{0.0, 0.0, 0.0};
    Q4 quat0{1.0, 0.0, 0.0, 0.0};

    for (int step = 0; step < max_steps; step++) {
        if (!__any(active)) break;
        // ---- FK along the ancestor chain of the site's body (the jointless bodies at its root are posed in the first iteration only: what they
        //      hand on -- pose0 -- is the same in every iteration, by the same arithmetic) ----
        V3 pos{0.0, 0.0, 0.0}, psite{0.0, 0.0, 0.0}, err_rot{0.0, 0.0, 0.0};
        Q4 quat{1.0, 0.0, 0.0, 0.0};
        double mat[9];
        const int b_first = (step > 0) ? h.n_pre : 0;
        if (b_first > 0) { pos = pos0; quat = quat0; quat2mat(mat, quat0); }
        for (int b = b_first; b < h.nb; b++) {
            const IkBodyI bi = *reinterpret_cast<const IkBodyI *>(GI + h.o_bi + 8 * b);
            const double *bd = GD + h.o_bd + 16 * b;   // pos[3] quat[4] axis[3] jpos[3] ref
            if (bi.jn == 1 && bi.jt == J_FREE) {
                const double *qp = row + bi.qadr;
                fk_free_step(qp, pos, quat);
            } else {
                V3 ppos;
                Q4 pquat;
                if (bi.load == -2) {
                    ppos = V3{0.0, 0.0, 0.0};
                    pquat = Q4{1.0, 0.0, 0.0, 0.0};
                    quat2mat(mat, pquat);
                } else if (bi.load >= 0) {
                    const double *sp = save + (size_t)bi.load * 7 * 64 + lane;
                    pose7_ld<64>(sp, ppos, pquat);
                    quat2mat(mat, pquat);
                } else {
                    ppos = pos;
                    pquat = quat;
                }
                pos = add3(ppos, mat_vec(mat, ld3(bd)));
                quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
                if (bi.jn == 1) {
                    const V3 jp = ld3(bd + 10);
                    double qv;
                    if (bi.col >= 0) {          // a movable joint: its running value (wave-uniform column index)
                        qv = qj[0];
#pragma unroll
                        for (int k = 1; k < kIkMaxJ; k++) qv = (bi.col == k) ? qj[k] : qv;
                    } else qv = row[bi.qadr];
                    apply_joint(bi.jt, ld3(bd + 7), jp, is_zero3(jp), qv - bd[13], pos, quat);
                }
                quat = quat_normalize(quat);
            }
            quat2mat(mat, quat);
            if (b + 1 == h.n_pre) { pos0 = pos; quat0 = quat; }
            if (bi.save >= 0) {
                double *sp = save + (size_t)bi.save * 7 * 64 + lane;
                pose7_st<64>(sp, pos, quat);
            }
            if (bi.col >= 0) {       // [3P] mj_jacSite inputs: joint axis and anchor in the world frame
                const V3 ax = mat_vec(mat, ld3(bd + 7));
                const V3 an = add3(pos, mat_vec(mat, ld3(bd + 10)));
                double *cp = cols + (size_t)bi.col * 6 * 64 + lane;
                cp[0] = ax.x; cp[64] = ax.y; cp[128] = ax.z; cp[192] = an.x; cp[256] = an.y; cp[320] = an.z;
            }
            if (b == h.site_k) {
                psite = add3(pos, mat_vec(mat, ld3(GD + h.o_off)));
                if (ROT) {      // :88-93  err_rot = quat2Vel(target_quat * conj(mat2Quat(site_xmat)), 1)
                    Q4 sq;
                    if (h.has_smat) {
                        const double *sl = GD + h.o_smat;
                        double sm[9];
#pragma unroll
                        for (int r = 0; r < 3; r++)
#pragma unroll
                            for (int c = 0; c < 3; c++)
                                sm[3 * r + c] = fma(mat[3 * r + 2], sl[6 + c], fma(mat[3 * r + 1], sl[3 + c], mat[3 * r] * sl[c]));
                        sq = mj_mat2quat(sm);
                    } else sq = mj_mat2quat(mat);
                    err_rot = mj_quat2vel(quat_mul(tq, Q4{sq.w, -sq.x, -sq.y, -sq.z}));
                }
            }
        }
        const V3 err = sub3(tgt, psite);
        double en_now = norm3(err);
        if (ROT) en_now = en_now + norm3(err_rot) * rot_weight;
        err_norm = active ? en_now : err_norm;
        if (active && err_norm < tol) { success = 1; steps = step; active = false; }
        // ---- J, J^T J + lambda I, J^T err ----
        double J[ROT ? 6 : 3][kIkMaxJ];
#pragma unroll
        for (int k = 0; k < kIkMaxJ; k++) {
            const double *cp = cols + (size_t)k * 6 * 64 + lane;
            const V3 ax{cp[0], cp[64], cp[128]};
            const bool slide = GI[h.o_col_type + k] == J_SLIDE;
            V3 cv;
            if (slide) cv = ax;
            else cv = cross3(ax, sub3(psite, V3{cp[192], cp[256], cp[320]}));
            J[0][k] = cv.x; J[1][k] = cv.y; J[2][k] = cv.z;
            if constexpr (ROT) {          // [3P] mj_jacSite jacr: hinge = world axis, slide = 0
                J[3][k] = slide ? 0.0 : ax.x; J[4][k] = slide ? 0.0 : ax.y; J[5][k] = slide ? 0.0 : ax.z;
            }
        }
        double H[kIkMaxJ][kIkMaxJ], g[kIkMaxJ], x[kIkMaxJ];
#pragma unroll
        for (int i = 0; i < kIkMaxJ; i++) {
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double hh = fma(J[2][i], J[2][j], fma(J[1][i], J[1][j], J[0][i] * J[0][j]));
                if constexpr (ROT) hh = fma(J[5][i], J[5][j], fma(J[4][i], J[4][j], fma(J[3][i], J[3][j], hh)));
                H[i][j] = hh;
            }
            H[i][i] = (i < h.n_joints) ? H[i][i] + reg : 1.0;
            double gi = fma(J[2][i], err.z, fma(J[1][i], err.y, J[0][i] * err.x));
            if constexpr (ROT) gi = fma(J[5][i], err_rot.z, fma(J[4][i], err_rot.y, fma(J[3][i], err_rot.x, gi)));
            g[i] = gi;
        }
        ik_chol_solve(H, g, x);
        double un2 = 0.0;
#pragma unroll
        for (int i = 0; i < kIkMaxJ; i++) un2 = (i < h.n_joints) ? fma(x[i], x[i], un2) : un2;
        const double update_norm = sqrt(un2);
        if (active && err_norm / update_norm > progress_thresh) { steps = step; active = false; }
        if (active) {
            const bool cap = update_norm > max_update_norm;
            const double sc = cap ? max_update_norm / update_norm : 1.0;
#pragma unroll
            for (int k = 0; k < kIkMaxJ; k++)
                if (k < h.n_joints) qj[k] = qj[k] + (cap ? x[k] * sc : x[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < kIkMaxJ; k++) qj_io[k] = qj[k];
    err_norm_io = err_norm; steps_io = steps; success_io = success;
}

template <bool ROT>
__global__ __launch_bounds__(64) void k_ik_solve(IkHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                 double *__restrict__ qpos, const double *__restrict__ target,
                                                 const double *__restrict__ target_quat, double rot_weight, int max_steps, double tol,
                                                 double max_update_norm, double progress_thresh, double reg,
                                                 double *__restrict__ err_norm_out, int *__restrict__ steps_out,
                                                 unsigned char *__restrict__ success_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cols = reinterpret_cast<double *>(smem);                 // [kIkMaxJ][6][64]: world axis, anchor
    double *save = cols + kIkMaxJ * 6 * 64;                          // [n_save][7][64]
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * 64 + lane;
    const bool in_range = e0 < E;
    const long long e = in_range ? e0 : E - 1;
    double *row = qpos + e * h.nq;
    const V3 tgt = ld3(target + 3 * e);
    Q4 tq{1.0, 0.0, 0.0, 0.0};
    if (ROT) tq = Q4{target_quat[4 * e], target_quat[4 * e + 1], target_quat[4 * e + 2], target_quat[4 * e + 3]};
    int steps = max_steps - 1, success = 0;
    double err_norm = 0.0;
    // the movable joints' values live in registers for the whole solve (written back once, at the end): updated through the qpos row they made
    // a store -> load round trip through memory in every iteration's chain walk
    double qj[kIkMaxJ];
#pragma unroll
    for (int k = 0; k < kIkMaxJ; k++) qj[k] = (k < h.n_joints) ? row[GI[h.o_col_adr + k]] : 0.0;
    ik_solve_lane<ROT>(h, GD, GI, row, qj, tgt, tq, rot_weight, max_steps, tol, max_update_norm, progress_thresh, reg, cols, save, lane, in_range,
                       err_norm, steps, success);
    if (in_range) {
#pragma unroll
        for (int k = 0; k < kIkMaxJ; k++)
            if (k < h.n_joints) row[GI[h.o_col_adr + k]] = qj[k];
        err_norm_out[e] = err_norm;
        steps_out[e] = steps;
        success_out[e] = (unsigned char)success;
    }
}

// The chain walk of the site's pose at `row` (the solver's first iteration without its Jacobian columns): psite = world position of the
// site, mat = world orientation of its body (row-major).  `save`: the wave's [n_save][7][64] doubles of LDS.
MOPA_D void ik_site_walk(const IkHdr &h, const double *__restrict__ GD, const int32_t *__restrict__ GI, const double *__restrict__ row,
                         double *save, const int lane, V3 &psite, double (&smat)[9]) {
    V3 pos{0.0, 0.0, 0.0};
    Q4 quat{1.0, 0.0, 0.0, 0.0};
    double mat[9];
    for (int b = 0; b < h.nb; b++) {
        const IkBodyI bi = *reinterpret_cast<const IkBodyI *>(GI + h.o_bi + 8 * b);
        const double *bd = GD + h.o_bd + 16 * b;
        if (bi.jn == 1 && bi.jt == J_FREE) {
            const double *qp = row + bi.qadr;
            fk_free_step(qp, pos, quat);
        } else {
            V3 ppos;
            Q4 pquat;
            if (bi.load == -2) {
                ppos = V3{0.0, 0.0, 0.0};
                pquat = Q4{1.0, 0.0, 0.0, 0.0};
                quat2mat(mat, pquat);
            } else if (bi.load >= 0) {
                const double *sp = save + (size_t)bi.load * 7 * 64 + lane;
                pose7_ld<64>(sp, ppos, pquat);
                quat2mat(mat, pquat);
            } else {
                ppos = pos;
                pquat = quat;
            }
            pos = add3(ppos, mat_vec(mat, ld3(bd)));
            quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
            if (bi.jn == 1) {
                const V3 jp = ld3(bd + 10);
                apply_joint(bi.jt, ld3(bd + 7), jp, is_zero3(jp), row[bi.qadr] - bd[13], pos, quat);
            }
            quat = quat_normalize(quat);
        }
        quat2mat(mat, quat);
        if (bi.save >= 0) {
            double *sp = save + (size_t)bi.save * 7 * 64 + lane;
            pose7_st<64>(sp, pos, quat);
        }
    }
    // (the chain ends at the site's body: mopa_ik_create walks up from it, site_k = nb - 1)
    psite = add3(pos, mat_vec(mat, ld3(GD + h.o_off)));
#pragma unroll
    for (int k = 0; k < 9; k++) smat[k] = mat[k];
}

// World pose of the site for E states: what the MoPA+IK rollouts read before they pose the IK problem
// (`env.sim.data.get_site_xpos / get_site_xmat(config.ik_target)`, rl/mopa_rollouts.py:91-99,692).  Same chain walk as the solver.
__global__ __launch_bounds__(64) void k_ik_site_pose(IkHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                     const double *__restrict__ qpos, double *__restrict__ site_pos,
                                                     double *__restrict__ site_mat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *save = reinterpret_cast<double *>(smem);                 // [n_save][7][64]
    const int lane = threadIdx.x;
    const long long e = (long long)blockIdx.x * 64 + lane;
    if (e >= E) return;
    V3 psite{0.0, 0.0, 0.0};
    double mat[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    ik_site_walk(h, GD, GI, qpos + e * h.nq, save, lane, psite, mat);
    st3(site_pos + 3 * e, psite);
    const double *sl = GD + h.o_smat;       // identity when the site carries no rotation of its own
    double *out = site_mat + 9 * e;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            out[3 * r + c] = h.has_smat ? fma(mat[3 * r + 2], sl[6 + c], fma(mat[3 * r + 1], sl[3 + c], mat[3 * r] * sl[c])) : mat[3 * r + c];
}

// The IK problem of the MoPA + IK action space posed for E envs in one launch, one lane per env (`MoPARolloutRunner._cart2dispalcement`,
// rl/mopa_rollouts.py:87-99,681-696 -- what mopa_rl_amd/rollout.py::ik_displacement used to spell as ~70 elementwise torch launches):
//     target_cart = clip(site_xpos + action_range * ac[:3], world box)
//     q_site      = quaternion of the FLOAT32-rounded site matrix (np.array(rmat, dtype=np.float32), util/env.py:232-288; closed form,
//                   branch on the largest of (trace, m00, m11, m22), normalised, w >= 0)
//     target_quat = mulQuat(q_site[(w, x, y, y)], ac[3:7] / |ac[3:7]|)          (the reference indexes [3, 0, 1, 1] of (x, y, z, w): sic)
// Operation for operation the torch expressions it replaces (no contraction; sums left to right).
__global__ __launch_bounds__(64) void k_ik_targets(long long E, const double *__restrict__ site_pos, const double *__restrict__ site_mat,
                                                   const double *__restrict__ ac, long long ac_stride, double action_range,
                                                   double lo0, double lo1, double lo2, double hi0, double hi1, double hi2,
                                                   double *__restrict__ target_cart, double *__restrict__ target_quat) {
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const double *a = ac + e * ac_stride;
    const double lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double t = site_pos[3 * e + i] + action_range * a[i];
        const double u = (t > lo[i]) ? t : lo[i];
        target_cart[3 * e + i] = (u < hi[i]) ? u : hi[i];
    }
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = (double)(float)site_mat[9 * e + k];
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const double tr = (m00 + m11) + m22;
    int pick = 0;
    double best = tr;
    if (m00 > best) { best = m00; pick = 1; }
    if (m11 > best) { best = m11; pick = 2; }
    if (m22 > best) { best = m22; pick = 3; }
    double q0, q1, q2, q3;
    if (pick == 0) { q0 = 1.0 + tr; q1 = m21 - m12; q2 = m02 - m20; q3 = m10 - m01; }
    else if (pick == 1) { q0 = m21 - m12; q1 = ((1.0 + m00) - m11) - m22; q2 = m01 + m10; q3 = m02 + m20; }
    else if (pick == 2) { q0 = m02 - m20; q1 = m01 + m10; q2 = ((1.0 - m00) + m11) - m22; q3 = m12 + m21; }
    else { q0 = m10 - m01; q1 = m02 + m20; q2 = m12 + m21; q3 = ((1.0 - m00) - m11) + m22; }
    const double nq = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    q0 = q0 / nq; q1 = q1 / nq; q2 = q2 / nq; q3 = q3 / nq;
    if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    const double aw = q0, ax = q1, ay = q2, az = q2;
    const double na = sqrt(((a[3] * a[3] + a[4] * a[4]) + a[5] * a[5]) + a[6] * a[6]);
    const double bw = a[3] / na, bx = a[4] / na, by = a[5] / na, bz = a[6] / na;
    double *tq = target_quat + 4 * e;
    tq[0] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    tq[1] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    tq[2] = ((aw * by - ax * bz) + ay * bw) + az * bx;
    tq[3] = ((aw * bz + ax * by) - ay * bx) + az * bw;
}

// The position-only IK problem of the MoPA + IK action space (an env whose world box has n_cart = 2 or 3 entries and whose action has no
// `quat` entry -- PusherObstacle-v0; rl/mopa_rollouts.py:91-98,684-690): components below n_cart = clip(site + action_range * ac, box),
// the others = the site's own.  A product, then a sum (no contraction: the numpy expression, bit for bit); np.clip's comparisons.
MOPA_D V3 ik_target_pos(const V3 site, const double *__restrict__ a, int n_cart, double action_range, const double (&lo)[3], const double (&hi)[3]) {
    const double sp[3] = {site.x, site.y, site.z};
    double out[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        out[i] = sp[i];
        if (i < n_cart) {
            const double t = sp[i] + action_range * a[i];
            const double u = (t < lo[i]) ? lo[i] : t;
            out[i] = (u > hi[i]) ? hi[i] : u;
        }
    }
    return V3{out[0], out[1], out[2]};
}

__global__ __launch_bounds__(64) void k_ik_targets_pos(long long E, const double *__restrict__ site_pos, const double *__restrict__ ac,
                                                       long long ac_stride, int n_cart, double action_range, double lo0, double lo1, double lo2,
                                                       double hi0, double hi1, double hi2, double *__restrict__ target_cart) {
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const double lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
    st3(target_cart + 3 * e, ik_target_pos(ld3(site_pos + 3 * e), ac + e * ac_stride, n_cart, action_range, lo, hi));
}

// The whole pre-step of a position-only MoPA + IK rollout call in one launch, one lane per env (`_cart2dispalcement` with target_quat = None,
// rl/mopa_rollouts.py:683-728): site pose of qpos -> the target above -> the solve of k_ik_solve<false> on the lane's own copy of the movable
// joints (qpos is only read) -> clip to jnt_lo / jnt_hi -> displacement = clipped - qpos[movable].  The pieces are the separate launches'
// own routines, so the result is theirs bit for bit (k_ik_site_pose, k_ik_targets_pos, k_ik_solve<false>, then torch's maximum / minimum /
// subtraction: a NaN stays a NaN).
__global__ __launch_bounds__(64) void k_ik_displacement_pos(IkHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                            const double *__restrict__ qpos, const double *__restrict__ ac, long long ac_stride,
                                                            int n_cart, double action_range, double lo0, double lo1, double lo2, double hi0,
                                                            double hi1, double hi2, int max_steps, double tol, double max_update_norm,
                                                            double progress_thresh, double reg, const double *__restrict__ jnt_lo,
                                                            const double *__restrict__ jnt_hi, double *__restrict__ displacement,
                                                            double *__restrict__ err_norm_out, int *__restrict__ steps_out,
                                                            unsigned char *__restrict__ success_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *cols = reinterpret_cast<double *>(smem);                 // [kIkMaxJ][6][64]: world axis, anchor
    double *save = cols + kIkMaxJ * 6 * 64;                          // [n_save][7][64]
    const int lane = threadIdx.x;
    const long long e0 = (long long)blockIdx.x * 64 + lane;
    const bool in_range = e0 < E;
    const long long e = in_range ? e0 : E - 1;      // (lanes behind the last env walk its row and write nothing)
    const double *row = qpos + e * h.nq;
    V3 psite{0.0, 0.0, 0.0};
    double smat[9];
    ik_site_walk(h, GD, GI, row, save, lane, psite, smat);
    const double lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
    const V3 tgt = ik_target_pos(psite, ac + e * ac_stride, n_cart, action_range, lo, hi);
    int steps = max_steps - 1, success = 0;
    double err_norm = 0.0;
    double qj[kIkMaxJ];
#pragma unroll
    for (int k = 0; k < kIkMaxJ; k++) qj[k] = (k < h.n_joints) ? row[GI[h.o_col_adr + k]] : 0.0;
    ik_solve_lane<false>(h, GD, GI, row, qj, tgt, Q4{1.0, 0.0, 0.0, 0.0}, 0.0, max_steps, tol, max_update_norm, progress_thresh, reg, cols, save,
                         lane, in_range, err_norm, steps, success);
    if (in_range) {
#pragma unroll
        for (int k = 0; k < kIkMaxJ; k++)
            if (k < h.n_joints) {
                const double u = (qj[k] < jnt_lo[k]) ? jnt_lo[k] : qj[k];
                const double c = (u > jnt_hi[k]) ? jnt_hi[k] : u;
                displacement[e * h.n_joints + k] = c - row[GI[h.o_col_adr + k]];
            }
        if (err_norm_out) err_norm_out[e] = err_norm;
        if (steps_out) steps_out[e] = steps;
        if (success_out) success_out[e] = (unsigned char)success;
    }
}

// Host half of IK creation: every argument check, the model's structure, then the compile -- the header into S.hdr, the tables into B.
// No device.
static int ik_build_host(const MopaIkDesc *desc, MopaIk &S, BlobPacker &B) {
    if (!desc) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const MopaModel &m = desc->model;
    if (m.nq <= 0 || m.nbody <= 0) return fail(MOPA_ERR_INVALID_ARG, "empty model");
    if (desc->n_joints <= 0 || desc->n_joints > kIkMaxJ) return fail(MOPA_ERR_LIMIT, "IK supports 1..8 movable joints");
    if (desc->site_body <= 0 || desc->site_body >= m.nbody) return fail(MOPA_ERR_INVALID_ARG, "site_body out of range");
    if (const int rc = check_model_structure(m)) return rc;

    // ancestor chain of the site's body, root first (a chain: no branching, no save slots needed -- kept general)
    std::vector<int> body_of;
    for (int b = desc->site_body; b > 0; b = m.body_parent[b]) body_of.push_back(b);
    std::reverse(body_of.begin(), body_of.end());
    const int nb = (int)body_of.size();

    std::vector<int32_t> col_of_joint(m.njnt, -1), col_type(kIkMaxJ, J_HINGE), col_adr(kIkMaxJ, 0);
    for (int c = 0; c < desc->n_joints; c++) {
        const int j = desc->joint_ids[c];
        if (j < 0 || j >= m.njnt) return fail(MOPA_ERR_INVALID_ARG, "joint id out of range");
        if (m.jnt_type[j] != J_HINGE && m.jnt_type[j] != J_SLIDE) return fail(MOPA_ERR_UNSUPPORTED, "IK joints must be hinge or slide");
        // (a joint has one column: listed twice, the first of its columns would stay zero and the solve would differ from the checker's)
        if (col_of_joint[j] >= 0) return fail(MOPA_ERR_INVALID_ARG, "IK: joint id " + std::to_string(j) + " is listed twice");
        col_of_joint[j] = c;
        col_type[c] = m.jnt_type[j];
        col_adr[c] = m.jnt_qposadr[j];
    }
    std::vector<int32_t> bi(8 * (size_t)nb, 0);
    std::vector<double> bd(16 * (size_t)nb, 0.0);
    for (int k = 0; k < nb; k++) {
        const int b = body_of[k];
        const int jn = m.body_jntnum[b];
        if (jn > 1) return fail(MOPA_ERR_UNSUPPORTED, "IK: bodies on the site's chain may carry at most one joint");
        fill_body_record(m, b, &bd[16 * (size_t)k]);
        int32_t *r = &bi[8 * (size_t)k];
        r[0] = jn;
        r[1] = (k == 0) ? -2 : -1;   // a chain: the parent is always the previous body
        r[2] = -1;
        r[3] = -1; r[5] = -1;
        if (jn == 1) {
            const int j = m.body_jntadr[b];
            if (m.jnt_type[j] == J_BALL) return fail(MOPA_ERR_UNSUPPORTED, "ball joints are not supported");
            r[3] = m.jnt_type[j];
            r[4] = m.jnt_qposadr[j];
            r[5] = col_of_joint[j];
        }
    }
    IkHdr &h = S.hdr;
    h.nq = m.nq; h.nb = nb; h.n_save = 0; h.n_joints = desc->n_joints; h.site_k = nb - 1;
    h.o_bi = B.add_i(bi);
    h.o_bd = B.add_d(bd);
    h.o_col_type = B.add_i(col_type);
    h.o_col_adr = B.add_i(col_adr);
    {
        int n_pre = 0;
        while (n_pre < nb - 1 && m.body_jntnum[body_of[n_pre]] == 0) n_pre++;      // (never the site's own body: its frame closes the walk)
        h.n_pre = (desc->n_joints > 0 && !std::getenv("MOPA_IK_NO_PREFIX")) ? n_pre : 0;
    }
    h.o_off = B.add_d(desc->site_off, 3);
    {
        const double *sq = desc->site_quat;
        const bool ident = (sq[0] == 0.0 && sq[1] == 0.0 && sq[2] == 0.0 && sq[3] == 0.0) || (sq[0] == 1.0 && sq[1] == 0.0 && sq[2] == 0.0 && sq[3] == 0.0);
        double sm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (!ident) quat2mat(sm, Q4{sq[0], sq[1], sq[2], sq[3]});
        h.o_smat = B.add_d(sm, 9);
        h.has_smat = ident ? 0 : 1;
    }
    return MOPA_OK;
}

extern "C" int mopa_ik_create(const MopaIkDesc *desc, MopaIk **out) {
    if (!desc || !out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    auto S = std::make_unique<MopaIk>();
    BlobPacker B;
    if (const int rc = ik_build_host(desc, *S, B)) return rc;
    if (const int rc = pick_device(desc->device, &S->device, "no HIP device available (this library has no CPU fallback)")) return rc;
    DeviceGuard guard(S->device);
    if (!guard.ok()) return fail(MOPA_ERR_HIP, "hipSetDevice failed");
    if (upload_tables(B.D, B.I, &S->d_dbl, &S->d_int) != hipSuccess) return fail(MOPA_ERR_HIP, "device allocation / upload of the IK tables failed");
    *out = S.release();
    return MOPA_OK;
}

// The host half alone: status, and for an accepted description the fingerprint of what mopa_ik_create would upload (header -- all
// ints, no padding --, double table, int table) with the chain's body count.
extern "C" int mopa_ik_tables_host(const MopaIkDesc *desc, uint64_t *fingerprint, int32_t *nb) {
    MopaIk S;
    BlobPacker B;
    if (const int rc = ik_build_host(desc, S, B)) return rc;
    Fnv f;
    f.add(&S.hdr, sizeof(IkHdr));
    f.add(B.D);
    f.add(B.I);
    if (fingerprint) *fingerprint = f.f;
    if (nb) *nb = S.hdr.nb;
    return MOPA_OK;
}

extern "C" void mopa_ik_destroy(MopaIk *ik) { delete ik; }

extern "C" int mopa_ik_solve_batch(MopaIk *ik, int64_t E, double *qpos_dev, const double *target_pos_dev, const double *target_quat_dev,
                                   double rot_weight, int32_t max_steps, double tol, double max_update_norm, double progress_thresh,
                                   double reg_strength, double *err_norm_dev, int32_t *steps_dev, uint8_t *success_dev, void *stream) {
    if (!ik) return fail(MOPA_ERR_INVALID_ARG, "null ik");
    if (E < 0 || max_steps <= 0) return fail(MOPA_ERR_INVALID_ARG, "negative E or max_steps <= 0");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !target_pos_dev || !err_norm_dev || !steps_dev || !success_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (!(reg_strength > 0.0)) return fail(MOPA_ERR_UNSUPPORTED, "regularization_strength must be > 0 (the reference always regularises: inverse_kinematics.py:113-115)");
    ON_DEVICE(ik->device);
    const size_t lds = ((size_t)kIkMaxJ * 6 * 64 + (size_t)std::max(ik->hdr.n_save, 1) * 7 * 64) * sizeof(double);
    const dim3 grid((unsigned)((E + 63) / 64));
    if (target_quat_dev)
        hipLaunchKernelGGL(k_ik_solve<true>, grid, dim3(64), lds, (hipStream_t)stream, ik->hdr, ik->d_dbl, ik->d_int, (long long)E, qpos_dev,
                           target_pos_dev, target_quat_dev, rot_weight, (int)max_steps, tol, max_update_norm, progress_thresh, reg_strength,
                           err_norm_dev, steps_dev, success_dev);
    else
        hipLaunchKernelGGL(k_ik_solve<false>, grid, dim3(64), lds, (hipStream_t)stream, ik->hdr, ik->d_dbl, ik->d_int, (long long)E, qpos_dev,
                           target_pos_dev, (const double *)nullptr, 0.0, (int)max_steps, tol, max_update_norm, progress_thresh, reg_strength,
                           err_norm_dev, steps_dev, success_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_ik_site_pose_batch(MopaIk *ik, int64_t E, const double *qpos_dev, double *site_pos_dev, double *site_mat_dev, void *stream) {
    if (!ik) return fail(MOPA_ERR_INVALID_ARG, "null ik");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !site_pos_dev || !site_mat_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(ik->device);
    const size_t lds = (size_t)std::max(ik->hdr.n_save, 1) * 7 * 64 * sizeof(double);
    hipLaunchKernelGGL(k_ik_site_pose, dim3((unsigned)((E + 63) / 64)), dim3(64), lds, (hipStream_t)stream, ik->hdr, ik->d_dbl, ik->d_int,
                       (long long)E, qpos_dev, site_pos_dev, site_mat_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_ik_targets_batch(MopaIk *ik, int64_t E, const double *site_pos_dev, const double *site_mat_dev, const double *ac_dev,
                                     int64_t ac_stride, double action_range, const double *world_lo, const double *world_hi,
                                     double *target_cart_dev, double *target_quat_dev, void *stream) {
    if (!ik) return fail(MOPA_ERR_INVALID_ARG, "null ik");
    if (E < 0 || ac_stride < 7) return fail(MOPA_ERR_INVALID_ARG, "negative E or an action row shorter than 7 (Cartesian displacement + quaternion)");
    if (E == 0) return MOPA_OK;
    if (!site_pos_dev || !site_mat_dev || !ac_dev || !world_lo || !world_hi || !target_cart_dev || !target_quat_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(ik->device);
    hipLaunchKernelGGL(k_ik_targets, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (long long)E, site_pos_dev, site_mat_dev, ac_dev,
                       (long long)ac_stride, action_range, world_lo[0], world_lo[1], world_lo[2], world_hi[0], world_hi[1], world_hi[2],
                       target_cart_dev, target_quat_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

static int ik_pos_action_args(const MopaIk *ik, int64_t E, int64_t ac_stride, int32_t n_cart) {
    if (!ik) return fail(MOPA_ERR_INVALID_ARG, "null ik");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (n_cart < 2 || n_cart > 3) return fail(MOPA_ERR_INVALID_ARG, "n_cart must be 2 or 3 (the entries of the env's world box)");
    if (ac_stride < n_cart) return fail(MOPA_ERR_INVALID_ARG, "an action row shorter than n_cart");
    return MOPA_OK;
}

extern "C" int mopa_ik_targets_pos_batch(MopaIk *ik, int64_t E, const double *site_pos_dev, const double *ac_dev, int64_t ac_stride,
                                         int32_t n_cart, double action_range, const double *world_lo, const double *world_hi,
                                         double *target_cart_dev, void *stream) {
    if (const int rc = ik_pos_action_args(ik, E, ac_stride, n_cart)) return rc;
    if (!site_pos_dev || !ac_dev || !world_lo || !world_hi || !target_cart_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(ik->device);
    const double lo2 = n_cart > 2 ? world_lo[2] : 0.0, hi2 = n_cart > 2 ? world_hi[2] : 0.0;
    hipLaunchKernelGGL(k_ik_targets_pos, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (long long)E, site_pos_dev, ac_dev,
                       (long long)ac_stride, (int)n_cart, action_range, world_lo[0], world_lo[1], lo2, world_hi[0], world_hi[1], hi2, target_cart_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_ik_displacement_pos_batch(MopaIk *ik, int64_t E, const double *qpos_dev, const double *ac_dev, int64_t ac_stride, int32_t n_cart,
                                              double action_range, const double *world_lo, const double *world_hi, int32_t max_steps, double tol,
                                              double max_update_norm, double progress_thresh, double reg_strength, const double *jnt_lo_dev,
                                              const double *jnt_hi_dev, double *displacement_dev, double *err_norm_dev, int32_t *steps_dev,
                                              uint8_t *success_dev, void *stream) {
    if (const int rc = ik_pos_action_args(ik, E, ac_stride, n_cart)) return rc;
    if (max_steps <= 0) return fail(MOPA_ERR_INVALID_ARG, "max_steps <= 0");
    if (!qpos_dev || !ac_dev || !world_lo || !world_hi || !jnt_lo_dev || !jnt_hi_dev || !displacement_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (!(reg_strength > 0.0)) return fail(MOPA_ERR_UNSUPPORTED, "regularization_strength must be > 0 (the reference always regularises: inverse_kinematics.py:113-115)");
    if (E == 0) return MOPA_OK;
    ON_DEVICE(ik->device);
    const size_t lds = ((size_t)kIkMaxJ * 6 * 64 + (size_t)std::max(ik->hdr.n_save, 1) * 7 * 64) * sizeof(double);
    const double lo2 = n_cart > 2 ? world_lo[2] : 0.0, hi2 = n_cart > 2 ? world_hi[2] : 0.0;
    hipLaunchKernelGGL(k_ik_displacement_pos, dim3((unsigned)((E + 63) / 64)), dim3(64), lds, (hipStream_t)stream, ik->hdr, ik->d_dbl, ik->d_int,
                       (long long)E, qpos_dev, ac_dev, (long long)ac_stride, (int)n_cart, action_range, world_lo[0], world_lo[1], lo2, world_hi[0],
                       world_hi[1], hi2, (int)max_steps, tol, max_update_norm, progress_thresh, reg_strength, jnt_lo_dev, jnt_hi_dev,
                       displacement_dev, err_norm_dev, steps_dev, success_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
