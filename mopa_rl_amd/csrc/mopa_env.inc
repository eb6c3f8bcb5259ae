// mopa_env.inc -- K4: batched KINEMATIC env.step of the Sawyer obstacle envs (SURVEY.md 8f row 1; push / lift / assembly).
// (included by mopa_hip.hip; C ABI in include/mopa_hip.h "mopa_env_*")
//
// What it restates (reference file:line) and what it replaces is documented on the ABI.  Mapping: one LANE
// per env, 64 envs per workgroup (one wave).  The frames the obs/reward need (sites, bodies, for Lift the can and
// the six finger boxes) pull in ~20 bodies of the kinematic tree; the wave walks that closure in DFS order with
// the pose (pos + quat) in registers, wave-uniform per-body records through scalar loads, and the few branch
// points of the tree parked in LDS save slots ([slot][7][64] doubles).  Every arithmetic step is the same
// sequence as in the CPU checker (tests), so obs, reward and flags can be compared bit for bit.
// The three env kinds are separate instantiations (KIND template parameter): frame slots are compile-time indices,
// and only Lift's carries the narrow phase (finger boxes vs the can's hull) of its grasp test.
// HBM per env-step (push): qpos row read (+ arm entries written) 288+56 B, action 56 B, prev_state 2x56 B,
// obs 320 B (f64), reward/flags/counters ~18 B  =>  ~0.85 KB; the kernel is latency- not bandwidth-bound.

constexpr int kEnvMaxFrames = 5, kEnvMaxTouch = 7, kEnvMaxAct = 12;

struct EnvHdr {
    int kind, nq, n_arm, n_grip, n_act, nb, n_save, n_frames, n_touch, n_touch_left, obs_dim, adim;
    int frame_k[kEnvMaxFrames];         // closure index of the body carrying frame f
    int quat_k[2];
    int touch_k[kEnvMaxTouch];          // closure index of the body carrying touch geom g (0 = the object)
    int o_bi, o_bd, o_j_type, o_j_qadr, o_j_axis, o_j_pos, o_j_ref, o_arm, o_grip, o_act, o_act_lo, o_act_hi, o_lim, o_lo, o_hi, o_off, o_tg;
    int max_episode_steps;
    double ac_scale, distance_threshold, success_reward;
};

// servo dynamics attached to an env (mopa_dyn.inc)
constexpr int kDynMax = 9;           // dofs per env the dynamics kernel keeps
struct DynHdr {
    int nd, n_save, nsub;
    int parent[kDynMax], jtype[kDynMax], qadr[kDynMax], load[kDynMax], save[kDynMax], limited[kDynMax], actuated[kDynMax],
        gravcomp[kDynMax], act_of[kDynMax];      // act_of: index of the env actuator (ctrl entry) driving the dof, -1 = none
    int arm_dof[8], grip_dof[4];                 // dof index of the env's arm / gripper joints (obs velocities)
    double gx, gy, gz, h;
    // stage B: the manipulated object (free body, penalty contacts).  obj_on = 0: it rests where it is.
    int obj_on, obj_qadr, obj_nfeat, obj_ncol, nv;      // nv: width of a qvel row = nd (+ 6: the object's v, w)
    int co_first[kDynMax + 2];                   // colliders [co_first[b + 1], co_first[b + 2]) ride on dynamic body b; b = -1: static ones
    double o_mass, o_in0, o_in1, o_in2, o_damp, o_h0, o_h1, o_h2, o_rbound, o_kn, o_dn, o_eps2, o_ctmax;
    double o_imass, o_iin0, o_iin1, o_iin2, o_margin;
    int o_every;
    // workgroup-per-64-envs form (k_env_dyn4): which bodies' inertia / force (own4) and which rows of M (rows4) wave w computes
    unsigned own4[4], rows4[4];
};
struct DynObs { int nd, nv; int arm_dof[8], grip_dof[4]; };   // what the obs needs of it

// Contact-force readout of the solver-backed contact stages (K7, K8; mopa_env_set_contact_force): after the last sub-step of a launch the
// kernel writes, per env that ran a sub-step, force [E] (sum over the contacts of the last constraint solve of |f0| + .. + |f5| of what
// mj_contactForce returns), total [E] += force, rows [E, K, 8] = (pair, key, f0 .. f5) per contact, count [E].  force == nullptr: off.
struct CfOut {
    double *force, *total, *rows;
    int32_t *count;
    int K;
};

struct MopaEnv {
    int device = 0;
    EnvHdr hdr{};
    double *d_dbl = nullptr;
    int32_t *d_int = nullptr;
    std::vector<int32_t> h_int;       // host copy of the int blob (attach_dynamics resolves actuator / joint addresses)
    double *d_dyn = nullptr;          // per-dof records of the dynamics kernel, nullptr = kinematic env
    double *d_obj = nullptr;          // stage B: [feature points | collider records] of the manipulated object
    DynHdr dyn{};
    DynHdr *d_dynhdr = nullptr;       // the same header in device memory (the kernel reads it through scalar loads)
    size_t dyn_lds = 0;
    bool dyn_slot_shared = false;     // two bodies of the dynamic tree park their pose in one save slot: launched in the single-wave form
    // stage C (mopa_contact.inc): [shape | feature | pair] tables, header, LDS bytes of a 4-env workgroup, optional counters
    double *d_ct = nullptr;
    size_t ct_ft_off = 0, ct_pr_off = 0;
    struct CtHdr *d_cthdr = nullptr;
    size_t ct_lds = 0;
    bool ct_on = false;
    int ct_solver = 0;      // 0: projected Gauss-Seidel, 1: Newton (pyramidal cones), 2: Newton (elliptic cones)
    int ct_arena = 0;       // solver 2: LDS slots (doubles) the contact records of an env share
    int ct_maxcon = 0;      // contacts an env keeps per sub-step (rows of a contact-force readout)
    int32_t *ct_stats = nullptr;
    // K8 (mopa_pusher_dyn.inc): the Pusher dynamics attached to this env, freed with it
    void *pusher = nullptr;
    void (*pusher_free)(void *) = nullptr;
    int pusher_maxcon = 0;
    CfOut cf{nullptr, nullptr, nullptr, nullptr, 0};      // contact-force readout of K7 / K8, off by default
    // waypoint execution scratch (one slot per env and waypoint), per stream, grow-only; outgrown buffers are retired and
    // freed with the handle (a kernel in flight may still read them)
    std::mutex mu;
    std::map<hipStream_t, DevBuf> exec_scratch;
    std::vector<void *> retired;
    ~MopaEnv() {
        if (d_dbl) (void)hipFree(d_dbl);
        if (d_int) (void)hipFree(d_int);
        if (d_dyn) (void)hipFree(d_dyn);
        if (d_dynhdr) (void)hipFree(d_dynhdr);
        if (d_obj) (void)hipFree(d_obj);
        if (d_ct) (void)hipFree(d_ct);
        if (d_cthdr) (void)hipFree((void *)d_cthdr);
        for (auto &kv : exec_scratch)
            if (kv.second.p) (void)hipFree(kv.second.p);
        for (void *q : retired) (void)hipFree(q);
        if (pusher_free) pusher_free(pusher);
    }
};

struct alignas(32) EnvBodyI { int jn, jntadr, load, save, jt, qadr, pad0, pad1; };

constexpr int env_nframes(int kind) { return kind == 1 ? 3 : (kind == 3 ? 4 : 5); }
constexpr int kTgStride = 12;    // touch geom record in the blob: local pos[3] quat[4] size[3] type rbound

// `_step`'s desired state of one arm joint: prev_state + clip(action [* ac_scale]) -- the planner's action comes unscaled.
// Pusher (env/pusher/pusher_obstacle.py:262-266): `desired_state = self._prev_state + action` overrides both scaled forms.
// The one statement of the rule: K4's env_advance / k_env_exec_pre / k_env_desired and the dynamics kernels' dyn_command
// (mopa_dyn.inc) call it; the ctrl-range and joint-limit clamps that follow differ per caller and stay with them.
__device__ __forceinline__ double env_desired(const EnvHdr &h, double pv, double a0, int is_planner, bool pusher) {
    return pusher ? pv + a0 : pv + clampd(is_planner ? a0 : a0 * h.ac_scale, -h.ac_scale, h.ac_scale);
}

// The state change of one env.step on one qpos row (`_step` around the physics + the joint-limit clamp): desired_state =
// prev_state + clip(action [* ac_scale]), the actuated joints reach their ctrl-range clamped targets (kinematic limit of
// the position servos), prev[] <- desired_state.  act: the env's action row, or nullptr when stepping from a trajectory row.
// RS / PS: element strides of `row` / `prev` (1 for rows in global memory, 64 for a row kept per lane in LDS).
template <int KIND, int RS = 1, int PS = 1>
__device__ __forceinline__ void env_advance(const EnvHdr &h, const double *__restrict__ GD, const int32_t *__restrict__ GI,
                                            double *__restrict__ row, double *__restrict__ prev, bool use_prev, bool move,
                                            const double *__restrict__ act, const double *__restrict__ traj_row, double extra,
                                            int is_planner) {
    // ---- _step: desired_state = prev_state + clip(action [* ac_scale]); ctrl = [desired_state, gripper targets] ----
    for (int j = 0; j < h.n_arm; j++) {
        const int adr = GI[h.o_arm + j];
        const double pv = use_prev ? prev[j * PS] : row[adr * RS];
        // traj_row: the action is env.form_action(next_qpos) = waypoint - current arm state (rl/mopa_rollouts.py:160)
        const double a0 = traj_row ? traj_row[adr] - row[adr * RS] : act[j];
        const double desired = env_desired(h, pv, a0, is_planner, KIND == 3);
        // kinematic limit of the position servo: the joint reaches its (ctrl-range clamped) target
        if (move) row[adr * RS] = clampd(desired, GD[h.o_act_lo + j], GD[h.o_act_hi + j]);
        prev[j * PS] = desired;   // `self._prev_state = np.copy(desired_state)`
    }
    if (KIND == 1) {
        // Lift: gripper_action = gripper qpos + action[-1] for both fingers (sawyer.py:340-342); all targets are formed
        // from the state BEFORE any of them is applied
        const double ga = traj_row ? extra : act[h.n_arm];
        double tgt[kEnvMaxAct];
#pragma unroll
        for (int k = 0; k < 2; k++) tgt[k] = row[GI[h.o_act + h.n_arm + k] * RS] + ga;
        if (move) {
#pragma unroll
            for (int k = 0; k < 2; k++)
                row[GI[h.o_act + h.n_arm + k] * RS] = clampd(tgt[k], GD[h.o_act_lo + h.n_arm + k], GD[h.o_act_hi + h.n_arm + k]);
        }
    }
    // ---- joint-limit clamp (env/base.py:269-290) ----
    // (Pusher: its torque motors have no range that stops a joint at its limit; the clamp comes after reward / obs, as in the reference)
    if (KIND != 3)
        for (int i = 0; i < h.nq; i++)
            if (GI[h.o_lim + i]) row[i * RS] = clampd(row[i * RS], GD[h.o_lo + i], GD[h.o_hi + i]);
}

// One env.step (or, with action == traj_row == nullptr, an obs refresh) of env e on this lane.
// extra: the action entry beyond the arm's (Lift: the gripper command) when stepping from a trajectory row.
template <int KIND>
__device__ __forceinline__ void env_step_lane(const EnvHdr &h, const double *__restrict__ GD, const int32_t *__restrict__ GI,
                                              double *save, int lane, long long e, double *__restrict__ qpos,
                                              double *__restrict__ prev_state, unsigned char *__restrict__ has_prev,
                                              int *__restrict__ ep_len, const double *__restrict__ action,
                                              const double *__restrict__ traj_row, double extra, int is_planner, unsigned flags,
                                              double *__restrict__ obs, double *__restrict__ reward,
                                              unsigned char *__restrict__ done, unsigned char *__restrict__ success,
                                              const double *__restrict__ qvel = nullptr, const DynObs *dob = nullptr) {
    constexpr int NF = env_nframes(KIND);
    double *row = qpos + e * h.nq;
    const bool stepping = action != nullptr || traj_row != nullptr;
    // qvel != nullptr: the servo dynamics (k_env_dyn) already advanced the state and prev_state; this call is the
    // reward / obs / bookkeeping half of the step, the obs reports the joint velocities, and the joint-limit clamp comes
    // AFTER reward and obs, as in the reference (env/base.py:269-290)
    const bool dyn = qvel != nullptr;

    if (stepping && !dyn) {
        env_advance<KIND>(h, GD, GI, row, prev_state + e * h.n_arm, is_planner && has_prev[e], (flags & 1u) != 0,
                          action ? action + e * h.adim : nullptr, traj_row, extra, is_planner);
        has_prev[e] = 1;
    }

    // ---- forward kinematics over the closure of the frame bodies ----
    V3 pos{0.0, 0.0, 0.0};
    Q4 quat{1.0, 0.0, 0.0, 0.0};
    double mat[9];
    V3 P[NF];
    Q4 q_ee{1, 0, 0, 0}, q_obj{1, 0, 0, 0};
    // Lift: posed frames (pos 3 + mat 9) of the can and the finger boxes, parked in LDS behind the save slots ([g][12][64]):
    // the grasp test walks them with a run-time index, and a run-time-indexed local array is scratch memory
    double *tl = save + (size_t)h.n_save * 7 * 64 + lane;
#pragma unroll
    for (int f = 0; f < NF; f++) P[f] = V3{0.0, 0.0, 0.0};
    for (int b = 0; b < h.nb; b++) {
        const EnvBodyI bi = *reinterpret_cast<const EnvBodyI *>(GI + h.o_bi + 8 * b);
        const double *bd = GD + h.o_bd + 16 * b;   // pos[3] quat[4] axis[3] jpos[3] ref
        if (bi.jn == 1 && bi.jt == J_FREE) {
            const double *qp = row + bi.qadr;
            fk_free_step(qp, pos, quat);
        } else {
            V3 ppos;
            Q4 pquat;
            if (bi.load == -2) {            // parent is the world body
                ppos = V3{0.0, 0.0, 0.0};
                pquat = Q4{1.0, 0.0, 0.0, 0.0};
                quat2mat(mat, pquat);
            } else if (bi.load >= 0) {      // parent pose was parked when the DFS left its subtree
                const double *sp = save + (size_t)bi.load * 7 * 64 + lane;
                pose7_ld<64>(sp, ppos, pquat);
                quat2mat(mat, pquat);
            } else {                        // parent is the previous body (mat still holds its rotation)
                ppos = pos;
                pquat = quat;
            }
            const V3 vv = mat_vec(mat, ld3(bd));
            pos = add3(ppos, vv);
            quat = quat_mul(pquat, Q4{bd[3], bd[4], bd[5], bd[6]});
            for (int jj = 0; jj < bi.jn; jj++) {
                V3 ax, jp;
                double ref;
                int jt, qadr;
                if (jj == 0) {
                    ax = ld3(bd + 7); jp = ld3(bd + 10); ref = bd[13]; jt = bi.jt; qadr = bi.qadr;
                } else {
                    const int j = bi.jntadr + jj;
                    ax = ld3(GD + h.o_j_axis + 3 * j); jp = ld3(GD + h.o_j_pos + 3 * j); ref = GD[h.o_j_ref + j];
                    jt = GI[h.o_j_type + j]; qadr = GI[h.o_j_qadr + j];
                }
                const double dq = row[qadr] - ref;
                apply_joint(jt, ax, jp, is_zero3(jp), dq, pos, quat);
            }
            quat = quat_normalize(quat);
        }
        quat2mat(mat, quat);
        if (bi.save >= 0) {
            double *sp = save + (size_t)bi.save * 7 * 64 + lane;
            pose7_st<64>(sp, pos, quat);
        }
        // frames on this body (wave-uniform tests)
#pragma unroll
        for (int f = 0; f < NF; f++)
            if (b == h.frame_k[f]) P[f] = add3(pos, mat_vec(mat, ld3(GD + h.o_off + 3 * f)));
        if (b == h.quat_k[0]) q_ee = quat;
        if (b == h.quat_k[1]) q_obj = quat;
        if (KIND == 1 && stepping) {
#pragma unroll
            for (int g = 0; g < kEnvMaxTouch; g++)
                if (g < h.n_touch && b == h.touch_k[g]) {
                    const double *tg = GD + h.o_tg + kTgStride * g;
                    const V3 tp = add3(pos, mat_vec(mat, ld3(tg)));
                    double tm[9];
                    quat2mat(tm, quat_mul(quat, Q4{tg[3], tg[4], tg[5], tg[6]}));
                    double *tr = tl + (size_t)g * 12 * 64;
                    tr[0] = tp.x; tr[64] = tp.y; tr[128] = tp.z;
#pragma unroll
                    for (int i = 0; i < 9; i++) tr[(3 + i) * 64] = tm[i];
                }
        }
    }

    // ---- compute_reward + _get_obs, per env kind ----
    double r = 0.0;
    bool succ = false;
    double *o = obs + e * h.obs_dim;
    int k = 0;
    const V3 p_eef = P[0];
    if (KIND == 3) {
        // PusherObstacle (env/pusher/pusher_obstacle.py:183-204 `_get_obs`, :223-245 `compute_reward`); frames: 0 site fingertip,
        // 1 body fingertip, 2 body box, 3 body target; the box / goal sliders are the last four qpos entries (:187, :202)
        const V3 tip_site = P[0], tip = P[1], box = P[2], target = P[3];
        for (int j = 0; j < h.n_arm; j++) {
            double sn, cs;
            mopa_sincos(row[GI[h.o_arm + j]], sn, cs);
            o[j] = cs; o[h.n_arm + j] = sn;
        }
        k = 2 * h.n_arm;
        o[k++] = row[h.nq - 2]; o[k++] = row[h.nq - 1];
        // joint and box velocities: 0 in the kinematic limit; with the dynamics (K8) qvel rows are joint0..3, box_x, box_y
        for (int j = 0; j < h.n_arm + 2; j++) o[k++] = dyn ? qvel[e * dob->nv + j] : 0.0;
        o[k++] = tip.x; o[k++] = tip.y;
        o[k++] = row[h.nq - 4]; o[k++] = row[h.nq - 3];
        const double dist_box_to_gripper = norm3(sub3(box, tip_site));
        const double box_to_target = norm3(sub3(box, target));
        double reward_reach = 0.0, reward_push = 0.0;
        if (dist_box_to_gripper < 0.1) reward_reach = 0.1 * (1.0 - mopa_tanh_pos(5.0 * dist_box_to_gripper));
        if (box_to_target < 0.1) reward_push = 0.3 * (1.0 - mopa_tanh_pos(5.0 * box_to_target));
        r = reward_reach + reward_push;
        if (box_to_target < h.distance_threshold) { r += h.success_reward; succ = true; }
    } else {
    for (int j = 0; j < h.n_arm; j++) o[k++] = row[GI[h.o_arm + j]];
    for (int j = 0; j < h.n_arm; j++) o[k++] = dyn ? qvel[e * dob->nv + dob->arm_dof[j]] : 0.0;
    for (int j = 0; j < h.n_grip; j++) o[k++] = row[GI[h.o_grip + j]];
    for (int j = 0; j < h.n_grip; j++) o[k++] = dyn ? qvel[e * dob->nv + dob->grip_dof[j]] : 0.0;
    o[k++] = p_eef.x; o[k++] = p_eef.y; o[k++] = p_eef.z;
    o[k++] = q_ee.x; o[k++] = q_ee.y; o[k++] = q_ee.z; o[k++] = q_ee.w;
    if (KIND == 0) {
        // sawyer_push_obstacle.py:71-119; frames: 1 right_eef, 2 left_eef, 3 cube, 4 target
        const V3 p_rf = P[1], p_lf = P[2], p_cube = P[3], p_target = P[4];
        const V3 grip{(p_rf.x + p_lf.x) / 2.0, (p_rf.y + p_lf.y) / 2.0, (p_rf.z + p_lf.z) / 2.0};
        const double gripper_to_cube = norm3(sub3(p_cube, grip));
        const double c2t0 = p_cube.x - p_target.x, c2t1 = p_cube.y - p_target.y;
        const double cube_to_target = sqrt(fma(c2t1, c2t1, c2t0 * c2t0));
        double reward_reach = 0.0, reward_push = 0.0;
        if (gripper_to_cube < 0.1) reward_reach = 0.1 * (1.0 - mopa_tanh_pos(10.0 * gripper_to_cube));
        if (cube_to_target < 0.1) reward_push = 0.5 * (1.0 - mopa_tanh_pos(5.0 * cube_to_target));
        r = reward_push + reward_reach;
        if (cube_to_target < h.distance_threshold) { r += h.success_reward; succ = true; }
        o[k++] = p_target.x; o[k++] = p_target.y; o[k++] = p_target.z;
        o[k++] = p_cube.x; o[k++] = p_cube.y; o[k++] = p_cube.z;
        o[k++] = q_obj.x; o[k++] = q_obj.y; o[k++] = q_obj.z; o[k++] = q_obj.w;
        o[k++] = p_eef.x - p_cube.x; o[k++] = p_eef.y - p_cube.y; o[k++] = p_eef.z - p_cube.z;
        o[k++] = c2t0; o[k++] = c2t1;
    } else if (KIND == 1) {
        // sawyer_lift_obstacle.py:93-163; frames: 1 the can ("cube"), 2 bin1
        const V3 p_cube = P[1], p_bin = P[2];
        const double reward_reach = (1.0 - mopa_tanh_pos(10.0 * norm3(sub3(p_cube, p_eef)))) * 0.1;
        bool touch_l = false, touch_r = false;
        if (stepping) {
            double R0[kGeomStride];       // the can
#pragma unroll
            for (int i = 0; i < 12; i++) R0[i] = tl[i * 64];
            R0[GO_SIZE] = GD[h.o_tg + 7]; R0[GO_SIZE + 1] = GD[h.o_tg + 8]; R0[GO_SIZE + 2] = GD[h.o_tg + 9];
#pragma unroll 1
            for (int g = 1; g < h.n_touch; g++) {
                // has_grasp: a contact between the can and a finger geom on each side; bounding-sphere cull, then the
                // narrow phase (box vs the can's hull: portal refinement), "contact" = the shapes intersect
                const double *tg = GD + h.o_tg + kTgStride * g, *t0 = GD + h.o_tg;
                double Rg[kGeomStride];
                const double *tr = tl + (size_t)g * 12 * 64;
#pragma unroll
                for (int i = 0; i < 12; i++) Rg[i] = tr[i * 64];
                Rg[GO_SIZE] = tg[7]; Rg[GO_SIZE + 1] = tg[8]; Rg[GO_SIZE + 2] = tg[9];
                const V3 diff = sub3(ld3(R0 + GO_POS), ld3(Rg + GO_POS));
                const double rs = tg[11] + t0[11];
                bool hit = false;
                if (!(dot3(diff, diff) > rs * rs))
                    hit = geom_dist<true>(PC_CONVEX_MESH, Rg, (int)tg[10], R0, G_MESH, GD) < 0.0;
                if (g <= h.n_touch_left) touch_l |= hit; else touch_r |= hit;
            }
        }
        const double reward_grasp = (touch_l && touch_r) ? 0.35 : 0.0;
        double reward_lift = 0.0;
        const double z_target = p_bin.z + 0.45;
        if (reward_grasp > 0.0) {
            const double z_dist = dmax(z_target - p_cube.z, 0.0);
            reward_lift = 0.35 + (1.0 - mopa_tanh_pos(15.0 * z_dist)) * (0.5 - 0.35);
        }
        r = dmax(dmax(reward_reach, reward_grasp), reward_lift);
        if (reward_grasp > 0.0 && fabs(p_cube.z - z_target) < 0.05) { r += h.success_reward; succ = true; }
        o[k++] = p_cube.x; o[k++] = p_cube.y; o[k++] = p_cube.z;
        o[k++] = q_obj.x; o[k++] = q_obj.y; o[k++] = q_obj.z; o[k++] = q_obj.w;
        o[k++] = p_eef.x - p_cube.x; o[k++] = p_eef.y - p_cube.y; o[k++] = p_eef.z - p_cube.z;
    } else {
        // sawyer_assembly_obstacle.py:33-59; frames: 1 hole, 2 hole_bottom, 3 pegHead, 4 pegEnd; quat 1 = body "peg" (wxyz)
        const V3 hole = P[1], bottom = P[2], head = P[3], pend = P[4];
        const double dist = norm3(sub3(head, hole)), dist_bottom = norm3(sub3(head, bottom));
        if (dist < 0.3) r = 0.4 * (1.0 - mopa_tanh_pos(15.0 * dist));
        if (dist_bottom < 0.025) { r += h.success_reward; succ = true; }
        o[k++] = hole.x; o[k++] = hole.y; o[k++] = hole.z;
        o[k++] = head.x; o[k++] = head.y; o[k++] = head.z;
        o[k++] = pend.x; o[k++] = pend.y; o[k++] = pend.z;
        o[k++] = q_obj.w; o[k++] = q_obj.x; o[k++] = q_obj.y; o[k++] = q_obj.z;
    }
    }
    if (stepping) {
        const int len = ep_len[e] + 1;   // env/base.py:296-302
        ep_len[e] = len;
        reward[e] = r;
        success[e] = succ ? 1 : 0;
        done[e] = (succ || len == h.max_episode_steps) ? 1 : 0;
        if (dyn || KIND == 3)
            for (int i = 0; i < h.nq; i++)
                if (GI[h.o_lim + i]) row[i] = clampd(row[i], GD[h.o_lo + i], GD[h.o_hi + i]);
    }
}

// (amdgpu_waves_per_eu(1, 2): a launch is a few dozen waves -- occupancy buys nothing, and at the default target of 3 waves
// per SIMD the Lift instantiation spilled registers to scratch)
template <int KIND>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_env_step(EnvHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                 double *__restrict__ qpos, double *__restrict__ prev_state,
                                                 unsigned char *__restrict__ has_prev, int *__restrict__ ep_len,
                                                 const double *__restrict__ action, int is_planner,
                                                 const unsigned char *__restrict__ move_mask, double *__restrict__ obs,
                                                 double *__restrict__ reward, unsigned char *__restrict__ done,
                                                 unsigned char *__restrict__ success, const double *__restrict__ qvel, DynObs dob) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *save = reinterpret_cast<double *>(smem);   // [n_save][7][64]
    const int lane = threadIdx.x;
    const long long e = (long long)blockIdx.x * 64 + lane;
    if (e >= E) return;   // no block-level barriers below: lanes are independent
    const unsigned flags = (action != nullptr && move_mask) ? move_mask[e] : 1u;   // bit 0: the actuated joints move, bit 1: env sits this step out
    if (flags & 2u) return;
    env_step_lane<KIND>(h, GD, GI, save, lane, e, qpos, prev_state, has_prev, ep_len, action, nullptr, 0.0, is_planner, flags, obs, reward,
                        done, success, qvel, &dob);
}

// Waypoint execution of the rollout (rl/mopa_rollouts.py:152-199) in ONE launch: env e steps through its path_len[e]
// waypoints (action = waypoint - current arm state, is_planner semantics), accumulating the SMDP return
// rew += discount^k * reward_k, until the path ends or a step reports done.  Optional per-waypoint record (obs after the
// step, running return, done flag) = the reference's ob_list / meta_rew_list / done_list.  Same step arithmetic as
// k_env_step, lane for lane; envs with path_len 0 are not touched.  Lift: the gripper entry of a waypoint's action is
// form_action's gripper difference, except at the path's last waypoint where it is the policy's (last_extra, :163-167).
template <int KIND>
__global__ __launch_bounds__(64) void k_env_exec(EnvHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                 double *__restrict__ qpos, double *__restrict__ prev_state,
                                                 unsigned char *__restrict__ has_prev, int *__restrict__ ep_len,
                                                 const double *__restrict__ traj, const long long *__restrict__ path_len, int L,
                                                 const double *__restrict__ disc_pow, const double *__restrict__ last_extra,
                                                 double *__restrict__ obs, double *__restrict__ reward, unsigned char *__restrict__ done,
                                                 unsigned char *__restrict__ success, double *__restrict__ smdp_rew,
                                                 unsigned char *__restrict__ smdp_done, long long *__restrict__ intra,
                                                 double *__restrict__ rec_ob, double *__restrict__ rec_rew,
                                                 unsigned char *__restrict__ rec_done, long long *__restrict__ n_exec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *save = reinterpret_cast<double *>(smem);
    const int lane = threadIdx.x;
    const long long e = (long long)blockIdx.x * 64 + lane;
    if (e >= E) return;
    const long long len = path_len[e] < L ? path_len[e] : L;
    double rew = smdp_rew[e];
    for (long long k = 0; k < len; k++) {
        const double *wp = traj + ((size_t)e * L + k) * h.nq;
        double extra = 0.0;
        if (KIND == 1) {
            const int g0 = GI[h.o_grip];
            extra = (k == len - 1) ? last_extra[e] : wp[g0] - qpos[e * h.nq + g0];
        }
        env_step_lane<KIND>(h, GD, GI, save, lane, e, qpos, prev_state, has_prev, ep_len, nullptr, wp, extra, 1, 1u, obs, reward, done, success);
        rew = rew + disc_pow[k] * reward[e];
        const unsigned char d = done[e];
        smdp_done[e] = d;
        intra[e] = k;
        if (rec_ob) {
            const double *o = obs + e * h.obs_dim;
            double *ro = rec_ob + ((size_t)e * L + k) * h.obs_dim;
            for (int i = 0; i < h.obs_dim; i++) ro[i] = o[i];
            rec_rew[(size_t)e * L + k] = rew;
            rec_done[(size_t)e * L + k] = d;
            n_exec[e] = k + 1;
        }
        if (d) break;      // `if done or ep_len >= max_step: break`
    }
    if (len > 0) smdp_rew[e] = rew;
}

// ---- waypoint execution, all waypoints of all envs side by side -------------------------------------------------
// k_env_exec walks a path one env.step after the other on one lane: a 25-waypoint path costs 25 dependent FK + reward
// evaluations (~25 us each) while 94 % of the chip idles.  Only the STATE CHANGE of a step depends on the step before
// (a handful of additions and clamps); the expensive part -- FK, reward, obs of the state reached -- does not.  So:
//   k_env_exec_pre   lane per env: the state before each of its steps (slot e * L + k), by the cheap part alone
//   k_env_exec_step  lane per (env, waypoint): the full env.step from that state (same code as k_env_step)
//   k_env_exec_fold  lane per env: SMDP return / done / intra_steps in waypoint order, stopping at the first `done`;
//                    the env takes the state, obs and flags of the step it stopped at
// Every value is produced by the arithmetic of the sequential walk, in its order: results are bit-identical.
struct ExecSlots {
    double *q, *prev, *obs, *rew;      // [E L nq], [E L n_arm], [E L obs_dim], [E L]
    int *ep;                           // [E L]
    unsigned char *has, *done, *succ;  // [E L]
};
// (one wave per env, one lane per qpos entry: env_advance's per-entry arithmetic with the row in registers -- every step is a
//  dozen instructions and the slot rows are written coalesced; the lane-per-env form of round 3 took 230 us per call for
//  scattered 8-byte stores)
template <int KIND>
__global__ __launch_bounds__(256) void k_env_exec_pre(EnvHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                      const double *__restrict__ qpos, const double *__restrict__ prev_state,
                                                      const unsigned char *__restrict__ has_prev, const int *__restrict__ ep_len,
                                                      const double *__restrict__ traj, const long long *__restrict__ path_len, int L,
                                                      ExecSlots v) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const long long len = path_len[e] < L ? path_len[e] : L;
    if (len <= 0) return;
    const long long base = e * L;
    const bool on = lane < h.nq;
    int j = -1;                                       // the arm joint this lane's qpos entry belongs to
    for (int k = 0; k < h.n_arm; k++)
        if (GI[h.o_arm + k] == lane) j = k;
    int gk = -1;                                      // Lift: the gripper actuator of this entry
    int g0 = 0;
    if (KIND == 1) {
        g0 = GI[h.o_grip];
        for (int k = 0; k < 2; k++)
            if (GI[h.o_act + h.n_arm + k] == lane) gk = k;
    }
    const double act_lo = j >= 0 ? GD[h.o_act_lo + j] : (gk >= 0 ? GD[h.o_act_lo + h.n_arm + gk] : 0.0);
    const double act_hi = j >= 0 ? GD[h.o_act_hi + j] : (gk >= 0 ? GD[h.o_act_hi + h.n_arm + gk] : 0.0);
    const bool lim = on && GI[h.o_lim + lane] != 0;
    const double lo = on ? GD[h.o_lo + lane] : 0.0, hi = on ? GD[h.o_hi + lane] : 0.0;
    double row = on ? qpos[e * h.nq + lane] : 0.0;
    double pv = j >= 0 ? prev_state[e * h.n_arm + j] : 0.0;
    bool has = has_prev[e] != 0;
    int ep = ep_len[e];
    for (long long k = 0; k < len; k++) {
        const long long s = base + k;          // slot s: the state BEFORE step k
        if (on) v.q[s * h.nq + lane] = row;
        if (j >= 0) v.prev[s * h.n_arm + j] = pv;
        if (lane == 0) {
            v.has[s] = has ? 1 : 0;
            v.ep[s] = ep;
        }
        if (k + 1 == len) break;
        const double wp = on ? traj[s * h.nq + lane] : 0.0;
        // env_advance (is_planner step from a trajectory row): the action is waypoint - current arm state
        if (KIND == 1) {
            // not the path's last waypoint (that one uses the policy's gripper action): gripper entry of form_action
            const double d = wp - row;
            const double ga = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(d), g0), __builtin_amdgcn_readlane(__double2loint(d), g0));
            if (gk >= 0) row = clampd(row + ga, act_lo, act_hi);
        }
        if (j >= 0) {
            const double desired = env_desired(h, has ? pv : row, wp - row, 1, KIND == 3);
            row = clampd(desired, act_lo, act_hi);
            pv = desired;
        }
        if (lim) row = clampd(row, lo, hi);
        has = true;
        ep++;
    }
}
template <int KIND>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_env_exec_step(EnvHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                      const double *__restrict__ traj, const long long *__restrict__ path_len, int L,
                                                      const double *__restrict__ last_extra, ExecSlots v) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *save = reinterpret_cast<double *>(smem);
    const int lane = threadIdx.x;
    const long long s = (long long)blockIdx.x * 64 + lane;
    if (s >= E * L) return;
    const long long e = s / L, k = s - e * L;
    const long long len = path_len[e] < L ? path_len[e] : L;
    if (k >= len) return;
    const double *wp = traj + s * h.nq;
    double extra = 0.0;
    if (KIND == 1) {
        const int g0 = GI[h.o_grip];
        extra = (k == len - 1) ? last_extra[e] : wp[g0] - v.q[s * h.nq + g0];
    }
    env_step_lane<KIND>(h, GD, GI, save, lane, s, v.q, v.prev, v.has, v.ep, nullptr, wp, extra, 1, 1u, v.obs, v.rew, v.done, v.succ);
}
__global__ __launch_bounds__(64) void k_env_exec_fold(EnvHdr h, long long E, double *__restrict__ qpos, double *__restrict__ prev_state,
                                                      unsigned char *__restrict__ has_prev, int *__restrict__ ep_len,
                                                      const long long *__restrict__ path_len, int L, const double *__restrict__ disc_pow,
                                                      double *__restrict__ obs, double *__restrict__ reward, unsigned char *__restrict__ done,
                                                      unsigned char *__restrict__ success, double *__restrict__ smdp_rew,
                                                      unsigned char *__restrict__ smdp_done, long long *__restrict__ intra,
                                                      double *__restrict__ rec_rew, unsigned char *__restrict__ rec_done,
                                                      long long *__restrict__ n_exec, ExecSlots v) {
    const long long e = (long long)blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const long long len = path_len[e] < L ? path_len[e] : L;
    if (len <= 0) return;
    const long long base = e * L;
    double rew = smdp_rew[e];
    long long last = 0;
    unsigned char d = 0;
    for (long long k = 0; k < len; k++) {
        rew = rew + disc_pow[k] * v.rew[base + k];
        d = v.done[base + k];
        last = k;
        if (rec_rew) {
            rec_rew[base + k] = rew;
            rec_done[base + k] = d;
        }
        if (d) break;      // `if done or ep_len >= max_step: break`
    }
    const long long s = base + last;
    if (rec_rew)        // the record shares the slots' obs: rows of steps that were not executed are left as the walk leaves them
        for (long long k = last + 1; k < len; k++)
            for (int i = 0; i < h.obs_dim; i++) v.obs[(base + k) * h.obs_dim + i] = 0.0;
    smdp_rew[e] = rew;
    smdp_done[e] = d;
    intra[e] = last;
    if (n_exec) n_exec[e] = last + 1;
    for (int i = 0; i < h.nq; i++) qpos[e * h.nq + i] = v.q[s * h.nq + i];
    for (int j = 0; j < h.n_arm; j++) prev_state[e * h.n_arm + j] = v.prev[s * h.n_arm + j];
    has_prev[e] = 1;
    ep_len[e] = v.ep[s];
    for (int i = 0; i < h.obs_dim; i++) obs[e * h.obs_dim + i] = v.obs[s * h.obs_dim + i];
    reward[e] = v.rew[s];
    done[e] = v.done[s];
    success[e] = v.succ[s];
}

// desired arm state of the NEXT step as the servo will reach it (ctrl-range and joint-limit clamped), without stepping:
// what the collision gate validates
__global__ __launch_bounds__(256) void k_env_desired(EnvHdr h, const double *__restrict__ GD, const int32_t *__restrict__ GI, long long E,
                                                     const double *__restrict__ qpos, const double *__restrict__ prev_state,
                                                     const unsigned char *__restrict__ has_prev, const double *__restrict__ action,
                                                     int is_planner, double *__restrict__ desired) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * h.n_arm) return;
    const long long e = i / h.n_arm;
    const int j = (int)(i - e * h.n_arm);
    const int adr = GI[h.o_arm + j];
    const double prev = (is_planner && has_prev[e]) ? prev_state[i] : qpos[e * h.nq + adr];
    double d = clampd(env_desired(h, prev, action[e * h.adim + j], is_planner, h.kind == 3), GD[h.o_act_lo + j], GD[h.o_act_hi + j]);
    if (GI[h.o_lim + adr]) d = clampd(d, GD[h.o_lo + adr], GD[h.o_hi + adr]);
    desired[i] = d;
}

// Host half of env creation: every argument check, the model's structure, then the compile -- the header into S.hdr, the tables into B,
// the int table's host copy into S.h_int.  No device.
static int env_build_host(const MopaEnvDesc *desc, MopaEnv &S, BlobPacker &B) {
    if (!desc) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    const MopaModel &m = desc->model;
    if (m.nq <= 0 || m.nbody <= 0) return fail(MOPA_ERR_INVALID_ARG, "empty model");
    const int kind = desc->kind;
    if (kind < MOPA_ENV_PUSH || kind > MOPA_ENV_PUSHER) return fail(MOPA_ERR_INVALID_ARG, "unknown env kind");
    const int nf = env_nframes(kind);
    if (desc->n_frames != nf || desc->n_quats != 2) return fail(MOPA_ERR_INVALID_ARG, "frame / quat slots do not match the env kind (see MopaEnvDesc)");
    if (desc->n_arm <= 0 || desc->n_grip < 0 || desc->n_act < desc->n_arm || desc->n_act > kEnvMaxAct)
        return fail(MOPA_ERR_INVALID_ARG, "bad joint / actuator counts");
    if (kind == MOPA_ENV_LIFT && (desc->n_act != desc->n_arm + 2 || desc->n_touch < 2 || desc->n_touch > kEnvMaxTouch ||
                                  desc->n_touch_left < 1 || desc->n_touch_left >= desc->n_touch - 1 + 1 || desc->n_grip < 1))
        return fail(MOPA_ERR_INVALID_ARG, "lift needs the two gripper actuators and touch geoms [object, left..., right...]");
    if (kind != MOPA_ENV_LIFT && desc->n_act != desc->n_arm) return fail(MOPA_ERR_INVALID_ARG, "push / assembly are actuated through the arm's servos only");
    std::vector<int> fb;
    for (int f = 0; f < nf; f++) fb.push_back(desc->frame_body[f]);
    for (int f = 0; f < 2; f++) fb.push_back(desc->quat_body[f]);
    const int n_touch = kind == MOPA_ENV_LIFT ? desc->n_touch : 0;
    for (int g = 0; g < n_touch; g++) {
        const int cg = desc->touch_geom[g];
        if (cg < 0 || cg >= m.ngeom) return fail(MOPA_ERR_INVALID_ARG, "touch geom index out of range");
        if (g == 0 ? (m.geom_type[cg] != G_MESH || !m.geom_dataid || m.geom_dataid[cg] < 0) : (m.geom_type[cg] != G_BOX))
            return fail(MOPA_ERR_UNSUPPORTED, "lift grasp test: the object must be a mesh geom and the finger geoms boxes");
        fb.push_back(m.geom_body[cg]);
    }
    for (int b : fb)
        if (b <= 0 || b >= m.nbody) return fail(MOPA_ERR_INVALID_ARG, "frame body id out of range");
    for (int j = 0; j < desc->n_arm; j++)
        if (desc->arm_qpos_idx[j] < 0 || desc->arm_qpos_idx[j] >= m.nq || desc->act_qpos_idx[j] != desc->arm_qpos_idx[j])
            return fail(MOPA_ERR_INVALID_ARG, "arm_qpos_idx out of range, or the first actuators are not the arm's");
    for (int j = 0; j < desc->n_act; j++)
        if (desc->act_qpos_idx[j] < 0 || desc->act_qpos_idx[j] >= m.nq) return fail(MOPA_ERR_INVALID_ARG, "act_qpos_idx out of range");
    for (int j = 0; j < desc->n_grip; j++)
        if (desc->grip_qpos_idx[j] < 0 || desc->grip_qpos_idx[j] >= m.nq) return fail(MOPA_ERR_INVALID_ARG, "grip_qpos_idx out of range");
    if (const int rc = check_model_structure(m)) return rc;

    // closure of the frame bodies, in id (= DFS preorder) order
    std::vector<char> needed(m.nbody, 0);
    for (int b : fb)
        for (int c = b; c > 0 && !needed[c]; c = m.body_parent[c]) needed[c] = 1;
    std::vector<int> k_of(m.nbody, -1), body_of;
    for (int b = 1; b < m.nbody; b++)
        if (needed[b]) { k_of[b] = (int)body_of.size(); body_of.push_back(b); }
    const int nb = (int)body_of.size();

    std::vector<int32_t> bi(8 * (size_t)nb, 0), j_type, j_qadr, parent_k(nb);
    std::vector<double> bd(16 * (size_t)nb, 0.0), j_axis, j_pos, j_ref;
    for (int k = 0; k < nb; k++) {
        const int b = body_of[k];
        parent_k[k] = m.body_parent[b] > 0 ? k_of[m.body_parent[b]] : -1;
        fill_body_record(m, b, &bd[16 * (size_t)k]);
        int32_t *r = &bi[8 * (size_t)k];
        r[0] = m.body_jntnum[b];
        r[1] = (int)j_type.size();
        r[4] = -1;
        for (int j = m.body_jntadr[b]; j < m.body_jntadr[b] + m.body_jntnum[b]; j++) {
            const int t = m.jnt_type[j];
            if (t == J_BALL) return fail(MOPA_ERR_UNSUPPORTED, "ball joints are not supported");
            if (t == J_FREE && m.body_jntnum[b] != 1) return fail(MOPA_ERR_UNSUPPORTED, "free joint combined with other joints");
            if (j == m.body_jntadr[b]) {
                r[4] = t;
                r[5] = m.jnt_qposadr[j];
            }
            j_type.push_back(t);
            j_qadr.push_back(m.jnt_qposadr[j]);
            j_axis.insert(j_axis.end(), m.jnt_axis + 3 * j, m.jnt_axis + 3 * j + 3);
            j_pos.insert(j_pos.end(), m.jnt_pos + 3 * j, m.jnt_pos + 3 * j + 3);
            j_ref.push_back(t == J_FREE ? 0.0 : m.jnt_ref[j]);
        }
    }
    const int n_save = save_slot_program(parent_k.data(), nb, bi.data() + 2, bi.data() + 3, 8);      // (EnvBodyI.load, .save)
    if (((size_t)n_save * 7 + (size_t)n_touch * 12) * 64 * sizeof(double) > 62 * 1024)
        return fail(MOPA_ERR_LIMIT, "kinematic tree too branchy for the LDS save slots");

    // pack the blobs
    EnvHdr &h = S.hdr;
    h.kind = kind;
    h.nq = m.nq; h.n_arm = desc->n_arm; h.n_grip = desc->n_grip; h.n_act = desc->n_act; h.nb = nb; h.n_save = n_save;
    h.n_frames = nf; h.n_touch = n_touch; h.n_touch_left = desc->n_touch_left;
    h.adim = desc->n_arm + (kind == MOPA_ENV_LIFT ? 1 : 0);
    h.obs_dim = kind == MOPA_ENV_PUSHER ? 3 * desc->n_arm + 8
                                        : 2 * desc->n_arm + 2 * desc->n_grip + 7 + (kind == MOPA_ENV_PUSH ? 15 : (kind == MOPA_ENV_LIFT ? 10 : 13));
    for (int f = 0; f < kEnvMaxFrames; f++) h.frame_k[f] = f < nf ? k_of[desc->frame_body[f]] : -1;
    for (int f = 0; f < 2; f++) h.quat_k[f] = k_of[desc->quat_body[f]];
    for (int g = 0; g < kEnvMaxTouch; g++) h.touch_k[g] = g < n_touch ? k_of[m.geom_body[desc->touch_geom[g]]] : -1;
    h.o_bi = B.add_i(bi);
    h.o_bd = B.add_d(bd);
    h.o_j_type = B.add_i(j_type);
    h.o_j_qadr = B.add_i(j_qadr);
    h.o_j_axis = B.add_d(j_axis);
    h.o_j_pos = B.add_d(j_pos);
    h.o_j_ref = B.add_d(j_ref);
    h.o_arm = B.add_i(desc->arm_qpos_idx, desc->n_arm);
    h.o_grip = B.add_i(desc->grip_qpos_idx, desc->n_grip);
    h.o_act = B.add_i(desc->act_qpos_idx, desc->n_act);
    h.o_act_lo = B.add_d(desc->act_ctrl_lo, desc->n_act);
    h.o_act_hi = B.add_d(desc->act_ctrl_hi, desc->n_act);
    h.o_lim = B.add_i(desc->qpos_limited, m.nq);
    h.o_lo = B.add_d(desc->qpos_min, m.nq);
    h.o_hi = B.add_d(desc->qpos_max, m.nq);
    h.o_off = B.add_d(desc->frame_off, 3 * (size_t)nf);
    h.o_tg = (int)B.D.size();
    if (n_touch > 0) {
        // touch geom records: local pos[3] quat[4] size[3] type rbound; the mesh's size slots = (vertex offset in this blob, count)
        const int cg0 = desc->touch_geom[0], mid = m.geom_dataid[cg0];
        const double *V = m.mesh_vert + 3 * (size_t)m.mesh_vertadr[mid];
        const int nv = m.mesh_vertnum[mid];
        std::vector<double> tg((size_t)kTgStride * n_touch, 0.0);
        const int o_verts = (int)B.D.size() + (int)tg.size();
        for (int g = 0; g < n_touch; g++) {
            const int cg = desc->touch_geom[g];
            double *r = &tg[(size_t)kTgStride * g];
            std::memcpy(r, m.geom_pos + 3 * cg, 24);
            std::memcpy(r + 3, m.geom_quat + 4 * cg, 32);
            r[10] = (double)m.geom_type[cg];
            if (g == 0) {
                r[7] = (double)o_verts; r[8] = (double)nv; r[9] = 0.0;
                double r2 = 0.0;
                for (int i = 0; i < nv; i++) r2 = std::max(r2, fma(V[3 * i + 2], V[3 * i + 2], fma(V[3 * i + 1], V[3 * i + 1], V[3 * i] * V[3 * i])));
                r[11] = sqrt(r2);
            } else {
                std::memcpy(r + 7, m.geom_size + 3 * cg, 24);
                r[11] = rbound_of(G_BOX, m.geom_size + 3 * cg);
            }
        }
        B.add_d(tg);
        if ((int)B.D.size() != o_verts) return fail(MOPA_ERR_INVALID_ARG, "internal: touch table misaligned");
        B.add_d(V, 3 * (size_t)nv);
    }
    h.max_episode_steps = desc->max_episode_steps;
    h.ac_scale = desc->ac_scale; h.distance_threshold = desc->distance_threshold; h.success_reward = desc->success_reward;
    S.h_int = B.I;
    return MOPA_OK;
}

extern "C" int mopa_env_create(const MopaEnvDesc *desc, MopaEnv **out) {
    if (!desc || !out) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    auto S = std::make_unique<MopaEnv>();
    BlobPacker B;
    if (const int rc = env_build_host(desc, *S, B)) return rc;
    if (const int rc = pick_device(desc->device, &S->device, "no HIP device available (this library has no CPU fallback)")) return rc;
    DeviceGuard guard(S->device);
    if (!guard.ok()) return fail(MOPA_ERR_HIP, "hipSetDevice failed");
    if (upload_tables(B.D, B.I, &S->d_dbl, &S->d_int) != hipSuccess) return fail(MOPA_ERR_HIP, "device allocation / upload of the env tables failed");
    *out = S.release();
    return MOPA_OK;
}

// The host half alone: status, and for an accepted description the fingerprint of what mopa_env_create would upload (header, double
// table, int table) with the walk's body and save-slot counts.
static_assert(sizeof(EnvHdr) == offsetof(EnvHdr, ac_scale) + 3 * sizeof(double) && offsetof(EnvHdr, ac_scale) == offsetof(EnvHdr, max_episode_steps) + sizeof(int),
              "EnvHdr has padding: mopa_env_tables_host would hash indeterminate bytes");
extern "C" int mopa_env_tables_host(const MopaEnvDesc *desc, uint64_t *fingerprint, int32_t *nb, int32_t *n_save) {
    MopaEnv S;
    BlobPacker B;
    if (const int rc = env_build_host(desc, S, B)) return rc;
    Fnv f;
    f.add(&S.hdr, sizeof(EnvHdr));
    f.add(B.D);
    f.add(B.I);
    if (fingerprint) *fingerprint = f.f;
    if (nb) *nb = S.hdr.nb;
    if (n_save) *n_save = S.hdr.n_save;
    return MOPA_OK;
}

extern "C" void mopa_env_destroy(MopaEnv *env) { delete env; }
extern "C" int mopa_env_obs_dim(const MopaEnv *env) { return env ? env->hdr.obs_dim : -1; }
extern "C" int mopa_env_action_dim(const MopaEnv *env) { return env ? env->hdr.adim : -1; }

// LDS of the step kernels: the DFS save slots, then (Lift) the posed frames of the touch geoms
static size_t env_lds_bytes(const EnvHdr &h) { return ((size_t)std::max(h.n_save, 1) * 7 + (size_t)h.n_touch * 12) * 64 * sizeof(double); }

// qvel_dev != nullptr: the reward / obs / bookkeeping half of a step whose physics k_env_dyn already ran
static int env_step_launch(MopaEnv *env, int64_t E, double *qpos_dev, double *prev_state_dev, uint8_t *has_prev_dev, int32_t *ep_len_dev,
                           const double *action_dev, int is_planner, const uint8_t *move_mask_dev, double *obs_dev, double *reward_dev,
                           uint8_t *done_dev, uint8_t *success_dev, const double *qvel_dev, hipStream_t st) {
    const unsigned blocks = (unsigned)((E + 63) / 64);
    const size_t lds = env_lds_bytes(env->hdr);
    DynObs dob{};
    if (qvel_dev) {
        dob.nd = env->dyn.nd;
        dob.nv = env->dyn.nv;
        for (int j = 0; j < 8; j++) dob.arm_dof[j] = env->dyn.arm_dof[j];
        for (int j = 0; j < 4; j++) dob.grip_dof[j] = env->dyn.grip_dof[j];
    }
    auto kern = env->hdr.kind == MOPA_ENV_PUSH ? k_env_step<0> : (env->hdr.kind == MOPA_ENV_LIFT ? k_env_step<1> : (env->hdr.kind == MOPA_ENV_PUSHER ? k_env_step<3> : k_env_step<2>));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, st, env->hdr, env->d_dbl, env->d_int, (long long)E,
                       qpos_dev, prev_state_dev, has_prev_dev, ep_len_dev, action_dev, is_planner, move_mask_dev, obs_dev,
                       reward_dev, done_dev, success_dev, qvel_dev, dob);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_env_step_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *prev_state_dev, uint8_t *has_prev_dev,
                                   int32_t *ep_len_dev, const double *action_dev, int32_t is_planner, const uint8_t *move_mask_dev,
                                   double *obs_dev, double *reward_dev, uint8_t *done_dev, uint8_t *success_dev, void *stream) {
    if (!env) return fail(MOPA_ERR_INVALID_ARG, "null env");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !obs_dev) return fail(MOPA_ERR_INVALID_ARG, "null qpos / obs buffer");
    if (action_dev && (!prev_state_dev || !has_prev_dev || !ep_len_dev || !reward_dev || !done_dev || !success_dev))
        return fail(MOPA_ERR_INVALID_ARG, "a stepping call needs prev_state, has_prev, ep_len, reward, done and success buffers");
    ON_DEVICE(env->device);
    return env_step_launch(env, E, qpos_dev, prev_state_dev, has_prev_dev, ep_len_dev, action_dev, (int)is_planner, move_mask_dev, obs_dev,
                           reward_dev, done_dev, success_dev, nullptr, (hipStream_t)stream);
}

extern "C" int mopa_env_exec_batch(MopaEnv *env, int64_t E, double *qpos_dev, double *prev_state_dev, uint8_t *has_prev_dev,
                                   int32_t *ep_len_dev, const double *traj_dev, const int64_t *path_len_dev, int32_t L,
                                   const double *disc_pow_dev, const double *last_extra_dev, double *obs_dev, double *reward_dev,
                                   uint8_t *done_dev, uint8_t *success_dev, double *smdp_rew_dev, uint8_t *smdp_done_dev,
                                   int64_t *intra_dev, double *rec_ob_dev, double *rec_rew_dev, uint8_t *rec_done_dev,
                                   int64_t *n_exec_dev, void *stream) {
    if (!env) return fail(MOPA_ERR_INVALID_ARG, "null env");
    if (E < 0 || L < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E / L");
    if (E == 0 || L == 0) return MOPA_OK;
    if (!qpos_dev || !prev_state_dev || !has_prev_dev || !ep_len_dev || !traj_dev || !path_len_dev || !disc_pow_dev || !obs_dev ||
        !reward_dev || !done_dev || !success_dev || !smdp_rew_dev || !smdp_done_dev || !intra_dev)
        return fail(MOPA_ERR_INVALID_ARG, "null argument");
    if (env->hdr.adim > env->hdr.n_arm && !last_extra_dev) return fail(MOPA_ERR_INVALID_ARG, "this env kind needs last_extra (the last waypoint's gripper action)");
    if (rec_ob_dev && (!rec_rew_dev || !rec_done_dev || !n_exec_dev)) return fail(MOPA_ERR_INVALID_ARG, "incomplete record buffers");
    ON_DEVICE(env->device);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((E + 63) / 64);
    const size_t lds = env_lds_bytes(env->hdr);
    const EnvHdr &h = env->hdr;
    // slots for every (env, waypoint): the parallel form; MOPA_ENV_EXEC=walk|slots pins the form for A/B runs and tests
    const size_t n_slots = (size_t)E * (size_t)L;
    const size_t per_slot = (size_t)(h.nq + h.n_arm + 1 + (rec_ob_dev ? 0 : h.obs_dim)) * sizeof(double) + sizeof(int) + 3;
    const char *force = getenv("MOPA_ENV_EXEC");
    const bool slots = h.nq <= 64 && (force ? std::strcmp(force, "slots") == 0 : (L >= 3 && n_slots * per_slot <= ((size_t)3 << 29)));
    if (slots) {
        DevBuf *buf;
        {
            std::lock_guard<std::mutex> lock(env->mu);
            buf = &env->exec_scratch[st];
        }
        const size_t bytes = n_slots * per_slot + 64;
        if (bytes > buf->cap) {
            void *np = nullptr;
            const size_t want = std::max(bytes, buf->cap + buf->cap / 2);
            HIP_TRY(hipMalloc(&np, want));
            if (buf->p) {
                std::lock_guard<std::mutex> lock(env->mu);
                env->retired.push_back(buf->p);
            }
            buf->p = np;
            buf->cap = want;
        }
        ExecSlots v;
        double *d = buf->as<double>();
        v.q = d; d += n_slots * h.nq;
        v.prev = d; d += n_slots * h.n_arm;
        v.rew = d; d += n_slots;
        if (rec_ob_dev) v.obs = rec_ob_dev;      // the per-waypoint record has the slots' layout: written in place
        else { v.obs = d; d += n_slots * h.obs_dim; }
        v.ep = reinterpret_cast<int *>(d);
        v.has = reinterpret_cast<unsigned char *>(v.ep + n_slots);
        v.done = v.has + n_slots;
        v.succ = v.done + n_slots;
        const unsigned sblocks = (unsigned)((n_slots + 63) / 64);
        const int kind = h.kind;
#define MOPA_EXEC_LAUNCH(K)                                                                                                      \
        hipLaunchKernelGGL(k_env_exec_pre<K>, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, st, h, env->d_dbl, env->d_int, (long long)E, qpos_dev,  \
                           prev_state_dev, has_prev_dev, ep_len_dev, traj_dev, (const long long *)path_len_dev, (int)L, v);     \
        hipLaunchKernelGGL(k_env_exec_step<K>, dim3(sblocks), dim3(64), lds, st, h, env->d_dbl, env->d_int, (long long)E,       \
                           traj_dev, (const long long *)path_len_dev, (int)L, last_extra_dev, v);
        if (kind == MOPA_ENV_PUSH) { MOPA_EXEC_LAUNCH(0) } else if (kind == MOPA_ENV_LIFT) { MOPA_EXEC_LAUNCH(1) } else if (kind == MOPA_ENV_PUSHER) { MOPA_EXEC_LAUNCH(3) } else { MOPA_EXEC_LAUNCH(2) }
#undef MOPA_EXEC_LAUNCH
        hipLaunchKernelGGL(k_env_exec_fold, dim3(blocks), dim3(64), 0, st, h, (long long)E, qpos_dev, prev_state_dev, has_prev_dev,
                           ep_len_dev, (const long long *)path_len_dev, (int)L, disc_pow_dev, obs_dev, reward_dev, done_dev, success_dev,
                           smdp_rew_dev, smdp_done_dev, (long long *)intra_dev, rec_ob_dev ? rec_rew_dev : nullptr, rec_done_dev,
                           (long long *)n_exec_dev, v);
        HIP_TRY(hipGetLastError());
        return MOPA_OK;
    }
    auto kern = env->hdr.kind == MOPA_ENV_PUSH ? k_env_exec<0> : (env->hdr.kind == MOPA_ENV_LIFT ? k_env_exec<1> : (env->hdr.kind == MOPA_ENV_PUSHER ? k_env_exec<3> : k_env_exec<2>));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, st, env->hdr, env->d_dbl, env->d_int, (long long)E,
                       qpos_dev, prev_state_dev, has_prev_dev, ep_len_dev, traj_dev, (const long long *)path_len_dev, (int)L, disc_pow_dev,
                       last_extra_dev, obs_dev, reward_dev, done_dev, success_dev, smdp_rew_dev, smdp_done_dev, (long long *)intra_dev,
                       rec_ob_dev, rec_rew_dev, rec_done_dev, (long long *)n_exec_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}

extern "C" int mopa_env_desired_batch(MopaEnv *env, int64_t E, const double *qpos_dev, const double *prev_state_dev,
                                      const uint8_t *has_prev_dev, const double *action_dev, int32_t is_planner,
                                      double *desired_dev, void *stream) {
    if (!env) return fail(MOPA_ERR_INVALID_ARG, "null env");
    if (E < 0) return fail(MOPA_ERR_INVALID_ARG, "negative E");
    if (E == 0) return MOPA_OK;
    if (!qpos_dev || !prev_state_dev || !has_prev_dev || !action_dev || !desired_dev) return fail(MOPA_ERR_INVALID_ARG, "null argument");
    ON_DEVICE(env->device);
    const long long n = (long long)E * env->hdr.n_arm;
    hipLaunchKernelGGL(k_env_desired, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, env->hdr, env->d_dbl,
                       env->d_int, (long long)E, qpos_dev, prev_state_dev, has_prev_dev, action_dev, (int)is_planner, desired_dev);
    HIP_TRY(hipGetLastError());
    return MOPA_OK;
}
