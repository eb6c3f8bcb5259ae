// mopa_scene_build.inc -- the scene compiler (included by mopa_hip.hip behind the validity kernels): every table the
// kernels read (blobs, header, FP32 pair table) from the description, and the K1 policy of the scene.  Host code only, no
// device needed (mopa_scene_k1_export runs it on its own; tools/bake_k1_scenes.py bakes scenes from it).
//
// The compiler is a sequence of steps over one working struct (SceneBuild); a step reads only what earlier steps wrote and
// returns a status code.  The ORDER of the B.add_d / B.add_i calls and of the alignment pads is the blob layout, which the
// baked kernels' fingerprints hash (k1_fingerprint below).
namespace {

struct Builder {
    std::vector<double> dbl;
    std::vector<int32_t> ints;
    int add_d(const std::vector<double> &v) { int o = (int)dbl.size(); dbl.insert(dbl.end(), v.begin(), v.end()); return o; }
    int add_i(const std::vector<int32_t> &v) { int o = (int)ints.size(); ints.insert(ints.end(), v.begin(), v.end()); return o; }
};

struct PairE { int code, g1, g2, model_idx; };

struct SceneBuild {
    const MopaSceneDesc *desc;
    const MopaModel &m;
    MopaScene *S;
    SceneHdr &h;
    Builder B;
    // glued compile (mopa_scene_create_glued): model body ids, -1 = the ordinary compile.  body glue_b is compiled as a jointless child of
    // glue_a whose local pose comes from the state's free-joint slots (J_GLUE); `par` is the body tree every step walks.
    int glue_a = -1, glue_b = -1;
    std::vector<int> par;
    std::vector<char> in_glue;         // [nbody] 1 = glue_b or below it
    SceneBuild(const MopaSceneDesc *desc_, MopaScene *S_, int glue_a_ = -1, int glue_b_ = -1)
        : desc(desc_), m(desc_->model), S(S_), h(S_->hdr), glue_a(glue_a_), glue_b(glue_b_) {}
    bool glued() const { return glue_b >= 0; }

    // 1.
    double reach = 0.0;
    // 2.
    std::vector<double> act_lo, act_hi, act_ext;
    std::vector<int32_t> act_adr, act_so2;
    std::vector<int> active_slot;
    int na = 0;
    // 3.
    std::vector<char> needed, is_static;
    std::vector<double> xpos, xquat, xmat;
    // 4.
    std::vector<int> mb_of_body, mb_body;
    int nmb = 0, nmj = 0, n_pq = 0, nmg = 0;
    std::vector<double> sf_pos, sf_quat, sf_mat;
    std::vector<double> mb_pos, mb_quat, mj_axis, mj_pos, mj_ref;
    std::vector<int32_t> mb_parent, mb_jntadr, mb_jntnum, mj_type, mj_qsrc, pq_adr;
    std::vector<int32_t> chain_adr, chain_len, chain_items;
    std::vector<double> g_lpos, g_lquat, g_rbound, g_rec;
    std::vector<int32_t> g_type, g_slot, g_mb, mg_geom;
    std::vector<PairE> pairs;
    std::vector<int32_t> pk;
    // 5.
    std::vector<int32_t> mb_load, mb_save, mb_mgadr, mb_mgnum;
    int n_save = 0;
    // 6.
    std::vector<int32_t> mg_store;
    std::vector<int32_t> mg_padr, mg_pnum, gp_word, mg_padr_mesh, mg_pnum_mesh, gp_word_mesh;
    std::vector<int32_t> t5_padr, t5_pnum, t5_word;
    int max_pnum = 0;
    std::vector<int32_t> mbr, mgr, mgr_mesh;
    std::vector<double> mbd, mgd;
    // 9.
    int o_mgr_mesh = 0, o_gp_word_mesh = 0;

    int check_model();
    int split_active();
    int static_frames();
    int moving_bodies();
    int geoms_and_pairs();
    int dfs_program();
    int pair_lists();
    int fp32_table();
    int packed_records();
    int assemble_tables();
    int tile_poses();
    int planner_fk();
    int finish_blobs();
    int k1_policy();
};

// 1. model checks; `reach` bounds every model-determined coordinate
int SceneBuild::check_model() {
    if (m.nq <= 0 || m.nbody <= 0 || m.ngeom < 0) return fail(MOPA_ERR_INVALID_ARG, "empty model");
    if (m.ngeom > 255) return fail(MOPA_ERR_LIMIT, "more than 255 collidable geoms");
    if (m.npair > 65535) return fail(MOPA_ERR_LIMIT, "more than 65535 candidate pairs");
    // The broad phase culls at zero margin: with a threshold > 0 a pair at distance (0, thr] would be reported or not
    // depending on the cull, and MuJoCo's own contact list (dist < margin) would have to be reproduced.  The reference
    // passes negative thresholds (config/sawyer.py:98-100, config/pusher.py:79-81); 0 keeps "any penetration".
    if (desc->contact_threshold > 0.0) return fail(MOPA_ERR_UNSUPPORTED, "contact_threshold > 0 is not supported (the broad phase culls at zero margin)");
    if (const int rc = check_model_structure(m)) return rc;
    for (int p = 0; p < m.npair; p++) {
        const int g1 = m.pair_geom[2 * p], g2 = m.pair_geom[2 * p + 1];
        if (g1 < 0 || g1 >= m.ngeom || g2 < 0 || g2 >= m.ngeom) return fail(MOPA_ERR_INVALID_ARG, "pair_geom out of range");
        if (g1 == g2) return fail(MOPA_ERR_INVALID_ARG, "pair_geom names one geom twice (pair " + std::to_string(p) + ")");
    }
    par.assign(m.body_parent, m.body_parent + m.nbody);
    in_glue.assign(m.nbody, 0);
    if (glued()) {
        // (the reference: GlueTransformation, mujoco_ompl_interface.cpp:810-907; its two-slide branch is not built)
        if (glue_a <= 0 || glue_a >= m.nbody || glue_b <= 0 || glue_b >= m.nbody) return fail(MOPA_ERR_INVALID_ARG, "glue: body id out of range (the world body cannot be glued)");
        if (m.body_jntnum[glue_b] != 1 || m.jnt_type[m.body_jntadr[glue_b]] != J_FREE)
            return fail(MOPA_ERR_UNSUPPORTED, "glue: body_b must carry exactly one free joint (the reference's two-slide branch is not built)");
        bool a_static = true;
        for (int b = glue_a; b > 0; b = m.body_parent[b])
            if (m.body_jntnum[b] > 0) a_static = false;
        if (a_static) return fail(MOPA_ERR_UNSUPPORTED, "glue: body_a is static (no joint moves it)");
        for (int b = glue_a; b > 0; b = m.body_parent[b])
            if (b == glue_b) return fail(MOPA_ERR_UNSUPPORTED, "glue: body_a lies inside body_b's subtree");
        if (glue_a >= glue_b) return fail(MOPA_ERR_UNSUPPORTED, "glue: body_a must come before body_b in body order");
        par[glue_b] = glue_a;
        in_glue[glue_b] = 1;
        for (int b = glue_b + 1; b < m.nbody; b++) in_glue[b] = in_glue[m.body_parent[b]];
    }
    // FP32 broad phase (third-generation kernel): its conservativeness proof assumes coordinates of a few metres (absolute
    // slack 2e-5 m vs the float rounding of a coordinate).  `reach` bounds every model-determined coordinate; larger scenes
    // use the FP64 cull of the second generation.  Free-joint positions come from qpos at run time and are the caller's
    // responsibility (the Sawyer world box is +-1.2 m x 2 m, env/sawyer/sawyer.py:52-53).  So is, in a glued compile, the offset
    // of the carried body from body_a: `reach` counts body_b at the origin of body_a, the attach state decides how far away it is.
    reach = 0.0;
    {
        std::vector<double> rb(m.nbody, 0.0);
        for (int b = 1; b < m.nbody; b++) {
            const double *p = m.body_pos + 3 * b;
            rb[b] = (b == glue_b) ? rb[glue_a] : rb[m.body_parent[b]] + sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            for (int j = m.body_jntadr[b]; j >= 0 && j < m.body_jntadr[b] + m.body_jntnum[b]; j++)
                if (m.jnt_type[j] == J_SLIDE && m.jnt_limited[j]) rb[b] += std::max(fabs(m.jnt_range[2 * j]), fabs(m.jnt_range[2 * j + 1]));
        }
        for (int g = 0; g < m.ngeom; g++) {
            if (m.geom_type[g] == G_PLANE) continue;
            const double *p = m.geom_pos + 3 * g, *z = m.geom_size + 3 * g;
            reach = std::max(reach, rb[m.geom_body[g]] + sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]));
        }
    }

    S->nq = m.nq;
    S->seed = desc->seed;
    S->ngeom_model = m.ngeom;
    S->npair_model = m.npair;
    return MOPA_OK;
}

// 2. active / passive split of the qpos coordinates
int SceneBuild::split_active() {
    // --- active / passive split (KinematicPlanner.cpp:263-269) ---
    std::vector<char> is_passive(m.nq, 0);
    for (int i = 0; i < desc->n_passive; i++) {
        int a = desc->passive_qpos_idx[i];
        if (a < 0 || a >= m.nq) { return fail(MOPA_ERR_INVALID_ARG, "passive_qpos_idx out of range"); }
        is_passive[a] = 1;
    }
    std::vector<int> qpos_jnt(m.nq, -1);
    for (int j = 0; j < m.njnt; j++) {
        int w = (m.jnt_type[j] == J_FREE) ? 7 : (m.jnt_type[j] == J_BALL ? 4 : 1);
        for (int k = 0; k < w; k++)
            if (m.jnt_qposadr[j] + k < m.nq) qpos_jnt[m.jnt_qposadr[j] + k] = j;
    }
    active_slot.assign(m.nq, -1);
    for (int i = 0; i < m.nq; i++) {
        if (is_passive[i]) continue;
        int j = qpos_jnt[i];
        if (j < 0) { return fail(MOPA_ERR_INVALID_ARG, "active qpos address without a joint"); }
        if (m.jnt_type[j] == J_FREE || m.jnt_type[j] == J_BALL) {
            return fail(MOPA_ERR_UNSUPPORTED, "free/ball joints cannot be planned over (only hinge/slide are active in the reference scenes)");
        }
        active_slot[i] = (int)act_adr.size();
        act_adr.push_back(i);
        // limited hinge / slide -> R^1 with the joint range; unlimited hinge -> OMPL SO2StateSpace
        // (mujoco_ompl_interface.cpp:227-249): samples in [-pi, pi], maximum extent pi, wrap-around metric
        double lo = m.jnt_range[2 * j], hi = m.jnt_range[2 * j + 1];
        bool so2 = (m.jnt_type[j] == J_HINGE) && !m.jnt_limited[j];
        if (so2) { lo = -kPi; hi = kPi; }
        act_lo.push_back(lo);
        act_hi.push_back(hi);
        act_ext.push_back(so2 ? kPi : hi - lo);
        act_so2.push_back(so2 ? 1 : 0);
    }
    na = (int)act_adr.size();
    S->na = na;
    S->active_idx.assign(act_adr.begin(), act_adr.end());
    return MOPA_OK;
}

// 3. which bodies matter, which are static, and the static world frames
int SceneBuild::static_frames() {
    // --- which bodies matter, which are static ---
    for (int g = 0; g < m.ngeom; g++) {
        int t = m.geom_type[g];
        if (t == G_MESH) {
            const int id = (m.nmesh > 0 && m.geom_dataid) ? m.geom_dataid[g] : -1;
            if (id < 0 || id >= m.nmesh || !m.mesh_vert || m.mesh_vertnum[id] <= 0 ||
                m.mesh_vertadr[id] < 0 || m.mesh_vertadr[id] + m.mesh_vertnum[id] > m.nmeshvert) {
                return fail(MOPA_ERR_INVALID_ARG, "mesh geom " + std::to_string(g) + " without a convex hull (MopaModel.geom_dataid / mesh_vert)");
            }
        } else if (!(t == G_PLANE || t == G_SPHERE || t == G_CAPSULE || t == G_CYLINDER || t == G_BOX)) {
            return fail(MOPA_ERR_UNSUPPORTED, "collidable geom type " + std::to_string(t) + " (ellipsoid/hfield) is not supported");
        }
    }
    needed.assign(m.nbody, 0);
    is_static.assign(m.nbody, 0);
    for (int g = 0; g < m.ngeom; g++) {
        int b = m.geom_body[g];
        while (b > 0 && !needed[b]) { needed[b] = 1; b = par[b]; }
    }
    needed[0] = 1;
    is_static[0] = 1;
    for (int b = 1; b < m.nbody; b++) is_static[b] = (m.body_jntnum[b] == 0) && is_static[par[b]];

    // static world frames (host FK with the same arithmetic as the device path)
    xpos.assign(3 * m.nbody, 0.0);
    xquat.assign(4 * m.nbody, 0.0);
    xmat.assign(9 * m.nbody, 0.0);
    xquat[0] = 1.0;
    quat2mat(&xmat[0], Q4{1.0, 0.0, 0.0, 0.0});
    for (int b = 1; b < m.nbody; b++) {
        if (!needed[b] || !is_static[b]) continue;
        int pid = m.body_parent[b];
        V3 v = mat_vec(&xmat[9 * pid], ld3(m.body_pos + 3 * b));
        V3 p = add3(ld3(&xpos[3 * pid]), v);
        const double *pq = &xquat[4 * pid], *bq = m.body_quat + 4 * b;
        Q4 q = quat_normalize(quat_mul(Q4{pq[0], pq[1], pq[2], pq[3]}, Q4{bq[0], bq[1], bq[2], bq[3]}));
        st3(&xpos[3 * b], p);
        xquat[4 * b] = q.w; xquat[4 * b + 1] = q.x; xquat[4 * b + 2] = q.y; xquat[4 * b + 3] = q.z;
        quat2mat(&xmat[9 * b], q);
    }
    return MOPA_OK;
}

// 4. moving bodies and their joints, static parent frames, ancestor chains
int SceneBuild::moving_bodies() {
    // moving bodies in id (topological) order
    std::vector<int> sf_of_body(m.nbody, -1);
    mb_of_body.assign(m.nbody, -1);
    for (int b = 1; b < m.nbody; b++)
        if (needed[b] && !is_static[b]) { mb_of_body[b] = (int)mb_body.size(); mb_body.push_back(b); }
    nmb = (int)mb_body.size();
    auto sf_index = [&](int b) {
        if (sf_of_body[b] < 0) {
            sf_of_body[b] = (int)sf_pos.size() / 3;
            sf_pos.insert(sf_pos.end(), &xpos[3 * b], &xpos[3 * b] + 3);
            sf_quat.insert(sf_quat.end(), &xquat[4 * b], &xquat[4 * b] + 4);
            sf_mat.insert(sf_mat.end(), &xmat[9 * b], &xmat[9 * b] + 9);
        }
        return sf_of_body[b];
    };
    sf_index(0);

    std::vector<int> pq_slot(m.nq, -1);
    auto passive_slot = [&](int adr) {
        if (pq_slot[adr] < 0) { pq_slot[adr] = (int)pq_adr.size(); pq_adr.push_back(adr); }
        return na + pq_slot[adr];
    };
    for (int k = 0; k < nmb; k++) {
        int b = mb_body[k];
        int pid = par[b];
        mb_parent.push_back(mb_of_body[pid] >= 0 ? mb_of_body[pid] : -(sf_index(pid) + 1));
        mb_pos.insert(mb_pos.end(), m.body_pos + 3 * b, m.body_pos + 3 * b + 3);
        mb_quat.insert(mb_quat.end(), m.body_quat + 4 * b, m.body_quat + 4 * b + 4);
        mb_jntadr.push_back((int)mj_type.size());
        mb_jntnum.push_back(m.body_jntnum[b]);
        if (b == glue_b) {
            // the carried body: one J_GLUE "joint" whose value slots are the free joint's 7 passive slots, read as the body's local pose
            // (pos[3] quat[4]) under body_a; the joint itself applies nothing (apply_joint knows slide and hinge only)
            const int adr = m.jnt_qposadr[m.body_jntadr[b]];
            mj_type.push_back(J_GLUE);
            mj_axis.insert(mj_axis.end(), 3, 0.0);
            mj_pos.insert(mj_pos.end(), 3, 0.0);
            mj_ref.push_back(0.0);
            const int first = passive_slot(adr);
            for (int c = 1; c < 7; c++)
                if (passive_slot(adr + c) != first + c) { return fail(MOPA_ERR_UNSUPPORTED, "free joint qpos not contiguous in the passive list"); }
            mj_qsrc.push_back(first);
            continue;
        }
        for (int j = m.body_jntadr[b]; j < m.body_jntadr[b] + m.body_jntnum[b]; j++) {
            int t = m.jnt_type[j];
            if (t == J_BALL) { return fail(MOPA_ERR_UNSUPPORTED, "ball joints are not supported (the reference throws as well: mujoco_ompl_interface.cpp:217-229)"); }
            if (t == J_FREE && m.body_jntnum[b] != 1) { return fail(MOPA_ERR_UNSUPPORTED, "free joint combined with other joints"); }
            mj_type.push_back(t);
            mj_axis.insert(mj_axis.end(), m.jnt_axis + 3 * j, m.jnt_axis + 3 * j + 3);
            mj_pos.insert(mj_pos.end(), m.jnt_pos + 3 * j, m.jnt_pos + 3 * j + 3);
            mj_ref.push_back(t == J_FREE ? 0.0 : m.jnt_ref[j]);
            int adr = m.jnt_qposadr[j];
            if (t == J_FREE) {
                int first = passive_slot(adr);
                for (int c = 1; c < 7; c++) {
                    int sl = passive_slot(adr + c);
                    if (sl != first + c) { return fail(MOPA_ERR_UNSUPPORTED, "free joint qpos not contiguous in the passive list"); }
                }
                mj_qsrc.push_back(first);
            } else {
                mj_qsrc.push_back(active_slot[adr] >= 0 ? active_slot[adr] : passive_slot(adr));
            }
        }
    }
    nmj = (int)mj_type.size();
    n_pq = (int)pq_adr.size();

    // ancestor chains (root-most moving ancestor first)
    chain_adr.assign(nmb, 0);
    chain_len.assign(nmb, 0);
    for (int k = 0; k < nmb; k++) {
        std::vector<int> path;
        for (int c = k; c >= 0; c = mb_parent[c]) path.push_back(c);
        std::reverse(path.begin(), path.end());
        chain_adr[k] = (int)chain_items.size();
        chain_len[k] = (int)path.size();
        chain_items.insert(chain_items.end(), path.begin(), path.end());
    }
    return MOPA_OK;
}

// 4. (continued) geoms, the candidate pair list, pair_slot / pair_model
int SceneBuild::geoms_and_pairs() {
    // geoms
    g_lpos.assign(3 * m.ngeom, 0.0);
    g_lquat.assign(4 * m.ngeom, 0.0);
    g_rbound.assign(m.ngeom, 0.0);
    g_rec.assign((size_t)kGeomStride * m.ngeom, 0.0);
    g_type.assign(m.ngeom, 0);
    g_slot.assign(m.ngeom, -1);
    g_mb.assign(m.ngeom, -1);
    for (int g = 0; g < m.ngeom; g++) {
        int b = m.geom_body[g];
        g_type[g] = m.geom_type[g];
        g_rbound[g] = rbound_of(m.geom_type[g], m.geom_size + 3 * g);
        if (m.geom_type[g] == G_MESH) {   // bounding radius about the geom origin: max |v| over the hull
            const double *V = m.mesh_vert + 3 * (size_t)m.mesh_vertadr[m.geom_dataid[g]];
            double r2 = 0.0;
            for (int i = 0; i < m.mesh_vertnum[m.geom_dataid[g]]; i++) r2 = dmax(r2, dot3(ld3(V + 3 * i), ld3(V + 3 * i)));
            g_rbound[g] = sqrt(r2);
        }
        std::memcpy(&g_lpos[3 * g], m.geom_pos + 3 * g, 24);
        std::memcpy(&g_lquat[4 * g], m.geom_quat + 4 * g, 32);
        double *rec = &g_rec[(size_t)kGeomStride * g];
        std::memcpy(rec + GO_SIZE, m.geom_size + 3 * g, 24);
        if (is_static[b]) {
            V3 gp = add3(ld3(&xpos[3 * b]), mat_vec(&xmat[9 * b], ld3(m.geom_pos + 3 * g)));
            const double *bq = &xquat[4 * b], *lq = m.geom_quat + 4 * g;
            Q4 gq = quat_mul(Q4{bq[0], bq[1], bq[2], bq[3]}, Q4{lq[0], lq[1], lq[2], lq[3]});
            st3(rec + GO_POS, gp);
            quat2mat(rec + GO_MAT, gq);
        } else {
            g_mb[g] = mb_of_body[b];
            g_slot[g] = (int)mg_geom.size();
            mg_geom.push_back(g);
        }
    }
    nmg = (int)mg_geom.size();
    if (nmg > 64) { return fail(MOPA_ERR_LIMIT, "more than 64 moving collidable geoms"); }

    // pairs: drop ignored (mujoco_ompl_interface.cpp:950-960), sort by narrow-phase cost class
    for (int p = 0; p < m.npair; p++) {
        int g1 = m.pair_geom[2 * p], g2 = m.pair_geom[2 * p + 1];
        // (in range and distinct: check_model)  Every pair list belongs to a moving geom, the later of the two: a pair of two static
        // geoms has no owner -- and no state changes its distance, so it is no candidate of MuJoCo's either
        if (g_slot[g1] < 0 && g_slot[g2] < 0) { return fail(MOPA_ERR_INVALID_ARG, "candidate pair of two static geoms (pair " + std::to_string(p) + ")"); }
        int a = m.geom_mjid[g1], b = m.geom_mjid[g2];
        int lo = std::min(a, b), hi = std::max(a, b);
        bool ignored = false;
        for (int i = 0; i < desc->n_ignored; i++)
            if (desc->ignored_pairs[2 * i] == lo && desc->ignored_pairs[2 * i + 1] == hi) ignored = true;
        if (ignored) continue;
        int code = pair_code(m.geom_type[g1], m.geom_type[g2]);
        if (code < 0) { return fail(MOPA_ERR_UNSUPPORTED, "unsupported geom type pair (must be ordered type1<=type2)"); }
        pairs.push_back(PairE{code, g1, g2, p});
    }
    std::stable_sort(pairs.begin(), pairs.end(), [](const PairE &a, const PairE &b) { return a.code < b.code; });
    pk.assign(pairs.size(), 0);
    S->pair_slot.assign(m.npair, -1);
    S->pair_model.assign(pairs.size(), 0);
    S->pruned = desc->pair_cull_radius != nullptr;
    for (size_t i = 0; i < pairs.size(); i++) {
        pk[i] = pairs[i].g1 | (pairs[i].g2 << 8) | (pairs[i].code << 16);
        S->pair_slot[pairs[i].model_idx] = (int)i;
        S->pair_model[i] = pairs[i].model_idx;
    }
    return MOPA_OK;
}

// 5. second-generation kernel: DFS program over the moving bodies, save slots
int SceneBuild::dfs_program() {
    // --- second-generation kernel: DFS program over the moving bodies + per-geom pair lists ---
    mb_load.resize(nmb);
    mb_save.resize(nmb);
    mb_mgadr.assign(nmb, 0);
    mb_mgnum.assign(nmb, 0);
    n_save = save_slot_program(mb_parent.data(), nmb, mb_load.data(), mb_save.data());
    if (glued() && mb_save[mb_of_body[glue_a]] >= 0) {
        // The save slots are numbered by depth, which is right for a tree in depth-first body order.  The carried body comes long after
        // body_a's own subtree, and whatever was parked at body_a's depth in between has overwritten its slot: body_a gets a slot of its own.
        const int ka = mb_of_body[glue_a];
        mb_save[ka] = n_save++;
        for (int k = 0; k < nmb; k++)
            if (mb_parent[k] == ka && mb_load[k] >= 0) mb_load[k] = mb_save[ka];
    }
    // moving geoms are in geom-id order == body order, so each body's geoms are a contiguous slot range
    for (int mslot = 0; mslot < nmg; mslot++) {
        int k = g_mb[mg_geom[mslot]];
        if (mb_mgnum[k] == 0) mb_mgadr[k] = mslot;
        else if (mb_mgadr[k] + mb_mgnum[k] != mslot) { return fail(MOPA_ERR_UNSUPPORTED, "moving geoms of a body are not contiguous"); }
        mb_mgnum[k]++;
    }
    for (int k = 1; k < nmb; k++)   // slots must follow body order for the "earlier partner" rule
        if (mb_mgnum[k] && mb_mgnum[k - 1] && mb_mgadr[k] < mb_mgadr[k - 1]) { return fail(MOPA_ERR_UNSUPPORTED, "geom order does not follow body order"); }
    return MOPA_OK;
}

// 6. per-owner-geom pair lists: main, mesh, and both for the FP32 table
int SceneBuild::pair_lists() {
    // Per-owner-geom pair lists for the lane-per-state kernels.  Pairs whose class involves a mesh are kept in a list
    // of their own: the main pass (k_is_valid_v5 / v2) then carries no mesh code at all, and a second, light pass of
    // the MESH instantiation handles the handful of mesh pairs and folds its verdict into the first one's.
    mg_store.assign(nmg, 0);
    auto build_lists = [&](int mode /*0 = mesh-free pairs, 1 = mesh pairs, 2 = all*/, std::vector<int32_t> &padr, std::vector<int32_t> &pnum, std::vector<int32_t> &words) {
        padr.assign(nmg, 0); pnum.assign(nmg, 0); words.clear();
        std::vector<std::vector<PairE>> own(nmg);
        for (const PairE &e : pairs) {   // already sorted by cost class
            const bool is_mesh = (e.code == PC_PLANE_MESH || e.code == PC_CONVEX_MESH);
            if (mode != 2 && is_mesh != (mode == 1)) continue;
            int s1 = g_slot[e.g1], s2 = g_slot[e.g2];
            int owner = (s2 > s1) ? s2 : s1;
            own[owner].push_back(e);
        }
        for (int mslot = 0; mslot < nmg; mslot++) {
            padr[mslot] = (int)words.size();
            pnum[mslot] = (int)own[mslot].size();
            for (const PairE &e : own[mslot]) {
                int cur = mg_geom[mslot];
                int cur_is_g2 = (e.g2 == cur) ? 1 : 0;
                int partner = cur_is_g2 ? e.g1 : e.g2;
                int pslot = g_slot[partner];
                if (pslot >= 0) mg_store[pslot] = 1;
                words.push_back(partner | (e.code << 8) | (cur_is_g2 << 12) | ((pslot >= 0 ? 1 : 0) << 13) | ((pslot >= 0 ? pslot : 0) << 14));
            }
        }
    };
    build_lists(0, mg_padr, mg_pnum, gp_word);
    build_lists(1, mg_padr_mesh, mg_pnum_mesh, gp_word_mesh);
    // The third-generation kernel culls the mesh pairs too (FP32, a few table entries more) -- not to evaluate them, but
    // to tell the second pass which states have one within reach at all: almost none do, and that pass then skips
    // whole tiles instead of posing every state again for nothing.
    t5_padr = mg_padr; t5_pnum = mg_pnum; t5_word = gp_word;
    if (!gp_word_mesh.empty()) build_lists(2, t5_padr, t5_pnum, t5_word);
    return MOPA_OK;
}

// 6. (continued) the FP32 broad-phase table
int SceneBuild::fp32_table() {
    // v5: FP32 broad-phase table, one 32-byte entry per (owner geom, partner) pair:
    //   [0..2] partner centre (static partners) / a point of the plane,
    //   [3] (owner radius + eps + partner radius)^2 / for a plane: owner radius + eps,
    //   [4..6] world-AABB half extents of a static partner + owner radius + eps / the plane normal,
    //   [7] flags: bits 0..13 = low bits of gp_word (partner gid, code, cur_is_g2, pmov), 14..21 partner slot, 30 plane
    // Within a geom's range the entries are ordered [moving partners | static non-plane partners | planes] (the kernel
    // runs one branch-free loop per group); the group sizes follow the table: tab[8 n_gp + slot] = nmov | nstat<<8 | nplane<<16.
    const size_t n5 = t5_word.size();
    std::vector<int32_t> gp_tab(8 * n5 + 3 * (size_t)nmg, 0);   // entries, then per geom: group counts, then (first entry, count)
    max_pnum = 0;
    {
        auto f2i = [](double x) { float f = (float)x; int32_t i; std::memcpy(&i, &f, 4); return i; };
        for (int mslot = 0; mslot < nmg; mslot++) {
            max_pnum = std::max(max_pnum, (int)t5_pnum[mslot]);
            gp_tab[8 * n5 + nmg + 2 * mslot] = t5_padr[mslot];
            gp_tab[8 * n5 + nmg + 2 * mslot + 1] = t5_pnum[mslot];
            std::vector<int> order[3];
            for (int p = t5_padr[mslot]; p < t5_padr[mslot] + t5_pnum[mslot]; p++) {
                const int w = t5_word[p];
                const int grp = ((w >> 13) & 1) ? 0 : (m.geom_type[w & 0xff] == G_PLANE ? 2 : 1);
                order[grp].push_back(p);
            }
            gp_tab[8 * n5 + mslot] = (int)order[0].size() | ((int)order[1].size() << 8) | ((int)order[2].size() << 16);
            if (getenv("MOPA_DEBUG"))
                fprintf(stderr, "[mopa]   geom slot %d: %zu moving + %zu static + %zu plane partners\n", mslot, order[0].size(), order[1].size(), order[2].size());
            size_t dst = (size_t)t5_padr[mslot];
            for (int grp = 0; grp < 3; grp++)
                for (int p : order[grp]) {
                    const int w = t5_word[p];
                    const int pg = w & 0xff, pmov = (w >> 13) & 1;
                    int32_t *te = &gp_tab[8 * dst++];
                    // the owner's inflated radius is folded into the entry (an entry belongs to one owner geom): FP32
                    // arithmetic here = what the kernel would do per pair and state
                    const float rg = (float)g_rbound[mg_geom[mslot]] + kCullEps;
                    auto ff2i = [](float f) { int32_t i; std::memcpy(&i, &f, 4); return i; };
                    float rs = rg + (float)g_rbound[pg];
                    // (a glued compile: the proofs were made with the carried body where the env row puts it -- not for its pairs)
                    if (desc->pair_cull_radius && !in_glue[m.geom_body[mg_geom[mslot]]] && !in_glue[m.geom_body[pg]]) {
                        // a proven bound on the centre distance at which this pair can reach the threshold at all
                        const int own = mg_geom[mslot];
                        for (int pp = 0; pp < m.npair; pp++) {
                            const int a = m.pair_geom[2 * pp], b = m.pair_geom[2 * pp + 1];
                            if (((a == own && b == pg) || (a == pg && b == own)) && desc->pair_cull_radius[pp] > 0.0)
                                rs = std::min(rs, std::nextafter((float)desc->pair_cull_radius[pp], 1.0e30f) + kCullEps);
                        }
                    }
                    te[3] = ff2i(rs * rs);
                    if (pmov) {
                        // [0] (moving partners only; their centre comes from the tile's table): the square of the centre distance
                        // below which the two geoms' INSCRIBED balls (radius r of a sphere / capsule, min(r, h) of a cylinder,
                        // the smallest half extent of a box, centred where the geom is) overlap by more than the threshold
                        // + 0.1 mm -- then the pair's distance is <= the threshold whatever its class computes (closed forms
                        // are exact, SAT reports the true depth, the portal refinement never less than the true depth - 1e-6):
                        // the verdict-only kernels call such a state invalid in the broad phase and drop all its entries
                        auto r_in = [&](int g) -> double {
                            const double *sz = &g_rec[(size_t)kGeomStride * g + GO_SIZE];
                            switch (m.geom_type[g]) {
                                case G_SPHERE: case G_CAPSULE: return sz[0];
                                case G_CYLINDER: return std::min(sz[0], sz[1]);
                                case G_BOX: return std::min(sz[0], std::min(sz[1], sz[2]));
                                default: return 0.0;
                            }
                        };
                        const double ra = r_in(mg_geom[mslot]), rb = r_in(pg);
                        const double reach = ra + rb - (std::max(0.0, -desc->contact_threshold) + 1e-4) - 4.0 * kCullEps;
                        te[0] = ff2i((ra > 0.0 && rb > 0.0 && reach > 0.0) ? (float)(reach * reach) * (1.0f - 1e-6f) : 0.0f);
                    }
                    int flags = w & 0x3fffff;    // gp_word already carries the slot in bits 14..21
                    if (!pmov) {
                        const double *rec = &g_rec[(size_t)kGeomStride * pg];
                        te[0] = f2i(rec[GO_POS]); te[1] = f2i(rec[GO_POS + 1]); te[2] = f2i(rec[GO_POS + 2]);
                        if (m.geom_type[pg] == G_PLANE) {
                            te[4] = f2i(rec[GO_MAT + 2]); te[5] = f2i(rec[GO_MAT + 5]); te[6] = f2i(rec[GO_MAT + 8]);
                            te[3] = ff2i(rg);
                            flags |= 1 << 30;
                        } else {
                            double H[3];
                            static_aabb_half(m.geom_type[pg], rec, g_rbound[pg], H);
                            te[4] = ff2i((float)H[0] + rg); te[5] = ff2i((float)H[1] + rg); te[6] = ff2i((float)H[2] + rg);
                        }
                    }
                    te[7] = flags;
                }
        }
    }
    S->h_gp_tab = gp_tab;
    return MOPA_OK;
}

// 6. (continued) packed per-body / per-geom records
int SceneBuild::packed_records() {
    mbr.assign(8 * (size_t)nmb, 0);
    mgr.assign(4 * (size_t)nmg, 0);
    mgr_mesh.assign(4 * (size_t)nmg, 0);
    mbd.assign(16 * (size_t)nmb, 0.0);
    mgd.assign(8 * (size_t)nmg, 0.0);
    for (int k = 0; k < nmb; k++) {
        int ja = mb_jntadr[k], jn = mb_jntnum[k];
        int32_t *r = &mbr[8 * (size_t)k];
        r[0] = jn; r[1] = ja; r[2] = mb_load[k]; r[3] = (mb_parent[k] < 0) ? -(mb_parent[k] + 1) : 0;
        r[4] = mb_save[k]; r[5] = mb_mgadr[k]; r[6] = mb_mgnum[k];
        // joint 0: type (7 bits) | bit 7 = anchor at the body origin (mopa_device.hpp: apply_joint) | value slot << 8
        const bool jp_zero = jn > 0 && mj_pos[3 * (size_t)ja] == 0.0 && mj_pos[3 * (size_t)ja + 1] == 0.0 && mj_pos[3 * (size_t)ja + 2] == 0.0;
        r[7] = (jn > 0) ? ((mj_type[ja] & 0x7f) | (jp_zero ? 0x80 : 0) | (mj_qsrc[ja] << 8)) : 0x7f;
        double *d = &mbd[16 * (size_t)k];
        std::memcpy(d, &mb_pos[3 * (size_t)k], 24);
        std::memcpy(d + 3, &mb_quat[4 * (size_t)k], 32);
        if (jn > 0) {
            std::memcpy(d + 7, &mj_axis[3 * (size_t)ja], 24);
            std::memcpy(d + 10, &mj_pos[3 * (size_t)ja], 24);
            d[13] = mj_ref[ja];
        }
    }
    for (int ms = 0; ms < nmg; ms++) {
        int g = mg_geom[ms];
        int32_t *r = &mgr[4 * (size_t)ms];
        r[0] = g; r[1] = mg_store[ms] | ((m.geom_type[g] == G_BOX ? 1 : 0) << 1); r[2] = mg_padr[ms]; r[3] = mg_pnum[ms];
        int32_t *rm = &mgr_mesh[4 * (size_t)ms];
        rm[0] = r[0]; rm[1] = r[1]; rm[2] = mg_padr_mesh[ms]; rm[3] = mg_pnum_mesh[ms];
        double *d = &mgd[8 * (size_t)ms];
        std::memcpy(d, &g_lpos[3 * (size_t)g], 24);
        std::memcpy(d + 3, &g_lquat[4 * (size_t)g], 32);
        d[7] = g_rbound[g];
    }
    return MOPA_OK;
}

// 9. blob assembly, first part (the order of the add_d / add_i calls IS the blob layout)
int SceneBuild::assemble_tables() {
    // --- assemble blobs ---
    h.na = na; h.nq = m.nq; h.n_pq = n_pq; h.nmb = nmb; h.nmj = nmj; h.nsf = (int)sf_pos.size() / 3;
    h.ng = m.ngeom; h.nmg = nmg; h.npair = (int)pairs.size();
    h.o_mb_pos = B.add_d(mb_pos); h.o_mb_quat = B.add_d(mb_quat);
    h.o_sf_pos = B.add_d(sf_pos); h.o_sf_quat = B.add_d(sf_quat); h.o_sf_mat = B.add_d(sf_mat);
    h.o_mj_axis = B.add_d(mj_axis); h.o_mj_pos = B.add_d(mj_pos); h.o_mj_ref = B.add_d(mj_ref);
    h.o_g_lpos = B.add_d(g_lpos); h.o_g_lquat = B.add_d(g_lquat); h.o_g_rbound = B.add_d(g_rbound);
    {
        std::vector<double> g_aabb(3 * (size_t)m.ngeom, 0.0);
        for (int g = 0; g < m.ngeom; g++)
            if (g_slot[g] < 0 && m.geom_type[g] != G_PLANE)
                static_aabb_half(m.geom_type[g], &g_rec[(size_t)kGeomStride * g], g_rbound[g], &g_aabb[3 * (size_t)g]);
        h.o_g_aabb = B.add_d(g_aabb);
    }
    if (B.dbl.size() & 1) B.dbl.push_back(0.0);   // 16-byte align the posed records
    // mesh hulls live in the double blob; a mesh geom's record carries (blob offset of its vertices, vertex count)
    // where primitives carry their size (mopa_device.hpp: mesh_support_local / d_plane_mesh)
    if (m.nmesh > 0) {
        h.has_mesh = 1;
        h.o_mesh = B.add_d(std::vector<double>(m.mesh_vert, m.mesh_vert + 3 * (size_t)m.nmeshvert));
        S->n_mesh_dbl = 3 * (int)m.nmeshvert;
        for (int g = 0; g < m.ngeom; g++)
            if (m.geom_type[g] == G_MESH) {
                double *rec = &g_rec[(size_t)kGeomStride * g];
                rec[GO_SIZE] = (double)(h.o_mesh + 3 * m.mesh_vertadr[m.geom_dataid[g]]);
                rec[GO_SIZE + 1] = (double)m.mesh_vertnum[m.geom_dataid[g]];
                rec[GO_SIZE + 2] = 0.0;
            }
    }
    h.o_g_rec = B.add_d(g_rec);
    h.o_act_lo = B.add_d(act_lo); h.o_act_hi = B.add_d(act_hi); h.o_act_ext = B.add_d(act_ext);
    if (B.dbl.size() & 1) B.dbl.push_back(0.0);
    h.o_mbd = B.add_d(mbd); h.o_mgd = B.add_d(mgd);
    if (B.dbl.size() & 1) B.dbl.push_back(0.0);
    h.o_mb_parent = B.add_i(mb_parent); h.o_mb_jntadr = B.add_i(mb_jntadr); h.o_mb_jntnum = B.add_i(mb_jntnum);
    h.o_mj_type = B.add_i(mj_type); h.o_mj_qsrc = B.add_i(mj_qsrc);
    h.o_g_type = B.add_i(g_type); h.o_g_slot = B.add_i(g_slot); h.o_g_mb = B.add_i(g_mb);
    h.o_mg_geom = B.add_i(mg_geom); h.o_chain_adr = B.add_i(chain_adr); h.o_chain_len = B.add_i(chain_len);
    h.o_chain_items = B.add_i(chain_items); h.o_pairs = B.add_i(pk); h.o_pq_adr = B.add_i(pq_adr);
    h.o_act_adr = B.add_i(act_adr); h.o_act_so2 = B.add_i(act_so2);
    {
        std::vector<double> act_ref(8, 0.0);
        std::vector<int32_t> act_hinge(8, 0);
        for (int j = 0; j < nmj; j++)
            if (mj_qsrc[j] >= 0 && mj_qsrc[j] < na && mj_qsrc[j] < 8) {
                act_ref[mj_qsrc[j]] = mj_ref[j];
                act_hinge[mj_qsrc[j]] = mj_type[j] == J_HINGE;
            }
        h.o_act_ref = B.add_d(act_ref);
        h.o_act_hinge = B.add_i(act_hinge);
    }
    h.n_save = n_save; h.n_gp = (int)t5_word.size();
    h.o_mb_load = B.add_i(mb_load); h.o_mb_save = B.add_i(mb_save); h.o_mb_mgadr = B.add_i(mb_mgadr); h.o_mb_mgnum = B.add_i(mb_mgnum);
    h.o_mg_padr = B.add_i(mg_padr); h.o_mg_pnum = B.add_i(mg_pnum); h.o_mg_store = B.add_i(mg_store); h.o_gp_word = B.add_i(gp_word);
    while (B.ints.size() & 7) B.ints.push_back(0);   // 32-byte align the packed records (scalar dwordx8 loads)
    h.o_mbr = B.add_i(mbr); h.o_mgr = B.add_i(mgr);
    return MOPA_OK;
}

// 7. tile-posed passive bodies (see SceneHdr); appends its tables to the int blob
int SceneBuild::tile_poses() {
    // tile-shared passive bodies (see SceneHdr)
    std::vector<char> pas(nmb, 0);
    std::vector<int> lvl(nmb, 0);
    int nlv = 0;
    for (int k = 0; k < nmb; k++) {
        bool p = true, is_free = false;
        for (int j = mb_jntadr[k]; j < mb_jntadr[k] + mb_jntnum[k]; j++) {
            if (mj_type[j] == J_FREE) is_free = true;
            else if (mj_qsrc[j] < na) p = false;
        }
        if (mb_parent[k] >= 0 && !is_free) { p = p && pas[mb_parent[k]]; lvl[k] = lvl[mb_parent[k]] + 1; }
        pas[k] = p ? 1 : 0;
        if (p) nlv = std::max(nlv, lvl[k] + 1);
    }
    std::vector<int32_t> pas_b, pas_lv, mb_pas(nmb, -1), pas_g, mg_pas(nmg, -1);
    for (int L = 0; L < nlv; L++) {
        pas_lv.push_back((int)pas_b.size());
        for (int k = 0; k < nmb; k++)
            if (pas[k] && lvl[k] == L) { mb_pas[k] = (int)pas_b.size(); pas_b.push_back(k); }
    }
    pas_lv.push_back((int)pas_b.size());
    for (int ms = 0; ms < nmg; ms++)
        if (pas[g_mb[mg_geom[ms]]]) { mg_pas[ms] = (int)pas_g.size(); pas_g.push_back(ms); }
    for (int k = 0; k < nmb; k++) {
        if (mb_pas[k] < 0) continue;
        bool cont = false;       // does a body that is NOT posed by the tile continue from this one's registers / saved pose?
        for (int c = 0; c < nmb; c++)
            if (mb_parent[c] == k && !pas[c]) cont = true;
        if (!cont) mb_pas[k] |= 1 << 16;
    }
    const size_t pas_min = std::getenv("MOPA_V5_TILE_MIN") ? (size_t)atoi(std::getenv("MOPA_V5_TILE_MIN")) : 4;      // (A/B knob)
    const bool on = pas_b.size() >= pas_min && pas_b.size() <= 64 && pas_g.size() <= 64 && nlv <= 8 && !std::getenv("MOPA_V5_NO_TILE_POSES");
    h.n_pas_b = on ? (int)pas_b.size() : 0; h.n_pas_g = on ? (int)pas_g.size() : 0; h.n_pas_lv = on ? nlv : 0;
    h.o_pas_b = B.add_i(pas_b); h.o_pas_lv = B.add_i(pas_lv); h.o_mb_pas = B.add_i(mb_pas); h.o_pas_g = B.add_i(pas_g); h.o_mg_pas = B.add_i(mg_pas);
    return MOPA_OK;
}

// 8. planner FK words; appends them to the int blob
int SceneBuild::planner_fk() {
    std::vector<int32_t> pfk(8 * (size_t)nmg, 0);
    int maxlen = 0;
    bool ok = nmb < 255;
    for (int ms = 0; ms < nmg && ok; ms++) {
        const int k = g_mb[mg_geom[ms]];
        const int len = chain_len[k];
        if (len > 16) { ok = false; break; }
        maxlen = std::max(maxlen, len);
        uint32_t w[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        for (int i = 0; i < len; i++) {
            const uint32_t b = (uint32_t)chain_items[chain_adr[k] + i];
            w[i >> 2] = (w[i >> 2] & ~(0xffu << (8 * (i & 3)))) | (b << (8 * (i & 3)));
        }
        for (int i = 0; i < 4; i++) pfk[8 * (size_t)ms + i] = (int32_t)w[i];
        pfk[8 * (size_t)ms + 4] = len;
        const int root = chain_items[chain_adr[k]];
        pfk[8 * (size_t)ms + 5] = (mb_parent[root] < 0) ? -(mb_parent[root] + 1) : 0;
    }
    h.o_pfk = B.add_i(pfk);
    h.pfk_maxlen = ok ? maxlen : 0;
    return MOPA_OK;
}

// 9. (continued) mesh-pass tables, header totals, wave-per-state LDS size
int SceneBuild::finish_blobs() {
    o_mgr_mesh = B.add_i(mgr_mesh); o_gp_word_mesh = B.add_i(gp_word_mesh);
    h.n_dbl = (int)B.dbl.size();
    h.n_int = (int)B.ints.size();
    h.wave_dbl = nmg * kGeomStride + na + n_pq + na + 2 * nmj;   // geom records, joint values, one spare state vector, sin/cos table
    int wl_bytes = (int)((pairs.size() * 2 + 15) & ~size_t(15));
    h.wave_bytes = ((h.wave_dbl * 8 + wl_bytes) + 15) & ~15;
    h.thr = desc->contact_threshold;
    h.range = desc->range;
    h.resolution = desc->resolution > 0.0 ? desc->resolution : 0.005;
    {
        // FP32 mirror of the planner's trees: coordinates rounded to FP32 (|x| <= X: error X 2^-24 each), their difference
        // rounded once more, na terms added with a rounding of the running sum (<= na 2X) each
        double X = kPi;
        for (int i = 0; i < na; i++) X = std::max(X, std::max(std::fabs(act_lo[i]), std::fabs(act_hi[i])));
        const double S1 = 2.0 * X * std::max(na, 1);
        h.nn_eps = (3.0 * na + 2.0) * std::ldexp(1.0, -24) * S1 * 1.5;
    }
    S->h_dbl = B.dbl;
    S->h_int = B.ints;
    S->lds_bytes = h.n_dbl * 8 + ((h.n_int + 1) & ~1) * 4 + kWavesPerBlock * h.wave_bytes;
    if (S->lds_bytes > kMaxLdsBytes) { return fail(MOPA_ERR_LIMIT, "scene does not fit the 160 KiB LDS"); }
    return MOPA_OK;
}

// 10. K1 policy: which validity kernels the scene gets, where the FP32 centre table of a tile lives, the entry caps and the LDS sizes
// (K1Policy; mopa_valid_launch.inc turns it into launches).  The creation-time knobs are parsed here and nowhere else.
int SceneBuild::k1_policy() {
    enum class Gen { Auto, V1, V2, V5 } gen = Gen::Auto;      // MOPA_VALID_KERNEL
    enum class Cen { Auto, Lds, Slab } cen = Cen::Auto;       // MOPA_V5_CENTRES: A/B runs and tests
    if (const char *ev = std::getenv("MOPA_VALID_KERNEL")) gen = !std::strcmp(ev, "v1") ? Gen::V1 : !std::strcmp(ev, "v2") ? Gen::V2 : !std::strcmp(ev, "v5") ? Gen::V5 : Gen::Auto;
    if (const char *ec = std::getenv("MOPA_V5_CENTRES")) cen = !std::strcmp(ec, "lds") ? Cen::Lds : !std::strcmp(ec, "slab") ? Cen::Slab : Cen::Auto;
    K1Policy &P = S->k1;
    P.v2_lds_bytes = h.n_dbl * 8 + ((h.n_int + 1) & ~1) * 4 + kWavesPerBlock * kV2LdsPerWave;
    P.use_v2 = gen != Gen::V1 && P.v2_lds_bytes <= kMaxLdsBytes;
    // MOPA_VALID_KERNEL=v2 / v5: the lane-per-state kernel for every N >= 64 (tests, A/B runs)
    P.v2_forced = gen == Gen::V2 || gen == Gen::V5;
    {
        // largest entry buffer (multiple of 64, 256..1024) that still lets two workgroups share a CU's 160 KiB of LDS;
        // if even the smallest does not fit with the FP32 centre table in LDS, the centres are read back from the slab
        const int fixed = h.n_dbl * 8 + ((h.n_int + 3) & ~3) * 4 + ((8 * h.n_gp + (gp_word_mesh.empty() ? 1 : 3) * nmg + 3) & ~3) * 4;
        bool cen_lds = true;
        int cap = kEntCapV5Max;
        for (int attempt = 0; attempt < 2; attempt++) {
            cen_lds = attempt == 0 && gp_word_mesh.empty();   // scenes with mesh pairs: the slab-centre instantiation carries the gate
            if (cen == Cen::Slab) cen_lds = false;
            if (cen == Cen::Lds && gp_word_mesh.empty()) cen_lds = true;   // (mesh scenes: always slab + gate)
            const int n_cen = cen_lds ? nmg : 0;
            cap = kEntCapV5Max;
            while (cap > 256 && fixed + kWavesPerBlock * v5_lds_per_wave(n_cen, cap, true) > 80 * 1024) cap -= 64;
            if (fixed + kWavesPerBlock * v5_lds_per_wave(n_cen, cap, true) <= 80 * 1024) break;
            if (cen == Cen::Lds) break;
        }
        if (fixed + kWavesPerBlock * v5_lds_per_wave(cen_lds ? nmg : 0, cap, true) > 80 * 1024) {   // one workgroup per CU anyway
            cap = 768;
            cen_lds = gp_word_mesh.empty() && cen != Cen::Slab;
        }
        P.v5_cen_lds = cen_lds;
        // (cap so far: the depth-reporting instantiations; the verdict-only ones have no depth words and take more entries)
        P.v5_ent_cap_md = cap;
        P.v5_lds_bytes_md = fixed + kWavesPerBlock * v5_lds_per_wave(cen_lds ? nmg : 0, cap, true);
        const int budget = std::max(P.v5_lds_bytes_md, 80 * 1024);
        while (cap + 64 <= kEntCapV5Max && fixed + kWavesPerBlock * v5_lds_per_wave(cen_lds ? nmg : 0, cap + 64, false) <= budget) cap += 64;
        h.v5_ent_cap = cap;
        // (the tile's passive poses overlay the entry buffer during the FK phase)
        if ((h.n_pas_b + h.n_pas_g) * 7 * 8 > 4 * std::min(cap, P.v5_ent_cap_md)) { h.n_pas_b = 0; h.n_pas_g = 0; h.n_pas_lv = 0; }
        P.v5_lds_bytes = fixed + kWavesPerBlock * v5_lds_per_wave(cen_lds ? nmg : 0, cap, false);
        if (std::getenv("MOPA_DEBUG"))
            fprintf(stderr, "[mopa] scene: nmg %d nmb %d save slots %d pairs %d (+%d mesh) lds: wave-per-state %d, v2 %d, v5 %d (entry cap %d / %d, fixed %d, centres in %s); tile-posed bodies %d geoms %d levels %d\n", nmg, nmb, n_save,
                    (int)gp_word.size(), (int)gp_word_mesh.size(), S->lds_bytes, P.v2_lds_bytes, P.v5_lds_bytes, cap, P.v5_ent_cap_md, fixed, cen_lds ? "LDS" : "slab", h.n_pas_b, h.n_pas_g, h.n_pas_lv);
    }
    // third generation (FP32 broad phase out of LDS): default wherever it applies; MOPA_VALID_KERNEL=v2 keeps the second
    // ... unless it would get one workgroup per CU where the second generation still gets two (LDS: the FP32 centre
    // table grows with the number of moving geoms; SawyerLift: 19 of them)
    const bool v5_fits2 = P.v5_lds_bytes <= 80 * 1024, v2_fits2 = P.v2_lds_bytes <= 80 * 1024;
    P.use_v5 = gen != Gen::V2 && P.use_v2 && max_pnum <= 64 && std::max(P.v5_lds_bytes, P.v5_lds_bytes_md) <= kMaxLdsBytes && reach <= kV5MaxReach &&
               (v5_fits2 || !v2_fits2 || gen == Gen::V5);
    // K2, expanded motion: a segment expands into at most ceil(1 / resolution) states (a joint cannot move further than its extent),
    // so chunks of INT32_MAX / that many segments keep every 32-bit offset of the count -> scan -> expand pipeline in range.
    // MOPA_MOTION_CHUNK (segments, clamped to 1 .. that default) is a test knob, not a tuning one: it makes a batch of a few
    // thousand segments take several chunks, so the tests reach the arithmetic on a chunk's first segment.
    const int64_t per_seg = (int64_t)std::ceil(1.0 / h.resolution) + 2;
    P.motion_chunk = std::max<int64_t>(1, 0x7fffffffLL / per_seg);
    if (const char *em = std::getenv("MOPA_MOTION_CHUNK")) P.motion_chunk = std::max<int64_t>(1, std::min<int64_t>(P.motion_chunk, atoll(em)));
    return MOPA_OK;
}

}  // namespace

// Host half of scene creation: runs the steps in order; the first refusal ends it.
// glue_a / glue_b >= 0: the glued compile of the same description (mopa_scene_create_glued); the ordinary compile's output does not
// depend on any of the glue code (every glued step is behind glued()).
static int scene_build_host(const MopaSceneDesc *desc, MopaScene *S, int glue_a = -1, int glue_b = -1) {
    SceneBuild W(desc, S, glue_a, glue_b);
    for (int (SceneBuild::*step)() : {&SceneBuild::check_model, &SceneBuild::split_active, &SceneBuild::static_frames, &SceneBuild::moving_bodies,
                                      &SceneBuild::geoms_and_pairs, &SceneBuild::dfs_program, &SceneBuild::pair_lists, &SceneBuild::fp32_table,
                                      &SceneBuild::packed_records, &SceneBuild::assemble_tables, &SceneBuild::tile_poses, &SceneBuild::planner_fk,
                                      &SceneBuild::finish_blobs, &SceneBuild::k1_policy}) {
        const int rc = (W.*step)();
        if (rc != MOPA_OK) return rc;
    }
    S->hdr_mesh = S->hdr;
    S->hdr_mesh.o_mgr = W.o_mgr_mesh; S->hdr_mesh.o_gp_word = W.o_gp_word_mesh; S->hdr_mesh.n_gp = (int)W.gp_word_mesh.size();
    S->n_mesh_gp = (int)W.gp_word_mesh.size();
    if (W.glued()) {
        S->glue_a = glue_a; S->glue_b = glue_b;
        S->glue_mb_a = W.mb_of_body[glue_a]; S->glue_mb_b = W.mb_of_body[glue_b];
        S->glue_adr = desc->model.jnt_qposadr[desc->model.body_jntadr[glue_b]];
        if (S->glue_mb_a < 0 || S->glue_mb_b < 0) return fail(MOPA_ERR_UNSUPPORTED, "glue: body_b carries no collidable geom (nothing to glue)");
    }
    return MOPA_OK;
}

// The bytes k_is_valid_v5 reads from a scene -- both blobs, the FP32 pair table, the header (no padding: asserted) -- hashed
// (FNV-1a, 64 bit).  A baked instantiation is launched only for a scene whose fingerprint equals the baked one.  The
// planner's fields of the header (range, resolution, nn_eps: never read by K1) are hashed as zeros, so the planner
// settings of a Scene do not decide which K1 it gets.
static_assert(offsetof(SceneHdr, thr) == offsetof(SceneHdr, wave_bytes) + sizeof(int) && sizeof(SceneHdr) == offsetof(SceneHdr, nn_eps) + sizeof(double),
              "SceneHdr has padding: k1_fingerprint would hash indeterminate bytes");
static uint64_t k1_fingerprint(const MopaScene *S) {
    Fnv f;
    f.add(S->h_dbl);
    f.add(S->h_int);
    f.add(S->h_gp_tab);
    SceneHdr h = S->hdr;
    h.range = 0.0; h.resolution = 0.0; h.nn_eps = 0.0;
    f.add(&h, sizeof(SceneHdr));
    return f.f;
}
// baked scene of this fingerprint (its index in MOPA_K1_BAKED_SCENES, from 1), 0 = none
static int k1_baked_index(uint64_t fp) {
#define MOPA_K1_MATCH(i_, T_) if (fp == T_::kFingerprint) return i_;
    MOPA_K1_BAKED_SCENES(MOPA_K1_MATCH)
#undef MOPA_K1_MATCH
    return 0;
}
