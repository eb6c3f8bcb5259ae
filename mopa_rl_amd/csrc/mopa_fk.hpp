// mopa_fk.hpp -- the pieces of the body-pose step that every forward-kinematics walk shares (included after mopa_device.hpp).
//
// Every walker (fk_one_geom, ms_fk, k_is_valid_v2, k_is_valid_v5 generic and baked, glue_walk, env_step_lane, the two IK walks) poses a
// body as  parent pose -> body offset -> joints -> normalise -> matrix  and must give the CPU oracle's pose bit for bit.  The walks keep
// their own loops -- their kernels' register allocation hangs on the loops' shape -- and are written over these
// pieces.  Everything is MOPA_HD: the arithmetic and its order are the contract.
#pragma once

namespace mopa {

// 7 doubles, pos then quat, STRIDE apart (64: a lane's column of a slab / save slot; 1: a row)
template <int STRIDE>
MOPA_HD void pose7_ld(const double *p, V3 &pos, Q4 &quat) {
    pos = V3{p[0], p[STRIDE], p[2 * STRIDE]};
    quat = Q4{p[3 * STRIDE], p[4 * STRIDE], p[5 * STRIDE], p[6 * STRIDE]};
}
template <int STRIDE>
MOPA_HD void pose7_st(double *p, V3 pos, Q4 quat) {
    p[0] = pos.x; p[STRIDE] = pos.y; p[2 * STRIDE] = pos.z;
    p[3 * STRIDE] = quat.w; p[4 * STRIDE] = quat.x; p[5 * STRIDE] = quat.y; p[6 * STRIDE] = quat.z;
}
// static frame `sf` of the scene blob: position, quaternion and the matrix the compiler stored with them
template <class H>
MOPA_HD void sf_frame_ld(const H &h, const double *D, int sf, V3 &ppos, Q4 &pquat, double *mat) {
    ppos = ld3(D + h.o_sf_pos + 3 * sf);
    const double *sq = D + h.o_sf_quat + 4 * sf;
    pquat = Q4{sq[0], sq[1], sq[2], sq[3]};
    const double *sm = D + h.o_sf_mat + 9 * sf;
#pragma unroll
    for (int i = 0; i < 9; i++) mat[i] = sm[i];
}
// a body with one free joint: its pose is the joint's 7 values
MOPA_HD void fk_free_step(const double *qp, V3 &pos, Q4 &quat) {
    pos = V3{qp[0], qp[1], qp[2]};
    quat = quat_normalize(Q4{qp[3], qp[4], qp[5], qp[6]});
}
// the carried body of a glued scene (J_GLUE): its offset under the parent is the 7 values of its free-joint slots (not normalised here)
MOPA_HD void fk_glue_step(V3 ppos, Q4 pquat, const double *mat, const double *qp, V3 &pos, Q4 &quat) {
    pos = add3(ppos, mat_vec(mat, ld3(qp)));
    quat = quat_mul(pquat, Q4{qp[3], qp[4], qp[5], qp[6]});
}
// world pose of a moving geom; gd = lpos[3] lquat[4] of its record
MOPA_HD void fk_geom_pose(V3 pos, Q4 quat, const double *mat, const double *gd, V3 &gp, Q4 &gq) {
    gp = add3(pos, mat_vec(mat, ld3(gd)));
    gq = quat_mul(quat, Q4{gd[3], gd[4], gd[5], gd[6]});
}
// posed geom record: position, matrix, and the size copied from the scene's record `srec`
MOPA_HD void fk_geom_rec_st(double *rec, V3 gp, Q4 gq, const double *srec) {
    double gm[9];
    quat2mat(gm, gq);
    st3(rec + GO_POS, gp);
#pragma unroll
    for (int i = 0; i < 9; i++) rec[GO_MAT + i] = gm[i];
    rec[GO_SIZE] = srec[GO_SIZE]; rec[GO_SIZE + 1] = srec[GO_SIZE + 1]; rec[GO_SIZE + 2] = srec[GO_SIZE + 2];
}

}  // namespace mopa
