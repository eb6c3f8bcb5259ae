// mopa_model_host.hpp -- host side of every body walk, shared by the compilers of both translation units (mopa_hip.hip: scene, IK;
// mopa_envdyn.hip: env, servo dynamics): the structure check of a MopaModel, the pose save-slot program of a depth-first walk, the
// body record, the blob packer with its upload, the device pick, the fingerprint of compiled tables.  Host code only: nothing here
// needs a device but upload_tables and pick_device, which a compiler calls after it has compiled.
#pragma once
#include <algorithm>
#include <memory>

#include "mopa_host.hpp"

// Depth-first order of a parent list (parent[k] < k; parent < 0: a root): every body's parent is the body just before it or one of
// that body's ancestors.  depth_first_at: body k keeps the order, given that the bodies before it do; parents_depth_first: the first
// body that breaks it, -1 = none.
static inline bool depth_first_at(const int32_t *parent, int k) {
    int a = k - 1;
    while (a > parent[k]) a = parent[a];
    return a == parent[k];
}
static inline int parents_depth_first(const int32_t *parent, int n) {
    for (int k = 1; k < n; k++)
        if (!depth_first_at(parent, k)) return k;
    return -1;
}

// The pose save-slot program of a walk over bodies in depth-first order (parent[k] < k; parent < 0: a root).  A body whose parent is
// not the body just before it reloads the parent's pose from a slot; slots are numbered by the count of saved proper ancestors, so a
// slot is free again exactly when the walk has left the subtree that parked a pose in it -- which holds in depth-first order only.
// load[k * stride]: -2 root, -1 the previous body's pose is the parent's, else the slot to load; save[k * stride]: the slot this body's
// pose goes to, -1 none (stride: the int records of a walk hold the two side by side).  Returns the number of slots.
static inline int save_slot_program(const int32_t *parent, int n, int32_t *load, int32_t *save, int stride = 1) {
    std::vector<char> need_save(n, 0);
    for (int k = 0; k < n; k++)
        if (parent[k] >= 0 && parent[k] != k - 1) need_save[parent[k]] = 1;
    std::vector<int> depth(n, 0);      // number of saved proper ancestors
    int n_save = 0;
    for (int k = 0; k < n; k++) {
        const int pk = parent[k];
        depth[k] = (pk >= 0) ? depth[pk] + (need_save[pk] ? 1 : 0) : 0;
        save[k * stride] = need_save[k] ? depth[k] : -1;
        if (need_save[k]) n_save = std::max(n_save, depth[k] + 1);
        load[k * stride] = (pk < 0) ? -2 : (pk == k - 1 ? -1 : save[pk * stride]);
    }
    return n_save;
}

// The structure every compiler indexes with (the preconditions of MopaModel, include/mopa_hip.h).  MuJoCo's compiler emits nothing
// else; a model built by hand is refused here instead of read out of bounds there.
static inline int check_model_structure(const MopaModel &m) {
    if (m.njnt < 0 || m.npair < 0 || m.nmesh < 0 || m.nmeshvert < 0) return fail(MOPA_ERR_INVALID_ARG, "negative count in the model");
    for (int b = 1; b < m.nbody; b++) {
        const int p = m.body_parent[b];
        if (p < 0 || p >= b) return fail(MOPA_ERR_INVALID_ARG, "body_parent[" + std::to_string(b) + "] out of range (a body's parent must come before it)");
        // (save_slot_program needs the order; checked body by body, so that the first defect in body order is the one reported)
        if (!depth_first_at(m.body_parent, b)) return fail(MOPA_ERR_UNSUPPORTED, "bodies are not in depth-first order (body " + std::to_string(b) + ")");
    }
    for (int b = 0; b < m.nbody; b++) {
        const int n = m.body_jntnum[b], a = m.body_jntadr[b];
        if (n < 0 || (n > 0 && (a < 0 || a > m.njnt - n))) return fail(MOPA_ERR_INVALID_ARG, "body_jntadr + body_jntnum out of range (body " + std::to_string(b) + ")");
    }
    for (int j = 0; j < m.njnt; j++) {
        const int t = m.jnt_type[j];
        if (t != MOPA_JNT_FREE && t != MOPA_JNT_BALL && t != MOPA_JNT_SLIDE && t != MOPA_JNT_HINGE) return fail(MOPA_ERR_INVALID_ARG, "unknown joint type " + std::to_string(t));
        const int w = (t == MOPA_JNT_FREE) ? 7 : (t == MOPA_JNT_BALL ? 4 : 1);
        if (m.jnt_qposadr[j] < 0 || m.jnt_qposadr[j] > m.nq - w) return fail(MOPA_ERR_INVALID_ARG, "jnt_qposadr out of range (joint " + std::to_string(j) + ")");
    }
    for (int g = 0; g < m.ngeom; g++)   // (a mesh geom's geom_dataid: the scene's static_frames, with the hull it names)
        if (m.geom_body[g] < 0 || m.geom_body[g] >= m.nbody) return fail(MOPA_ERR_INVALID_ARG, "geom_body out of range (geom " + std::to_string(g) + ")");
    return MOPA_OK;
}

// The 14 doubles of a walk's body record: local pos[3] quat[4], then the first joint's axis[3] anchor[3] ref (a free joint's ref is 0);
// a jointless body leaves the joint part as it is.
static inline void fill_body_record(const MopaModel &m, int b, double *d) {
    std::memcpy(d, m.body_pos + 3 * b, 24);
    std::memcpy(d + 3, m.body_quat + 4 * b, 32);
    if (m.body_jntnum[b] <= 0) return;
    const int j = m.body_jntadr[b];
    std::memcpy(d + 7, m.jnt_axis + 3 * j, 24);
    std::memcpy(d + 10, m.jnt_pos + 3 * j, 24);
    d[13] = (m.jnt_type[j] == MOPA_JNT_FREE) ? 0.0 : m.jnt_ref[j];
}

// The two tables a walk's kernels read: every array starts at a 16-byte (doubles) / 32-byte (ints) boundary; add_* return its offset.
struct BlobPacker {
    std::vector<double> D;
    std::vector<int32_t> I;
    int add_d(const double *p, size_t n) { const int o = (int)D.size(); D.insert(D.end(), p, p + n); while (D.size() & 1) D.push_back(0.0); return o; }
    int add_i(const int32_t *p, size_t n) { const int o = (int)I.size(); I.insert(I.end(), p, p + n); while (I.size() & 7) I.push_back(0); return o; }
    int add_d(const std::vector<double> &v) { return add_d(v.data(), v.size()); }
    int add_i(const std::vector<int32_t> &v) { return add_i(v.data(), v.size()); }
};

// One device array from a host one; on failure nothing is left allocated.
template <class T>
static inline hipError_t upload_array(const T *src, size_t n, T **dst) {
    T *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T));
    if (e == hipSuccess && n) e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (p) (void)hipFree(p); return e; }
    *dst = p;
    return hipSuccess;
}
// Both tables to the current device, into their owner's fields: after a failure the owner frees what is there, as it does anyway.
static inline hipError_t upload_tables(const std::vector<double> &D, const std::vector<int32_t> &I, double **d_dbl, int32_t **d_int) {
    const hipError_t e = upload_array(D.data(), D.size(), d_dbl);
    return e != hipSuccess ? e : upload_array(I.data(), I.size(), d_int);
}

// The device an object lives on: ordinal `wanted`, or the caller's current device when wanted < 0.  no_device: the caller's own words
// for a machine without one.
static inline int pick_device(int wanted, int *device, const char *no_device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MOPA_ERR_HIP, no_device);
    if (wanted >= ndev) return fail(MOPA_ERR_INVALID_ARG, "device ordinal out of range");
    if (wanted >= 0) *device = wanted;
    else if (hipGetDevice(device) != hipSuccess) return fail(MOPA_ERR_HIP, "hipGetDevice failed");
    return MOPA_OK;
}

// FNV-1a, 64 bit: the fingerprint of compiled tables (the scene's k1_fingerprint, mopa_env / _ik / _dyn_tables_host).  Hash values, never
// a struct's padding bytes.
struct Fnv {
    uint64_t f = 0xcbf29ce484222325ull;
    void add(const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; i++) f = (f ^ b[i]) * 0x100000001b3ull;
    }
    template <class T> void add(const std::vector<T> &v) { add(v.data(), v.size() * sizeof(T)); }
};
