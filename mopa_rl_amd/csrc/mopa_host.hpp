// mopa_host.hpp -- host-side plumbing shared by the translation units of libmopa_hip.so (mopa_hip.hip: scene, K1-K3, K5,
// path post-processing; mopa_envdyn.hip: K4 env.step, K6 servo dynamics, K7 contacts): error state, HIP call check,
// device guard, grow-only device buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mopa_hip.h"

constexpr int kMaxLdsBytes = 160 * 1024;   // LDS per CU on gfx950
int mopa_fail(int code, const std::string &msg);      // sets the thread's last error (mopa_last_error) and returns `code`
static inline int fail(int code, const std::string &msg) { return mopa_fail(code, msg); }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(MOPA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

// Every entry point runs on its object's device and leaves the caller's current device as it found it (a torch process
// that touches several GPUs keeps its own notion of "current").
class DeviceGuard {
    int prev_ = -1;
    bool ok_ = false, switched_ = false;
public:
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev_) != hipSuccess) return;
        if (prev_ != device) {
            if (hipSetDevice(device) != hipSuccess) return;
            switched_ = true;
        }
        ok_ = true;
    }
    ~DeviceGuard() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    bool ok() const { return ok_; }
};
#define ON_DEVICE(dev)                                                        \
    DeviceGuard _guard(dev);                                                  \
    if (!_guard.ok()) return fail(MOPA_ERR_HIP, "cannot switch to the object's HIP device")

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;     // bytes
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// The device block behind a single-state form (host pointers in, host pointers out, synchronous): its fields are declared in
// order -- doubles, then int32, then bytes, so every field is aligned by construction -- alloc() is the one hipMalloc, dev() hands
// the batch form typed device pointers, fetch() copies the WHOLE block back at once into a host mirror that host() / out() read.
// seed() uploads one field (a segment form's qb).  The block is freed with the object.
class Staging {
public:
    template <class T> struct Field { size_t off, n; };       // byte offset in the block, elements
private:
    size_t bytes_ = 0, last_size_ = sizeof(double);
    unsigned char *dev_ = nullptr;
    std::vector<unsigned char> host_;
    template <class T> Field<T> add(size_t n) {
        assert(!dev_ && sizeof(T) <= last_size_);
        const Field<T> f{bytes_, n};
        last_size_ = sizeof(T);
        bytes_ += n * sizeof(T);
        return f;
    }
public:
    Field<double> dbl(size_t n) { return add<double>(n); }
    Field<int32_t> i32(size_t n) { return add<int32_t>(n); }
    Field<uint8_t> u8(size_t n) { return add<uint8_t>(n); }
    hipError_t alloc() { return hipMalloc(reinterpret_cast<void **>(&dev_), bytes_ ? bytes_ : 8); }
    template <class T> T *dev(Field<T> f) const { return reinterpret_cast<T *>(dev_ + f.off); }
    hipError_t seed(Field<double> f, const double *src) { return hipMemcpy(dev(f), src, f.n * sizeof(double), hipMemcpyHostToDevice); }
    hipError_t fetch() {       // (synchronises with the null stream's launches)
        host_.resize(bytes_);
        return bytes_ ? hipMemcpy(host_.data(), dev_, bytes_, hipMemcpyDeviceToHost) : hipSuccess;
    }
    template <class T> const T *host(Field<T> f) const { return reinterpret_cast<const T *>(host_.data() + f.off); }
    template <class T> void out(Field<T> f, T *dst) const {       // the field into a caller's buffer (null: not asked for)
        if (dst) std::memcpy(dst, host(f), f.n * sizeof(T));
    }
    Staging() = default;
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() {
        if (dev_) (void)hipFree(dev_);
    }
};

// bounding radius of a primitive geom about its origin
static inline double rbound_of(int type, const double *sz) {
    switch (type) {
        case 2: return sz[0];                                                            // sphere
        case 3: return sz[0] + sz[1];                                                    // capsule
        case 5: return sqrt(fma(sz[1], sz[1], sz[0] * sz[0]));                           // cylinder
        case 6: return sqrt(fma(sz[2], sz[2], fma(sz[1], sz[1], sz[0] * sz[0])));        // box
        default: return 0.0;
    }
}
