// Host-side driver helpers shared by the translation units of libamgcore_hip.so: the error macros, the launch
// checks, the launch geometry of the one-lane-per-item setup kernels, the owner of device memory and a stage timer.
// Apart from the two error functions and the allocation counter, everything here has internal or hidden linkage:
// the library exports nothing else from this header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>

namespace amg {

// ---------------------------------------------------------------- errors
void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);
#define AMG_HIP(call)                                                         \
    do {                                                                      \
        hipError_t e__ = (call);                                              \
        if (e__ != hipSuccess) return amg::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)
// an internal call that returns one of the library's own status codes
#define CHK(call)                   \
    do {                            \
        int rc__ = (call);          \
        if (rc__ != 0) return rc__; \
    } while (0)

// Arrays are over-allocated by PAD entries so that 16-byte vector loads that
// start up to 3 entries before / end up to 3 entries after a row block stay in
// bounds.
constexpr int PAD = 16;

// ---------------------------------------------------------------- device memory
// Live device allocations of the whole process that a DevArr made and still holds (amg_dev_live_buffers).
extern std::atomic<long> dev_live __attribute__((visibility("hidden")));

// Owner of ONE device allocation: move-only, frees in its destructor, reads as a T* wherever one is expected.  It is
// about lifetime only: size, fill, synchronisation and byte accounting stay with the caller (dev_alloc in hier.hip,
// DBuf below).  release() hands the pointer to a caller outside the library, who frees it through the C ABI.
template <class T> struct __attribute__((visibility("hidden"))) DevArr {
    T *p = nullptr;
    DevArr() = default;
    DevArr(const DevArr &) = delete;
    DevArr &operator=(const DevArr &) = delete;
    DevArr(DevArr &&o) noexcept : p(o.p) { o.p = nullptr; }
    template <class U> DevArr(DevArr<U> &&o) noexcept : p(o.p) { o.p = nullptr; }      // a typed array into a void one
    DevArr &operator=(DevArr &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevArr() { reset(); }
    void reset()
    {
        if (!p) return;
        hipFree(p);
        p = nullptr;
        dev_live.fetch_sub(1, std::memory_order_relaxed);
    }
    T *release()
    {
        T *q = p;
        p = nullptr;
        if (q) dev_live.fetch_sub(1, std::memory_order_relaxed);
        return q;
    }
    hipError_t malloc_bytes(size_t bytes)      // exactly `bytes`, uninitialised; frees what it held
    {
        reset();
        hipError_t e = hipMalloc((void **)&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        dev_live.fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    operator T *() const { return p; }
    template <class U> U *as() const { return (U *)p; }
};

// Untyped owner for the setup stages.  Every allocation reaches 128 bytes (PAD doubles) past what was asked for, so a
// buffer of no bytes is still a valid pointer and a 16-byte load that starts inside the array ends inside the allocation.
// One type for the whole library (hidden, not unit-local), so that a function that crosses units can take one.
struct __attribute__((visibility("hidden"))) DBuf : DevArr<void> {
    int alloc(size_t bytes)
    {
        hipError_t e = malloc_bytes(bytes + PAD * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
        return 0;
    }
    int zero(size_t bytes)
    {
        CHK(alloc(bytes));
        AMG_HIP(hipMemset(p, 0, bytes + PAD * sizeof(double)));
        return 0;
    }
    int from_host(const void *src, size_t bytes)
    {
        CHK(alloc(bytes));
        if (bytes) AMG_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    int to_host(void *dst, size_t bytes) const
    {
        if (bytes) AMG_HIP(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    double *d() const { return as<double>(); }
    int *i() const { return as<int>(); }
};

}  // namespace amg

// after a launch inside a function that returns a status: leave with the launch's error, if it has one
#define LAUNCH_CHECK(what)                                                            \
    do {                                                                              \
        hipError_t e__ = hipGetLastError();                                           \
        if (e__ != hipSuccess) return amg::hip_fail(e__, what, __FILE__, __LINE__);   \
    } while (0)
// the same as the last statement of a launch wrapper: leaves either way, with 0 after a good launch
#define LAUNCH_RETURN(what) \
    do {                    \
        LAUNCH_CHECK(what); \
        return 0;           \
    } while (0)

namespace amg {
namespace {

// LAUNCH_CHECK as an expression, for `return launched(...)` and `CHK(launched(...))`
[[maybe_unused]] int launched(const char *what)
{
    LAUNCH_RETURN(what);
}

// one lane per item in workgroups of TB; an empty launch still gets one workgroup
constexpr int TB = 256;
inline dim3 grid_for(long work) { return dim3((unsigned)std::max<long>(1, (work + TB - 1) / TB)); }

// stage timer on the steady clock: lap() is the milliseconds since the previous lap (the first: since construction)
struct LapClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap()
    {
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return ms;
    }
};

// the times a stage entry reports, before anything has run (a caller may pass none)
inline void clear_times(double *times_ms, int count = 3) { if (times_ms) std::fill(times_ms, times_ms + count, 0.0); }

}  // namespace
}  // namespace amg
