// Host-side driver helpers shared by the translation units of libamgcore_hip.so: the launch checks, the launch
// geometry of the one-lane-per-item setup kernels, an owning device buffer and a stage timer.  Everything here has
// internal linkage: the library exports nothing from this header.
#pragma once
#include "amg_dev.hpp"

#include <algorithm>
#include <chrono>

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

// Owning device buffer.  Every allocation reaches 128 bytes (PAD doubles) past what was asked for, so a buffer of
// no bytes is still a valid pointer and a 16-byte load that starts inside the array ends inside the allocation.
struct DBuf {
    void *p = nullptr;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    DBuf(DBuf &&o) noexcept : p(o.p) { o.p = nullptr; }      // for the vectors of per-level buffer sets
    ~DBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes)
    {
        hipError_t e = hipMalloc(&p, bytes + PAD * sizeof(double));
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
    template <class T> T *as() const { return (T *)p; }
    double *d() const { return as<double>(); }
    int *i() const { return as<int>(); }
};

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

}  // namespace
}  // namespace amg
