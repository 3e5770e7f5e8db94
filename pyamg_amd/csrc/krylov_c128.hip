// Complex128 vector kernels of the device-resident Krylov methods (pyamg_amd/krylov_c128.py; include/amgcore_hip.h,
// section 5, amg_devx_*): the conjugated inner product, the BLAS-1 updates and the Householder sequences of the two
// GMRES variants (amg_core/krylov.h: apply_householders, householder_hornerscheme).  Vectors are caller-supplied
// device pointers to (re, im) pairs of doubles; every launch is eager on the caller's stream (the hierarchy's).
//
// Arithmetic: products and sums go through scalar.hpp (the library builds with
// -ffp-contract=off), so every update kernel has one fixed rounding per real operation.  zdotc sums in a fixed order
// that depends on n alone: entry k goes to thread k mod (ZDOT_BLOCKS ZDOT_WG) in ascending k, a workgroup adds its
// ZDOT_WG sums by a halving tree, one workgroup adds the ZDOT_BLOCKS partial sums the same way.
//
// Scratch (amg_hierx_scratch): ZDOT_BLOCKS partial sums followed by AMG_DEVX_SLOTS result slots, all complex128.
#include "driver.hpp"
#include "../../include/amgcore_hip.h"
#include "scalar.hpp"

using namespace amg;
using namespace amg::sc;

namespace {

constexpr int ZDOT_BLOCKS = AMG_DEVX_PARTIALS;
constexpr int ZDOT_WG = 256;
constexpr int VEC_WG = 256;

int blocks_of(long n, int per) { return (int)((n + per - 1) / per); }

// the workgroup's ZDOT_WG values added by a halving tree; the sum is s[0]
__device__ void tree_sum(c128 *s)
{
    __syncthreads();
    for (int w = ZDOT_WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = add(s[threadIdx.x], s[threadIdx.x + w]);
        __syncthreads();
    }
}

// part[block] = sum over the block's entries of conj(x_k) y_k
__global__ void __launch_bounds__(ZDOT_WG)
zdotc_partial(const c128 *__restrict__ x, const c128 *__restrict__ y, long n, c128 *__restrict__ part)
{
    __shared__ c128 s[ZDOT_WG];
    c128 acc = from_real<c128>(0.0);
    for (long k = (long)blockIdx.x * ZDOT_WG + threadIdx.x; k < n; k += (long)gridDim.x * ZDOT_WG)
        acc = add(acc, mul(conj(x[k]), y[k]));
    s[threadIdx.x] = acc;
    tree_sum(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(ZDOT_WG) zdotc_final(const c128 *__restrict__ part, int np, c128 *__restrict__ out)
{
    __shared__ c128 s[ZDOT_WG];
    c128 acc = from_real<c128>(0.0);
    for (int k = threadIdx.x; k < np; k += ZDOT_WG) acc = add(acc, part[k]);
    s[threadIdx.x] = acc;
    tree_sum(s);
    if (threadIdx.x == 0) out[0] = s[0];
}

// y += a x; the scalar by value, or (slot[0] scaled component-wise by the real f) read from device memory
__global__ void axpy_kernel(long n, c128 *__restrict__ y, const c128 *__restrict__ x, c128 a,
                            const c128 *__restrict__ slot, double f)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot) a = mulr(slot[0], f);
    if (i < n) y[i] = add(y[i], mul(a, x[i]));
}

// p = beta p + z
__global__ void xpby_kernel(long n, c128 *__restrict__ p, c128 beta, const c128 *__restrict__ z)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = add(mul(beta, p[i]), z[i]);
}

// out = c x (out may be x)
__global__ void scale_kernel(long n, c128 *out, const c128 *x, c128 c)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mul(c, x[i]);
}

// out = a - b (out may be a or b)
__global__ void sub_kernel(long n, c128 *out, const c128 *a, const c128 *b)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sub(a[i], b[i]);
}

__global__ void fill_kernel(long n, c128 *__restrict__ x, c128 v)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}

// z[j] += y[j] (householder_hornerscheme, krylov.h:111)
__global__ void add_entry(c128 *__restrict__ z, const c128 *__restrict__ y, long j)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) z[j] = add(z[j], y[j]);
}

int zdotc(const c128 *x, const c128 *y, long n, c128 *scratch, c128 *slot, hipStream_t st)
{
    hipLaunchKernelGGL(zdotc_partial, dim3(ZDOT_BLOCKS), dim3(ZDOT_WG), 0, st, x, y, n, scratch);
    CHK(launched("zdotc partial"));
    hipLaunchKernelGGL(zdotc_final, dim3(1), dim3(ZDOT_WG), 0, st, (const c128 *)scratch, ZDOT_BLOCKS, slot);
    return launched("zdotc final");
}

int axpy(c128 *y, const c128 *x, c128 a, const c128 *slot, double f, long n, hipStream_t st)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(axpy_kernel, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, st, n, y, x, a, slot, f);
    return launched("axpy");
}

// v <- v - 2 <w, v> w (krylov.h:47-50: alpha = dot_prod(w, v); alpha *= -2; v += alpha w); alpha stays on the device
int reflect(c128 *v, const c128 *w, long n, c128 *scratch, hipStream_t st)
{
    c128 *slot = scratch + ZDOT_BLOCKS;
    CHK(zdotc(w, v, n, scratch, slot, st));
    return axpy(v, w, c128{0.0, 0.0}, slot, -2.0, n, st);
}

// the reflectors j = start, start + step, ... (stop excluded) all lie in W[0 .. nW)
int check_range(const void *v, const void *const *W, int nW, long n, int start, int stop, int step, const void *scratch)
{
    if (!v || !scratch || n < 0 || step == 0) { set_error("bad Householder arguments"); return AMG_EINVAL; }
    if (start == stop) return 0;
    const int last = stop - step;
    if (!W || (stop - start) % step != 0 || (stop - start) / step < 0 || start < 0 || start >= nW || last < 0 || last >= nW) {
        set_error("bad Householder range");
        return AMG_EINVAL;
    }
    for (int j = start; j != stop; j += step)
        if (!W[j]) { set_error("null Householder vector"); return AMG_EINVAL; }
    return 0;
}

}  // namespace

extern "C" {

int amg_devx_zdotc(const void *x, const void *y, long n, void *scratch, int slot, double *host, void *stream)
{
    if (!x || !y || !scratch || n < 0 || slot < 0 || slot >= AMG_DEVX_SLOTS) { set_error("bad zdotc arguments"); return AMG_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    c128 *out = (c128 *)scratch + ZDOT_BLOCKS + slot;
    CHK(zdotc((const c128 *)x, (const c128 *)y, n, (c128 *)scratch, out, st));
    if (host) {
        AMG_HIP(hipMemcpyAsync(host, out, sizeof(c128), hipMemcpyDeviceToHost, st));
        AMG_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int amg_devx_axpy(void *y, const void *x, double are, double aim, long n, void *stream)
{
    return axpy((c128 *)y, (const c128 *)x, c128{are, aim}, nullptr, 0.0, n, (hipStream_t)stream);
}

int amg_devx_axpy_slot(void *y, const void *x, const void *scratch, int slot, double factor, long n, void *stream)
{
    if (!scratch || slot < 0 || slot >= AMG_DEVX_SLOTS) { set_error("bad slot"); return AMG_EINVAL; }
    return axpy((c128 *)y, (const c128 *)x, c128{0.0, 0.0}, (const c128 *)scratch + ZDOT_BLOCKS + slot, factor, n,
                (hipStream_t)stream);
}

int amg_devx_xpby(void *p, double bre, double bim, const void *z, long n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(xpby_kernel, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, (hipStream_t)stream, n, (c128 *)p,
                       c128{bre, bim}, (const c128 *)z);
    return launched("xpby");
}

int amg_devx_scale(void *out, const void *x, double cre, double cim, long n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(scale_kernel, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, (hipStream_t)stream, n, (c128 *)out,
                       (const c128 *)x, c128{cre, cim});
    return launched("scale");
}

int amg_devx_sub(void *out, const void *a, const void *b, long n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sub_kernel, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, (hipStream_t)stream, n, (c128 *)out,
                       (const c128 *)a, (const c128 *)b);
    return launched("sub");
}

int amg_devx_fill(void *x, double vre, double vim, long n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, (hipStream_t)stream, n, (c128 *)x,
                       c128{vre, vim});
    return launched("fill");
}

int amg_devx_copy(void *dst, const void *src, long n, int kind, void *stream)
{
    if (n <= 0) return 0;
    if (kind < 0 || kind > 2) { set_error("bad copy kind"); return AMG_EINVAL; }
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    AMG_HIP(hipMemcpyAsync(dst, src, sizeof(c128) * (size_t)n, k, (hipStream_t)stream));
    if (kind != 2) AMG_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int amg_devx_householders(void *v, const void *const *W, int nW, long n, int start, int stop, int step, void *scratch,
                          void *stream)
{
    CHK(check_range(v, W, nW, n, start, stop, step, scratch));
    for (int j = start; j != stop; j += step)
        CHK(reflect((c128 *)v, (const c128 *)W[j], n, (c128 *)scratch, (hipStream_t)stream));
    return 0;
}

int amg_devx_horner(void *v, const void *const *W, int nW, const void *y, long n, int start, int stop, int step,
                    void *scratch, void *stream)
{
    CHK(check_range(v, W, nW, n, start, stop, step, scratch));
    if (start != stop && !y) { set_error("null y"); return AMG_EINVAL; }
    for (int j = start; j != stop; j += step) {
        if (j >= n) { set_error("Householder index beyond the vector"); return AMG_EINVAL; }
        hipLaunchKernelGGL(add_entry, dim3(1), dim3(64), 0, (hipStream_t)stream, (c128 *)v, (const c128 *)y, (long)j);
        CHK(launched("horner entry"));
        CHK(reflect((c128 *)v, (const c128 *)W[j], n, (c128 *)scratch, (hipStream_t)stream));
    }
    return 0;
}

}  // extern "C"
