// Value-type templated relaxation kernels shared by the flat float32 / complex64 / complex128 table
// (typed.hip) and the complex128 resident hierarchy (hier_c128.hip, on the host scaffold of resident.hpp).
// Every expression goes through the scalar rules of scalar.hpp, so a kernel gives the reference's bits
// whichever file launches it.
#pragma once
#include <hip/hip_runtime.h>

#include "scalar.hpp"

namespace amg {
namespace tk {
// internal linkage: every file that launches them registers its own copies
namespace {

using namespace amg::sc;

constexpr int ROWS_PER_WG = 256;    // rows of one SpMV / Jacobi workgroup (one thread per row)
constexpr int CHUNK = 1024;         // entries whose products are staged in LDS at a time
constexpr int LEVEL_WG = 128;       // threads of a level launch

// MATVEC: y[i] = y[i] + sum_k a_k x_k (scipy's csr_matvec).  JACOBI (relaxation.h:201-239): rows of the sweep
// (start, start+step, ...) in [lo, hi); x[i] = (1 - w) temp[i] + w ((b[i] - sum_{j != i} a_ij temp[j]) / a_ii).
enum { ROWS_MATVEC = 0, ROWS_JACOBI = 1 };

template <class T, int MODE>
__global__ void __launch_bounds__(ROWS_PER_WG)
rows_stream(int lo, int hi, int start, int step, const int *__restrict__ Ap, const int *__restrict__ Aj,
            const T *__restrict__ Ax, const T *__restrict__ v, const T *__restrict__ b, const T *__restrict__ omega,
            T *__restrict__ out)
{
    __shared__ T prod[CHUNK];
    __shared__ int col[MODE == ROWS_JACOBI ? CHUNK : 1];
    const int r0 = lo + blockIdx.x * ROWS_PER_WG;
    const int r1 = min(hi, r0 + ROWS_PER_WG);
    const int i = r0 + (int)threadIdx.x;
    const bool mine = i < r1;
    const int e0 = Ap[r0], e1 = Ap[r1];
    const int rs = mine ? Ap[i] : 0, re = mine ? Ap[i + 1] : 0;
    T acc = MODE == ROWS_MATVEC ? (mine ? out[i] : from_real<T>(0.0)) : from_real<T>(0.0);
    T diag = from_real<T>(0.0);
    for (int c0 = e0; c0 < e1; c0 += CHUNK) {
        const int cn = min(CHUNK, e1 - c0);
        for (int k = threadIdx.x; k < cn; k += ROWS_PER_WG) {
            const int j = Aj[c0 + k];
            prod[k] = mul(Ax[c0 + k], v[j]);
            if (MODE == ROWS_JACOBI) col[k] = j;
        }
        __syncthreads();
        const int a = max(rs, c0), z = min(re, c0 + cn);
        for (int k = a; k < z; ++k) {
            if (MODE == ROWS_JACOBI && col[k - c0] == i) diag = Ax[k];
            else acc = add(acc, prod[k - c0]);
        }
        __syncthreads();
    }
    if (!mine) return;
    if (MODE == ROWS_MATVEC) {
        out[i] = acc;
    } else if ((i - start) % step == 0 && nonzero(diag)) {
        const T w = omega[0];
        out[i] = add(mul(sub(from_real<T>(1.0), w), v[i]), mul(w, div(sub(b[i], acc), diag)));
    }
}

// dst[i] = src[i] for the rows of a sweep in [lo, hi)
template <class T>
__global__ void copy_sweep(int lo, int hi, int start, int step, const T *__restrict__ src, T *__restrict__ dst)
{
    const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < hi && (i - start) % step == 0) dst[i] = src[i];
}

// relaxation.h:33-62 / 394-426, one dependency level
template <class T>
__global__ void gs_level(const int *Ap, const int *Aj, const T *Ax, T *x, const T *b, const int *rows, int count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = rows[t];
    T rsum = from_real<T>(0.0), diag = from_real<T>(0.0);
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
        const int j = Aj[jj];
        if (i == j) diag = Ax[jj];
        else rsum = add(rsum, mul(Ax[jj], x[j]));
    }
    if (nonzero(diag)) x[i] = div(sub(b[i], rsum), diag);
}

// relaxation.h:89-173 (GS: src = dst = x) and 267-360 (JACOBI: src = temp): block row i, its point rows k in
// sweep order.  Point row k's off-diagonal blocks read other block rows only, so its residual is formed
// right before its diagonal step -- the same operations as the reference's two passes.
template <class T, bool JACOBI>
__global__ void bsr_point_level(const int *Ap, const int *Aj, const T *Ax, const T *src, T *x, const T *b,
                                const T *omega, const int *brows, int count, int bs, int reverse)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = brows[t];
    const long B2 = (long)bs * bs;
    long diag_ptr = -1;
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj)
        if (Aj[jj] == i) diag_ptr = jj * B2;
    for (int s = 0; s < bs; ++s) {
        const int k = reverse ? bs - 1 - s : s;
        T r = b[(long)i * bs + k];
        for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
            const int j = Aj[jj];
            if (j == i) continue;
            const T *A = Ax + jj * B2 + (long)k * bs;
            const T *xc = src + (long)j * bs;
            T loc = from_real<T>(0.0);
            for (int c = 0; c < bs; ++c) loc = add(loc, mul(A[c], xc[c]));
            r = sub(r, loc);
        }
        if (diag_ptr < 0) continue;
        T diag = from_real<T>(1.0);
        for (int s2 = 0; s2 < bs; ++s2) {
            const int kk = reverse ? bs - 1 - s2 : s2;
            const T a = Ax[diag_ptr + (long)k * bs + kk];
            if (k == kk) diag = a;
            else r = sub(r, mul(a, src[(long)i * bs + kk]));
        }
        if (nonzero(diag)) {
            const long o = (long)i * bs + k;
            if (JACOBI) {
                const T w = omega[0];
                x[o] = add(mul(sub(from_real<T>(1.0), w), src[o]), div(mul(w, r), diag));
            } else {
                x[o] = div(r, diag);
            }
        }
    }
}

// relaxation.h:661-728 (JACOBI: src = temp) and 755-810 (GS: src = x): rsum = b - sum_{j != i} A_ij src_j,
// then Dinv_i rsum; rsum lives in scratch[i*bs ..]
template <class T, bool JACOBI>
__global__ void block_level(const int *Ap, const int *Aj, const T *Ax, const T *Dinv, const T *src, T *x, const T *b,
                            const T *omega, T *scratch, const int *brows, int count, int bs)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = brows[t];
    const long B2 = (long)bs * bs, o = (long)i * bs;
    T *rsum = scratch + o;
    for (int k = 0; k < bs; ++k) rsum[k] = from_real<T>(0.0);
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
        const int j = Aj[jj];
        if (j == i) continue;
        const T *xc = src + (long)j * bs;
        for (int k = 0; k < bs; ++k) {
            const T *A = Ax + jj * B2 + (long)k * bs;
            T v = from_real<T>(0.0);
            for (int c = 0; c < bs; ++c) v = add(v, mul(A[c], xc[c]));
            rsum[k] = add(rsum[k], v);
        }
    }
    for (int k = 0; k < bs; ++k) rsum[k] = sub(b[o + k], rsum[k]);
    const T *D = Dinv + (long)i * B2;
    for (int m = 0; m < bs; ++m) {
        T v = from_real<T>(0.0);
        for (int c = 0; c < bs; ++c) v = add(v, mul(D[(long)m * bs + c], rsum[c]));
        if (JACOBI) {
            const T w = omega[0];
            x[o + m] = add(mul(sub(from_real<T>(1.0), w), src[o + m]), mul(w, v));
        } else {
            x[o + m] = v;
        }
    }
}

}  // namespace
}  // namespace tk
}  // namespace amg
