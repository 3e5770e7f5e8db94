// Evolution strength of connection (pyamg/strength.py:433-816, amg_core/evolution_strength.h) on the device.
//
// Part 1: the flat entries incomplete_mat_mult_csr, apply_distance_filter, apply_absolute_distance_filter and
// min_blocks of include/amgcore_hip.h section 1 (float64), each the reference's loop with the same operations in the
// same order: a sum starts from 0.0 and takes its products in index order, multiply and add round separately.
//
// Part 2: the whole measure for one candidate vector as a pipeline in HBM (amg_evolution_strength_device /
// amg_strength_fetch).  The stages are the reference's statements, one or two kernels each; where the reference marks
// entries by writing 0.0 and then calls eliminate_zeros(), so does the pipeline (count per row, scan, fill, order
// kept).  Transposes and row sorts are one radix sort of (row, column) keys: indices are unique, so the order is
// scipy's.  Only row counts and offsets travel to the host between upload and fetch.
#include "graph_dev.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>

using namespace amg;

namespace amg {
// spgemm.hip: C = A * A for a square CSR operand in HBM with scipy's csr_matmat arithmetic and output order; the
// arrays of C are allocated there and handed to the caller's owners
int spgemm_square_device(int n, long nnz, const long *Ap, const int *Aj, const double *Ax, long *Cnnz, DevArr<long> &Cp, DevArr<int> &Cj,
                         DevArr<double> &Cx);
}

namespace {

// row of entry e: the last row whose offset is <= e (empty rows are stepped over)
template <class P>
__device__ __forceinline__ int row_of_entry(const P *Sp, int n_row, long e)
{
    int lo = 0, hi = n_row;                 // invariant: Sp[lo] <= e < Sp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((long)Sp[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- flat kernels
// evolution_strength.h:575-699: one lane per entry of S; consecutive lanes share their row of A and store side by side
template <class P>
__global__ __launch_bounds__(TB) void incomplete_mat_mult_kernel(const P *Ap, const int *Aj, const double *Ax, const P *Bp, const int *Bj,
                                                                 const double *Bx, const P *Sp, const int *Sj, double *Sx, int n_row, long nnz)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    const int row = row_of_entry(Sp, n_row, e);
    const int col = Sj[e];
    double sum = 0.0;
    long a = Ap[row], b = Bp[col];
    const long a_end = Ap[row + 1], b_end = Bp[col + 1];
    while (a < a_end && b < b_end) {
        const int ja = Aj[a], jb = Bj[b];
        if (ja == jb) { sum += Ax[a] * Bx[b]; ++a; ++b; }
        else if (ja < jb) ++a;
        else ++b;
    }
    Sx[e] = sum;
}

// evolution_strength.h:61-83 and :136-167: one lane per row
template <class P>
__global__ __launch_bounds__(TB) void distance_filter_kernel(int n_row, double epsilon, const P *Sp, const int *Sj, double *Sx, int absolute)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_row) return;
    const long lo = Sp[i], hi = Sp[i + 1];
    double threshold = epsilon;
    if (!absolute) {
        double m = DBL_MAX;
        for (long jj = lo; jj < hi; ++jj)
            if (Sj[jj] != i) m = fmin(m, Sx[jj]);
        threshold = epsilon * m;
    }
    for (long jj = lo; jj < hi; ++jj) {
        if (Sj[jj] == i) Sx[jj] = 1.0;
        else if (Sx[jj] >= threshold) Sx[jj] = 0.0;
    }
}

// evolution_strength.h:213-237: one lane per block
__global__ __launch_bounds__(TB) void min_blocks_kernel(int n_blocks, int blocksize, const double *Sx, double *Tx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_blocks) return;
    const double *block = Sx + (long)i * blocksize;
    double m = DBL_MAX;
    for (int j = 0; j < blocksize; ++j) {
        const double v = block[j];
        if (v != 0.0) m = fmin(m, v);
    }
    Tx[i] = m;
}

// a CSR pointer array of an entry's arguments: n + 1 offsets that never decrease, within the arrays they index.
// Not graph_dev.hpp's pair: the amgcore_* entries accept a first offset above 0, as the reference's loops do.
int check_offsets(const char *name, const int *p, int p_size, int n, int j_size, int x_size)
{
    if (!p || n < 0 || p_size < n + 1) { set_error(std::string(name) + ": pointer array shorter than rows + 1"); return AMG_EINVAL; }
    if (p[0] < 0) { set_error(std::string(name) + ": negative offset"); return AMG_EINVAL; }
    for (int i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) { set_error(std::string(name) + ": offsets decrease"); return AMG_EINVAL; }
    if (p[n] > j_size || p[n] > x_size) { set_error(std::string(name) + ": index or value array shorter than the last offset"); return AMG_EINVAL; }
    return 0;
}

int check_columns(const char *name, const int *p, const int *j, int n, int n_col)
{
    for (int e = p[0]; e < p[n]; ++e)
        if (j[e] < 0 || j[e] >= n_col) { set_error(std::string(name) + ": column index outside the matrix"); return AMG_EINVAL; }
    return 0;
}

int filter_entry(int n_row, double epsilon, const int *Sp, int Sp_size, const int *Sj, int Sj_size, double *Sx, int Sx_size, int absolute)
{
    CHK(require_device());
    CHK(check_offsets("apply_distance_filter", Sp, Sp_size, n_row, Sj_size, Sx_size));
    if (n_row == 0 || Sp[n_row] == 0) return 0;
    if (!Sj || !Sx) { set_error("apply_distance_filter: null array"); return AMG_EINVAL; }
    const size_t nnz = (size_t)Sp[n_row];
    DBuf dp, dj, dx;
    CHK(dp.from_host(Sp, sizeof(int) * ((size_t)n_row + 1)));
    CHK(dj.from_host(Sj, sizeof(int) * nnz));
    CHK(dx.from_host(Sx, sizeof(double) * nnz));
    hipLaunchKernelGGL(distance_filter_kernel<int>, grid_for(n_row), dim3(TB), 0, nullptr, n_row, epsilon, dp.i(), dj.i(), dx.d(), absolute);
    LAUNCH_CHECK("distance filter launch");
    AMG_HIP(hipDeviceSynchronize());
    return dx.to_host(Sx, sizeof(double) * nnz);
}

// ---------------------------------------------------------------------------------------------- the pipeline
// A square CSR matrix in HBM with 64-bit offsets in typed arrays, the layout of spgemm.hip's operands and results, which
// are moved in and out of it.  Not graph_dev.hpp's HbmCsr, whose offsets are ints in untyped buffers.
struct DMat {
    int n = 0;
    long nnz = 0;
    DevArr<long> p;
    DevArr<int> j;
    DevArr<double> x;
    void swap(DMat &o) { std::swap(*this, o); }
    int alloc_entries(long count)
    {
        nnz = count;
        AMG_HIP(j.malloc_bytes(sizeof(int) * (size_t)std::max(count, 1L)));
        AMG_HIP(x.malloc_bytes(sizeof(double) * (size_t)std::max(count, 1L)));
        return 0;
    }
};

// offsets (n + 1, a DMat's own: no DBuf, and no bound, for graph_dev.hpp's helper) from per-row counts (count[n] = 0)
int scan_counts(int n, const long *count, long *offsets, long *total)
{
    CHK(exclusive_scan(count, offsets, (size_t)n + 1));
    return last_offset(offsets, n, total);
}

// Every count/fill pair below is ONE device function instantiated twice, so both passes take the same decisions.

// ---- stage (a), (b): M = I - (1/rho) * (Dinv (.)rows A), scipy's canonical csr_minus_csr: 1 - x on the diagonal, 0 - x
// off it, 1.0 where A stores no diagonal, results equal to zero dropped.  Dinv_i = 1/d_i, 1.0 where d_i == 0.
template <bool FILL>
__global__ __launch_bounds__(TB) void jacobi_step_kernel(int n, const long *Ap, const int *Aj, const double *Ax, double inv_rho,
                                                         long *count, const long *Mp, int *Mj, double *Mx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { if (!FILL) count[n] = 0; return; }
    const long lo = Ap[i], hi = Ap[i + 1];
    double d = 0.0;
    for (long jj = lo; jj < hi; ++jj)
        if (Aj[jj] == i) d += Ax[jj];
    const double dinv = d != 0.0 ? 1.0 / d : 1.0;
    long at = FILL ? Mp[i] : 0;
    bool diag_done = false;
    for (long jj = lo; jj < hi; ++jj) {
        const int j = Aj[jj];
        if (!diag_done && j > i) {                  // the identity's entry alone: 1 - 0
            if (FILL) { Mj[at] = i; Mx[at] = 1.0; }
            ++at; diag_done = true;
        }
        const double x = (Ax[jj] * dinv) * inv_rho;
        double v;
        if (j == i) { v = 1.0 - x; diag_done = true; } else v = 0.0 - x;
        if (v != 0.0) {
            if (FILL) { Mj[at] = j; Mx[at] = v; }
            ++at;
        }
    }
    if (!diag_done) {
        if (FILL) { Mj[at] = i; Mx[at] = 1.0; }
        ++at;
    }
    if (!FILL) count[i] = at;
}

// ---- eliminate_zeros: entries equal to zero leave, the others keep their order
template <bool FILL>
__global__ __launch_bounds__(TB) void drop_zeros_kernel(int n, const long *Sp, const int *Sj, const double *Sx, long *count,
                                                        const long *Tp, int *Tj, double *Tx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { if (!FILL) count[n] = 0; return; }
    long at = FILL ? Tp[i] : 0;
    for (long jj = Sp[i]; jj < Sp[i + 1]; ++jj) {
        const double v = Sx[jj];
        if (v != 0.0) {
            if (FILL) { Tj[at] = Sj[jj]; Tx[at] = v; }
            ++at;
        }
    }
    if (!FILL) count[i] = at;
}

// ---- sort keys: (major << 32) | minor of every entry; transposed: major = column
__global__ __launch_bounds__(TB) void entry_keys_kernel(int n, long nnz, const long *Sp, const int *Sj, int transposed, unsigned long long *keys)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    const unsigned long long row = (unsigned)row_of_entry(Sp, n, e), col = (unsigned)Sj[e];
    keys[e] = transposed ? ((col << 32) | row) : ((row << 32) | col);
}

__global__ __launch_bounds__(TB) void major_count_kernel(long nnz, const unsigned long long *keys, int *count32)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    atomicAdd(&count32[(int)(keys[e] >> 32)], 1);
}

__global__ __launch_bounds__(TB) void widen_kernel(int n, const int *in, long *out)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i <= n) out[i] = i < n ? in[i] : 0;
}

__global__ __launch_bounds__(TB) void minor_kernel(long nnz, const unsigned long long *keys, int *minor)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e < nnz) minor[e] = (int)(keys[e] & 0xffffffffULL);
}

// T = S with its entries ordered by (row, column) (transposed = 0: sort_indices) or S^T with sorted rows (1: what
// scipy's .T.tocsr() / .tocsc() give)
int reorder(const DMat &S, int transposed, DMat &T)
{
    const int n = S.n;
    T = DMat();
    T.n = n;
    AMG_HIP(T.p.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
    CHK(T.alloc_entries(S.nnz));
    const long nnz = S.nnz;
    DBuf keys_in, keys_out, cnt32, cnt64, tmp;
    CHK(keys_in.alloc(sizeof(unsigned long long) * (size_t)nnz));
    CHK(keys_out.alloc(sizeof(unsigned long long) * (size_t)nnz));
    CHK(cnt32.zero(sizeof(int) * ((size_t)n + 1)));
    CHK(cnt64.alloc(sizeof(long) * ((size_t)n + 1)));
    if (nnz > 0) {
        hipLaunchKernelGGL(entry_keys_kernel, grid_for(nnz), dim3(TB), 0, nullptr, n, nnz, S.p, S.j, transposed, keys_in.as<unsigned long long>());
        LAUNCH_CHECK("strength: sort keys launch");
        size_t bytes = 0;
        AMG_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(), (double *)S.x, (double *)T.x,
                                          (size_t)nnz, 0u, 64u, nullptr));
        CHK(tmp.alloc(bytes));
        AMG_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, keys_in.as<unsigned long long>(), keys_out.as<unsigned long long>(), (double *)S.x, (double *)T.x,
                                          (size_t)nnz, 0u, 64u, nullptr));
        hipLaunchKernelGGL(major_count_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, keys_out.as<unsigned long long>(), cnt32.as<int>());
        LAUNCH_CHECK("strength: row count launch");
        hipLaunchKernelGGL(minor_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, keys_out.as<unsigned long long>(), T.j);
        LAUNCH_CHECK("strength: column launch");
    }
    hipLaunchKernelGGL(widen_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, cnt32.as<int>(), cnt64.as<long>());
    LAUNCH_CHECK("strength: count widening launch");
    long total = 0;
    CHK(scan_counts(n, cnt64.as<long>(), T.p, &total));
    if (total != nnz) { set_error("strength: reordered matrix lost entries"); return AMG_ESTATE; }
    return 0;
}

// count / scan / fill around a row kernel: KERNEL<false> fills count (n + 1), KERNEL<true> writes T
#define COUNT_SCAN_FILL(KCOUNT, KFILL, MAT, NROWS, what, ...)                                                              \
    do {                                                                                                             \
        DBuf count__;                                                                                                \
        CHK(count__.alloc(sizeof(long) * ((size_t)(NROWS) + 1)));                                                        \
        (MAT) = DMat();                                                                                              \
        (MAT).n = (NROWS);                                                                                                 \
        AMG_HIP((MAT).p.malloc_bytes(sizeof(long) * ((size_t)(NROWS) + 1)));                                         \
        hipLaunchKernelGGL(KCOUNT, grid_for((long)(NROWS) + 1), dim3(TB), 0, nullptr, __VA_ARGS__, count__.as<long>(),   \
                           (const long *)nullptr, (int *)nullptr, (double *)nullptr);                               \
        LAUNCH_CHECK(what " (count)");                                                                               \
        long total__ = 0;                                                                                            \
        CHK(scan_counts((NROWS), count__.as<long>(), (MAT).p, &total__));                                                  \
        CHK((MAT).alloc_entries(total__));                                                                             \
        hipLaunchKernelGGL(KFILL, grid_for((long)(NROWS) + 1), dim3(TB), 0, nullptr, __VA_ARGS__, (long *)nullptr,       \
                           (const long *)(MAT).p, (MAT).j, (MAT).x);                                                       \
        LAUNCH_CHECK(what " (fill)");                                                                                \
    } while (0)

int drop_zeros(DMat &S)
{
    DMat T;
    COUNT_SCAN_FILL(drop_zeros_kernel<false>, drop_zeros_kernel<true>, T, S.n, "strength: eliminate_zeros", S.n, (const long *)S.p,
                    (const int *)S.j, (const double *)S.x);
    S.swap(T);
    return 0;
}

// ---- stage (f): the one-candidate measure, strength.py:690-737, in place.  b zero -> 1; z~_ij = (d_i / b_i) * b_j with d the
// diagonal of Atilde (0 where absent); weak when z~ * z < 0 or |z~ / z| < 1e-4, else |1 - z~ / z|; what is neither
// weak nor exactly zero and lies below sqrt(eps) becomes 1e-4.  Weak entries are written as 0.0 for drop_zeros.
__global__ __launch_bounds__(TB) void measure_kernel(int n, const long *Sp, const int *Sj, double *Sx, const double *b)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long lo = Sp[i], hi = Sp[i + 1];
    double d = 0.0;
    for (long jj = lo; jj < hi; ++jj)
        if (Sj[jj] == i) d += Sx[jj];
    double bi = b[i];
    if (bi == 0.0) bi = 1.0;
    const double r = d / bi;
    for (long jj = lo; jj < hi; ++jj) {
        double bj = b[Sj[jj]];
        if (bj == 0.0) bj = 1.0;
        const double z = Sx[jj];
        const double zt = r * bj;
        const bool angle = (zt * z + 0.0 * 0.0) < 0.0;
        const double ratio = zt / z;
        const bool weak = fabs(ratio) < 1e-4;
        double v = fabs(1.0 - ratio);
        if (weak || angle) v = 0.0;
        if (v != 0.0 && v < 1.4901161193847656e-08) v = 1e-4;
        Sx[jj] = v;
    }
}

// ---- stage (h): 0.5 * (S + T), T = S^T with sorted rows: scipy's canonical csr_plus_csr (a + b, a + 0, 0 + b; sums equal to
// zero dropped), then every stored sum times 0.5
template <bool FILL>
__global__ __launch_bounds__(TB) void symmetrize_kernel(int n, const long *Sp, const int *Sj, const double *Sx, const long *Tp,
                                                        const int *Tj, const double *Tx, long *count, const long *Cp, int *Cj, double *Cx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { if (!FILL) count[n] = 0; return; }
    long a = Sp[i], b = Tp[i];
    const long a_end = Sp[i + 1], b_end = Tp[i + 1];
    long at = FILL ? Cp[i] : 0;
    while (a < a_end || b < b_end) {
        int j;
        double v;
        const int ja = a < a_end ? Sj[a] : 2147483647, jb = b < b_end ? Tj[b] : 2147483647;
        if (ja == jb) { j = ja; v = Sx[a] + Tx[b]; ++a; ++b; }
        else if (ja < jb) { j = ja; v = Sx[a] + 0.0; ++a; }
        else { j = jb; v = 0.0 + Tx[b]; ++b; }
        if (v != 0.0) {
            if (FILL) { Cj[at] = j; Cx[at] = v * 0.5; }
            ++at;
        }
    }
    if (!FILL) count[i] = at;
}

// ---- stage (i): S + (I - diag(S)): d + (1 - d) on the diagonal, 1.0 where S stores none, a + 0 elsewhere; zero results dropped
template <bool FILL>
__global__ __launch_bounds__(TB) void unit_diagonal_kernel(int n, const long *Sp, const int *Sj, const double *Sx, long *count,
                                                           const long *Cp, int *Cj, double *Cx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { if (!FILL) count[n] = 0; return; }
    const long lo = Sp[i], hi = Sp[i + 1];
    double d = 0.0;
    for (long jj = lo; jj < hi; ++jj)
        if (Sj[jj] == i) d += Sx[jj];
    const double one_minus_d = 1.0 - d;
    long at = FILL ? Cp[i] : 0;
    bool diag_done = false;
    for (long jj = lo; jj < hi; ++jj) {
        const int j = Sj[jj];
        if (!diag_done && j > i) {
            const double v = 0.0 + one_minus_d;
            if (v != 0.0) { if (FILL) { Cj[at] = i; Cx[at] = v; } ++at; }
            diag_done = true;
        }
        double v;
        if (j == i) { v = Sx[jj] + one_minus_d; diag_done = true; } else v = Sx[jj] + 0.0;
        if (v != 0.0) { if (FILL) { Cj[at] = j; Cx[at] = v; } ++at; }
    }
    if (!diag_done) {
        const double v = 0.0 + one_minus_d;
        if (v != 0.0) { if (FILL) { Cj[at] = i; Cx[at] = v; } ++at; }
    }
    if (!FILL) count[i] = at;
}

// ---- stages (j), (k): x -> 1/x, then every row times 1 / (its largest magnitude, counted from DBL_MIN up: maximum_row_value,
// ruge_stuben.h:110-130, and scale_rows_by_largest_entry, util/utils.py:1830-1869)
__global__ __launch_bounds__(TB) void invert_scale_kernel(int n, const long *Sp, double *Sx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long lo = Sp[i], hi = Sp[i + 1];
    double m = DBL_MIN;
    for (long jj = lo; jj < hi; ++jj) {
        const double v = 1.0 / Sx[jj];
        Sx[jj] = v;
        m = fmax(m, fabs(v));
    }
    const double s = 1.0 / m;
    for (long jj = lo; jj < hi; ++jj) Sx[jj] = Sx[jj] * s;
}

}   // namespace

struct __attribute__((visibility("hidden"))) amg_strength {
    DMat C;
};

namespace {

int run_pipeline(DMat &A, const double *b_dev, double rho, double epsilon, int k, int symmetrize, DMat &C)
{
    const int n = A.n;
    // (a), (b) one time step, M = I - (1/rho) Dinv A, and (c) Atilde = M^T
    DMat M, At;
    COUNT_SCAN_FILL(jacobi_step_kernel<false>, jacobi_step_kernel<true>, M, n, "strength: Jacobi step", n, (const long *)A.p, (const int *)A.j,
                    (const double *)A.x, 1.0 / rho);
    CHK(reorder(M, 1, At));
    // (d) Atilde^k on the pattern of A
    if (k > 1) {
        int nsquare = 0;
        while ((1 << (nsquare + 1)) <= k) ++nsquare;
        DMat Csc;                                           // Atilde as sorted CSC = its transpose as sorted CSR
        if (nsquare > 1) {
            for (int s = 0; s < nsquare - 1; ++s) {         // Atilde = Atilde * Atilde, scipy's product and order
                DMat P;
                P.n = n;
                CHK(spgemm_square_device(n, At.nnz, At.p, At.j, At.x, &P.nnz, P.p, P.j, P.x));
                At.swap(P);
            }
            CHK(reorder(At, 1, Csc));
            DMat sorted;
            CHK(reorder(At, 0, sorted));
            At.swap(sorted);
        } else {
            Csc.swap(M);                                    // (M^T)^T, already sorted
        }
        M = DMat();
        DMat S;                                             // the mask: A's pattern, values overwritten
        S.n = n;
        AMG_HIP(S.p.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
        AMG_HIP(hipMemcpy(S.p, A.p, sizeof(long) * ((size_t)n + 1), hipMemcpyDeviceToDevice));
        CHK(S.alloc_entries(A.nnz));
        if (A.nnz > 0) {
            AMG_HIP(hipMemcpy(S.j, A.j, sizeof(int) * (size_t)A.nnz, hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(incomplete_mat_mult_kernel<long>, grid_for(A.nnz), dim3(TB), 0, nullptr, (const long *)At.p, (const int *)At.j,
                               (const double *)At.x, (const long *)Csc.p, (const int *)Csc.j, (const double *)Csc.x, (const long *)S.p,
                               (const int *)S.j, S.x, n, A.nnz);
            LAUNCH_CHECK("strength: incomplete product launch");
        }
        // (e) eliminate_zeros
        CHK(drop_zeros(S));
        At.swap(S);
    }
    M = DMat();
    A = DMat();
    // (f) the measure, weak entries dropped
    hipLaunchKernelGGL(measure_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const long *)At.p, (const int *)At.j, At.x, b_dev);
    LAUNCH_CHECK("strength: measure launch");
    CHK(drop_zeros(At));
    // (g) drop tolerance
    if (!std::isinf(epsilon)) {
        hipLaunchKernelGGL(distance_filter_kernel<long>, grid_for(n), dim3(TB), 0, nullptr, n, epsilon, (const long *)At.p, (const int *)At.j, At.x, 0);
        LAUNCH_CHECK("strength: distance filter launch");
        CHK(drop_zeros(At));
    }
    // (h) 0.5 (S + S^T)
    if (symmetrize) {
        DMat T, H;
        CHK(reorder(At, 1, T));
        COUNT_SCAN_FILL(symmetrize_kernel<false>, symmetrize_kernel<true>, H, n, "strength: symmetrisation", n, (const long *)At.p,
                        (const int *)At.j, (const double *)At.x, (const long *)T.p, (const int *)T.j, (const double *)T.x);
        At.swap(H);
    }
    // (i) unit diagonal
    COUNT_SCAN_FILL(unit_diagonal_kernel<false>, unit_diagonal_kernel<true>, C, n, "strength: unit diagonal", n, (const long *)At.p,
                    (const int *)At.j, (const double *)At.x);
    // (j), (k)
    hipLaunchKernelGGL(invert_scale_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const long *)C.p, C.x);
    LAUNCH_CHECK("strength: scaling launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

}   // namespace

extern "C" {

int amgcore_incomplete_mat_mult_csr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[], int Ax_size,
                                        const int Bp[], int Bp_size, const int Bj[], int Bj_size, const double Bx[], int Bx_size,
                                        const int Sp[], int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size, int num_rows)
{
    CHK(require_device());
    CHK(check_offsets("incomplete_mat_mult_csr: A", Ap, Ap_size, num_rows, Aj_size, Ax_size));
    CHK(check_offsets("incomplete_mat_mult_csr: B", Bp, Bp_size, num_rows, Bj_size, Bx_size));
    CHK(check_offsets("incomplete_mat_mult_csr: S", Sp, Sp_size, num_rows, Sj_size, Sx_size));
    if (num_rows == 0 || Sp[num_rows] == 0) return 0;
    if (Sp[0] != 0) { set_error("incomplete_mat_mult_csr: S does not start at offset 0"); return AMG_EINVAL; }
    if (!Sj || !Sx) { set_error("incomplete_mat_mult_csr: null array"); return AMG_EINVAL; }
    CHK(check_columns("incomplete_mat_mult_csr: S", Sp, Sj, num_rows, num_rows));
    const size_t np = (size_t)num_rows + 1, na = (size_t)Ap[num_rows], nb = (size_t)Bp[num_rows], ns = (size_t)Sp[num_rows];
    if ((na && (!Aj || !Ax)) || (nb && (!Bj || !Bx))) { set_error("incomplete_mat_mult_csr: null array"); return AMG_EINVAL; }
    DBuf dAp, dAj, dAx, dBp, dBj, dBx, dSp, dSj, dSx;
    CHK(dAp.from_host(Ap, sizeof(int) * np)); CHK(dAj.from_host(Aj, sizeof(int) * na)); CHK(dAx.from_host(Ax, sizeof(double) * na));
    CHK(dBp.from_host(Bp, sizeof(int) * np)); CHK(dBj.from_host(Bj, sizeof(int) * nb)); CHK(dBx.from_host(Bx, sizeof(double) * nb));
    CHK(dSp.from_host(Sp, sizeof(int) * np)); CHK(dSj.from_host(Sj, sizeof(int) * ns)); CHK(dSx.alloc(sizeof(double) * ns));
    hipLaunchKernelGGL(incomplete_mat_mult_kernel<int>, grid_for((long)ns), dim3(TB), 0, nullptr, (const int *)dAp.i(), (const int *)dAj.i(),
                       (const double *)dAx.d(), (const int *)dBp.i(), (const int *)dBj.i(), (const double *)dBx.d(), (const int *)dSp.i(),
                       (const int *)dSj.i(), dSx.d(), num_rows, (long)ns);
    LAUNCH_CHECK("incomplete_mat_mult_csr launch");
    AMG_HIP(hipDeviceSynchronize());
    return dSx.to_host(Sx, sizeof(double) * ns);
}

int amgcore_apply_distance_filter_f64(int n_row, double epsilon, const int Sp[], int Sp_size, const int Sj[], int Sj_size, double Sx[],
                                      int Sx_size)
{
    return filter_entry(n_row, epsilon, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size, 0);
}

int amgcore_apply_absolute_distance_filter_f64(int n_row, double epsilon, const int Sp[], int Sp_size, const int Sj[], int Sj_size,
                                               double Sx[], int Sx_size)
{
    return filter_entry(n_row, epsilon, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size, 1);
}

int amgcore_min_blocks_f64(int n_blocks, int blocksize, const double Sx[], int Sx_size, double Tx[], int Tx_size)
{
    CHK(require_device());
    if (n_blocks < 0 || blocksize < 0 || (long)n_blocks * blocksize > Sx_size || n_blocks > Tx_size) {
        set_error("min_blocks: arrays shorter than n_blocks * blocksize / n_blocks");
        return AMG_EINVAL;
    }
    if (n_blocks == 0) return 0;
    if (!Tx || (blocksize && !Sx)) { set_error("min_blocks: null array"); return AMG_EINVAL; }
    DBuf dS, dT;
    CHK(dS.from_host(Sx, sizeof(double) * (size_t)n_blocks * (size_t)blocksize));
    CHK(dT.alloc(sizeof(double) * (size_t)n_blocks));
    hipLaunchKernelGGL(min_blocks_kernel, grid_for(n_blocks), dim3(TB), 0, nullptr, n_blocks, blocksize, (const double *)dS.d(), dT.d());
    LAUNCH_CHECK("min_blocks launch");
    AMG_HIP(hipDeviceSynchronize());
    return dT.to_host(Tx, sizeof(double) * (size_t)n_blocks);
}

// The measure of strength.py:433-816 for a real float64 operator and one candidate vector.  A: n x n CSR on the host, rows
// sorted, no duplicates, no stored zeros; b: the candidate (n values); rho: the spectral radius estimate of Dinv A;
// k a power of two.  On return Cp (n + 1 offsets) is filled and *out holds the result for amg_strength_fetch.
// times_ms (or null): [0] upload, [1] the stages.
int amg_evolution_strength_device(int n, const int64_t *Ap, const int *Aj, const double *Ax, const double *b, double rho,
                                  double epsilon, int k, int symmetrize, int64_t *Cp, amg_strength **out, double *times_ms)
{
    if (!out || !Ap || !b || !Cp || n < 0) { set_error("evolution strength: bad arguments"); return AMG_EINVAL; }
    if (k < 1 || (k & (k - 1)) != 0) { set_error("evolution strength: the device pipeline takes k = 1, 2, 4, 8, ..."); return AMG_ENOTIMPL; }
    if (!(epsilon >= 1.0)) { set_error("evolution strength: expected epsilon > 1.0"); return AMG_EINVAL; }
    if (Ap[0] != 0) { set_error("evolution strength: offsets do not start at 0"); return AMG_EINVAL; }
    for (int i = 0; i < n; ++i) {
        if (Ap[i + 1] < Ap[i]) { set_error("evolution strength: offsets decrease"); return AMG_EINVAL; }
        if (Ap[i + 1] > Ap[i] && (!Aj || !Ax)) { set_error("evolution strength: null array"); return AMG_EINVAL; }
        for (int64_t jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
            if (Aj[jj] < 0 || Aj[jj] >= n || (jj > Ap[i] && Aj[jj] <= Aj[jj - 1])) {
                set_error("evolution strength: rows must hold sorted, unique columns inside the matrix");
                return AMG_EINVAL;
            }
            if (Ax[jj] == 0.0) { set_error("evolution strength: stored zeros must be removed first"); return AMG_EINVAL; }
        }
    }
    CHK(require_device());
    LapClock timer;
    DMat A;
    A.n = n;
    const long nnz = (long)Ap[n];
    AMG_HIP(A.p.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
    CHK(A.alloc_entries(nnz));
    AMG_HIP(hipMemcpy(A.p, Ap, sizeof(long) * ((size_t)n + 1), hipMemcpyHostToDevice));
    if (nnz > 0) {
        AMG_HIP(hipMemcpy(A.j, Aj, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
        AMG_HIP(hipMemcpy(A.x, Ax, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
    }
    DBuf bd;
    CHK(bd.from_host(b, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    std::unique_ptr<amg_strength> s(new amg_strength);
    int rc = run_pipeline(A, bd.d(), rho, epsilon, k, symmetrize, s->C);
    if (rc == 0 && hipMemcpy(Cp, s->C.p, sizeof(long) * ((size_t)n + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("evolution strength: offset download failed");
        rc = AMG_ENODEV;
    }
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = timer.lap(); }
    CHK(rc);
    *out = s.release();
    return 0;
}

// columns and values (Cp[n] entries each) to the host; releases the result
int amg_strength_fetch(amg_strength *s, int *Cj, double *Cx)
{
    if (!s) return AMG_EINVAL;
    std::unique_ptr<amg_strength> own(s);
    if (s->C.nnz > 0) {
        if (!Cj || !Cx || hipMemcpy(Cj, s->C.j, sizeof(int) * (size_t)s->C.nnz, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(Cx, s->C.x, sizeof(double) * (size_t)s->C.nnz, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("evolution strength: download failed");
            return AMG_ENODEV;
        }
    }
    return 0;
}

}   // extern "C"
