// The one internal header of the graph stages of the setup (split, classical, transpose, misagg, prolong; strength and
// energy for the scan and the checks): what more than one of them needs on the host side of its drivers -- the checks
// every host array passes before anything is launched on it, a CSR matrix in HBM, the scan that numbers what a kernel
// counted and the offsets it leaves -- and the functions of one unit that another one calls.
#pragma once
#include "flat.hpp"

#include <rocprim/device/device_scan.hpp>

#include <string>
#include <vector>

namespace amg {

// what one device transpose did (amg_transpose_last_route)
struct TransposeRoute { int launched = 0, lane_rows = 0, lds_rows = 0, hbm_rows = 0; };

// ---- the functions that cross units; like dev_live (driver.hpp) they stay out of the library's dynamic symbols
// split.hip: the two selection loops on buffers that are already in HBM, and out[0, count) = value
__attribute__((visibility("hidden"))) int mis_rounds_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F,
                                                            int *x, int *flag, int *rounds);
__attribute__((visibility("hidden"))) int cljp_passes_device(int n, long nnz, const int *Sp, const int *Sj, const int *Tp, const int *Tj,
                                                             double *weight, int *splitting, int *passes);
__attribute__((visibility("hidden"))) int fill_int_device(const char *what, long count, int value, int *out);
// transpose.hip: R = P^T in HBM; how: what it did, as the calling thread's amg_transpose_last_route then reports it
__attribute__((visibility("hidden"))) int transpose_device(int n_row, int n_col, long nnz, const int *Pp, const int *Pj, const double *Px,
                                                           DBuf &Rp, DBuf &Rj, DBuf &Rx, TransposeRoute &how);
// misagg.hip: MIS(2) aggregation of a graph that is already in HBM (p, j: n + 1 offsets and columns; y: n weights) into
// freshly allocated agg (n ints, -1: no aggregate) and cpts (the roots, *n_agg of them, ascending); *rounds: rounds of the set
__attribute__((visibility("hidden"))) int mis_aggregation_resident(int n, const int *p, const int *j, const double *y, DBuf &agg,
                                                                   DBuf &cpts, int *n_agg, int *rounds);

namespace {

constexpr int WAVE = 64;
constexpr int F_NODE = 0, C_NODE = 1, U_NODE = 2;       // the states of a splitting

[[maybe_unused]] __device__ __forceinline__ int peek(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
[[maybe_unused]] __device__ __forceinline__ void poke(int *p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

[[maybe_unused]] int bad(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return AMG_EINVAL;
}

// The checks of a CSR matrix in host arrays, in two halves; nothing is launched on less.  n + 1 offsets from 0 up that never
// decrease, within j_size indices and x_size values at per_block an entry (x_size < 0: no values); an int, so nnz < 2^31.
[[maybe_unused]] int check_csr_offsets(const char *who, int n, const int *p, int p_size, long j_size, long x_size, long per_block)
{
    if (n < 0) return bad(who, "negative size");
    if (!p || p_size < n + 1) return bad(who, "offsets shorter than n + 1");
    if (p[0] != 0) return bad(who, "offsets do not start at 0");
    for (int i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return bad(who, "offsets decrease");
    if (p[n] > j_size || (x_size >= 0 && (long)p[n] * per_block > x_size)) return bad(who, "arrays shorter than the last offset");
    return 0;
}

// every column in [0, n_col), under offsets that check_csr_offsets has passed
[[maybe_unused]] int check_csr_columns(const char *who, int n, int n_col, const int *p, const int *j)
{
    const int nnz = p[n];
    if (nnz > 0 && !j) return bad(who, "null array");
    for (int e = 0; e < nnz; ++e)
        if (j[e] < 0 || j[e] >= n_col) return bad(who, "column index outside the matrix");
    return 0;
}

// offsets, then columns, for scalar entries: arrays as long as the offsets say (x_size < 0: no values)
[[maybe_unused]] int check_csr_arrays(const char *who, int n, int n_col, const int *p, int p_size, const int *j, int j_size, const void *x,
                                      int x_size)
{
    CHK(check_csr_offsets(who, n, p, p_size, j_size, x_size, 1));
    if (p[n] > 0 && x_size >= 0 && !x) return bad(who, "null array");
    return check_csr_columns(who, n, n_col, p, j);
}

// the pattern of a graph of n vertices, its arrays as long as its offsets say
[[maybe_unused]] int check_graph(const char *who, int n, const int *p, const int *j)
{
    return check_csr_arrays(who, n, n, p, n + 1, j, 0x7fffffff, nullptr, -1);
}

[[maybe_unused]] int check_splitting(const char *who, int n, const int *splitting, int size)
{
    if (size < n || (n > 0 && !splitting)) return bad(who, "splitting shorter than n");
    for (int i = 0; i < n; ++i)
        if (splitting[i] != 0 && splitting[i] != 1) return bad(who, "splitting holds a value other than 0 and 1");
    return 0;
}

// no column twice in a row of an n x n_col matrix (host arrays that check_csr_arrays has passed)
[[maybe_unused]] int check_unique_columns(const char *who, int n, int n_col, const int *p, const int *j)
{
    std::vector<int> seen((size_t)std::max(n_col, 0), -1);
    for (int i = 0; i < n; ++i)
        for (int e = p[i]; e < p[i + 1]; ++e) {
            if (seen[(size_t)j[e]] == i) return bad(who, "a column is stored twice in a row");
            seen[(size_t)j[e]] = i;
        }
    return 0;
}

// A on the device: 32-bit offsets, columns and (where the caller has any) values
struct HbmCsr {
    DBuf p, j, x;
    // valued: x is allocated even where Ax is null, as it may be for a matrix without entries whose kernels are handed x
    int upload(int n, const int *Ap, const int *Aj, const double *Ax, bool valued = false)
    {
        const size_t nnz = (size_t)Ap[n];
        CHK(p.from_host(Ap, sizeof(int) * ((size_t)n + 1)));
        CHK(j.from_host(Aj, sizeof(int) * nnz));
        if (Ax) CHK(x.from_host(Ax, sizeof(double) * nnz));
        else if (valued) CHK(x.alloc(0));
        return 0;
    }
};

// out[k] = in[0] + ... + in[k - 1] for k < count
template <class T> int exclusive_scan(const T *in, T *out, size_t count)
{
    size_t bytes = 0;
    AMG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), count, rocprim::plus<T>(), nullptr));
    DBuf tmp;
    CHK(tmp.alloc(bytes));
    AMG_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, T(0), count, rocprim::plus<T>(), nullptr));
    return 0;
}

template <class T> int last_offset(const T *offsets, int n, long *out)
{
    T v = 0;
    AMG_HIP(hipMemcpy(&v, offsets + n, sizeof(T), hipMemcpyDeviceToHost));
    *out = v;
    return 0;
}

// The middle of count / scan / fill: n + 1 offsets, allocated here, from the counts a kernel wrote (count[n]: the
// scan's last addend, 0), and their last one read back as *total.  A total outside [0, upper] is refused with
// AMG_ESTATE before anything is allocated or filled by it; upper < 0: the caller has no bound.
template <class T> int offsets_from_counts(const char *who, int n, const T *count, long upper, DBuf &offsets, long *total)
{
    CHK(offsets.alloc(sizeof(T) * ((size_t)n + 1)));
    CHK(exclusive_scan(count, offsets.as<T>(), (size_t)n + 1));
    CHK(last_offset(offsets.as<T>(), n, total));
    if (upper >= 0 && (*total < 0 || *total > upper)) { set_error(std::string(who) + ": the scan left its bound"); return AMG_ESTATE; }
    return 0;
}

// One bit per fact about a CSR operator in HBM, by one lane per row: ROWS_UNSORTED where a row is not strictly
// ascending, VALUE_NOT_FINITE where a value is an infinity or a NaN.  Integer atomics: the result does not depend on order.
constexpr int ROWS_UNSORTED = 1, VALUE_NOT_FINITE = 2;

[[maybe_unused]] __global__ __launch_bounds__(TB) void operator_facts_kernel(int n, const int *Ap, const int *Aj, const double *Ax, int *facts)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    int found = 0;
    if (i < n) {
        const long lo = Ap[i], hi = Ap[i + 1];
        for (long jj = lo; jj < hi; ++jj) {
            if (jj > lo && Aj[jj] <= Aj[jj - 1]) found |= ROWS_UNSORTED;
            if (!isfinite(Ax[jj])) found |= VALUE_NOT_FINITE;
        }
    }
    if (found) atomicOr(facts, found);
}

}  // namespace
}  // namespace amg
