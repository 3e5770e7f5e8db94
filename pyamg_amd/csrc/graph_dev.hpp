// The one internal header of the graph stages of the setup (split.hip, classical.hip, transpose.hip, misagg.hip): what
// more than one of them needs on the host side of its drivers -- the checks every host array passes before anything is
// launched on it, a CSR matrix in HBM, the int scan that numbers what a kernel flagged -- and the functions of one
// unit that another one calls.
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

// n + 1 offsets from 0 up that never decrease, every column in [0, n_col), arrays as long as the offsets say (x_size < 0:
// no values).  The last offset is an int, so nnz < 2^31.  Nothing is launched on less.
[[maybe_unused]] int check_csr_arrays(const char *who, int n, int n_col, const int *p, int p_size, const int *j, int j_size, const void *x,
                                      int x_size)
{
    if (n < 0) return bad(who, "negative size");
    if (!p || p_size < n + 1) return bad(who, "offsets shorter than n + 1");
    if (p[0] != 0) return bad(who, "offsets do not start at 0");
    for (int i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) return bad(who, "offsets decrease");
    const int nnz = p[n];
    if (nnz > j_size || (x_size >= 0 && nnz > x_size)) return bad(who, "arrays shorter than the last offset");
    if (nnz > 0 && (!j || (x_size >= 0 && !x))) return bad(who, "null array");
    for (int e = 0; e < nnz; ++e)
        if (j[e] < 0 || j[e] >= n_col) return bad(who, "column index outside the matrix");
    return 0;
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

// A on the device
struct HbmCsr {
    DBuf p, j, x;
    int upload(int n, const int *Ap, const int *Aj, const double *Ax)
    {
        const size_t nnz = (size_t)Ap[n];
        CHK(p.from_host(Ap, sizeof(int) * ((size_t)n + 1)));
        CHK(j.from_host(Aj, sizeof(int) * nnz));
        if (Ax) CHK(x.from_host(Ax, sizeof(double) * nnz));
        return 0;
    }
};

[[maybe_unused]] int last_offset(const int *offsets, int n, long *out)
{
    int v = 0;
    AMG_HIP(hipMemcpy(&v, offsets + n, sizeof(int), hipMemcpyDeviceToHost));
    *out = v;
    return 0;
}

// out[k] = in[0] + ... + in[k - 1] for k < count
[[maybe_unused]] int exclusive_scan(const int *in, int *out, size_t count)
{
    size_t bytes = 0;
    AMG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, count, rocprim::plus<int>(), nullptr));
    DBuf tmp;
    CHK(tmp.alloc(bytes));
    AMG_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, 0, count, rocprim::plus<int>(), nullptr));
    return 0;
}

}  // namespace
}  // namespace amg
