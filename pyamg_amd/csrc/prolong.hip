// The three smoothed-aggregation stages that had no device route, each as a stage entry of its own
// with upload, kernels and fetch: symmetric strength of connection (amg_core/smoothed_aggregation.h:49-99 with the row
// scaling of pyamg/strength.py), the tentative prolongator (fit_candidates, smoothed_aggregation.h:323-452) and Jacobi
// prolongation smoothing (pyamg/aggregation/smooth.py:67-210).  Every kernel gives one lane a whole row -- or a whole
// aggregate -- and walks it in stored order, so each sum is the host route's sequence of additions; nothing is
// contracted (-ffp-contract=off), square root and division are the correctly rounded ones.  Offsets are widened to 64
// bits inside the kernels; every count fits an int because the sizes are checked before the first launch.  The products
// of the smoothing are spgemm.hip's, the members of an aggregate come from transpose.hip.
// Every stage is a core on buffers already in HBM (*_resident) inside a thin entry: checks, upload, core, copy back.
#include "graph_dev.hpp"
#include "hier.hpp"

#include <memory>
#include <string>

// the columns and values of a stage's result, held for its fetch (hidden, like classical.hip's handles)
struct __attribute__((visibility("hidden"))) amg_prolong {
    long nnz = 0;
    amg::DBuf j, x;
};

// A chain of smoothed-aggregation levels.  It owns the resident operator A (n x n, nnz entries,
// in the order its product left it; `sorted` where that order is ascending in every row) with the candidate B and,
// between amg_sa_chain_level and amg_sa_chain_fetch, the level built from them: S, the aggregates, T, the sorted copy
// of A, P, R, the coarse operator C and the coarse candidate Bc.  The fetch moves C and Bc into A and B and drops the rest.
enum { SA_IDLE = 0, SA_BUILT = 1, SA_REFUSED = 2, SA_STOPPED = 3 };
struct __attribute__((visibility("hidden"))) amg_sa_chain {
    int n = 0, sorted = 0, state = SA_IDLE;
    long nnz = 0;
    amg::HbmCsr A;
    amg::DBuf B;
    double upload_ms = 0.0;         // of A_0 and B_0: reported with the first level
    int n_coarse = 0, c_facts = 0;
    long s_nnz = 0, t_nnz = 0, p_nnz = 0, c_nnz = 0;
    amg::HbmCsr S, T, Asorted, P;
    amg::DBuf agg, Bc, Rp, Rj, Rx, Cp, Cj, Cx;
    double times_ms[AMG_SA_CHAIN_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    void drop_level()
    {
        S = amg::HbmCsr{}; T = amg::HbmCsr{}; Asorted = amg::HbmCsr{}; P = amg::HbmCsr{};
        agg.reset(); Bc.reset(); Rp.reset(); Rj.reset(); Rx.reset(); Cp.reset(); Cj.reset(); Cx.reset();
        state = SA_IDLE;
    }
};
// the deleter of "drop the level on the way out": std::unique_ptr<amg_sa_chain, SaLevelDrop>
struct SaLevelDrop {
    void operator()(amg_sa_chain *c) const { c->drop_level(); }
};

namespace amg {
namespace {

// ------------------------------------------------------------------------------------------------ symmetric strength
// The three kernels take the operator's values as they are stored (SQ = false) or squared, a * a in one rounding
// (SQ = true): what the host hands on for a BSR operator with 1 x 1 blocks, the "norms" of its blocks.
template <bool SQ> __device__ __forceinline__ double sym_value(double a) { return SQ ? a * a : a; }

// diags[i] = |sum of the stored diagonal entries of row i, in stored order from zero|
template <bool SQ>
__global__ __launch_bounds__(TB) void sym_diagonal_kernel(int n, const int *Ap, const int *Aj, const double *Ax, double *diags)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj)
        if (Aj[jj] == i) d = d + sym_value<SQ>(Ax[jj]);
    diags[i] = fabs(d);
}

__device__ __forceinline__ bool sym_keeps(int i, int j, double a, double eps, const double *diags)
{
    return j == i || a * a >= eps * diags[j];
}

// count pass: the entries row i keeps; lane n writes the scan's last addend
template <bool SQ>
__global__ __launch_bounds__(TB) void sym_count_kernel(int n, double theta2, const int *Ap, const int *Aj, const double *Ax,
                                                       const double *diags, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0; return; }
    const double eps = theta2 * diags[i];
    int kept = 0;
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj)
        if (sym_keeps(i, Aj[jj], sym_value<SQ>(Ax[jj]), eps, diags)) ++kept;
    count[i] = kept;
}

// fill pass: the magnitudes of the kept entries from Sp[i] on, in stored order, then the row divided by its largest one
// (by 1 where that is 0)
template <bool SQ>
__global__ __launch_bounds__(TB) void sym_fill_kernel(int n, double theta2, const int *Ap, const int *Aj, const double *Ax,
                                                      const double *diags, const int *Sp, int *Sj, double *Sx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const double eps = theta2 * diags[i];
    const long lo = Sp[i], hi = Ap[i + 1];
    long at = lo;
    double m = 0.0;
    for (long jj = Ap[i]; jj < hi; ++jj) {
        const int j = Aj[jj];
        const double a = sym_value<SQ>(Ax[jj]);
        if (!sym_keeps(i, j, a, eps, diags)) continue;
        const double v = fabs(a);
        if (m < v) m = v;
        Sj[at] = j;
        Sx[at] = v;
        ++at;
    }
    if (m == 0.0) m = 1.0;
    for (long e = lo; e < at; ++e) Sx[e] = Sx[e] / m;
}

// out[e] = 1.0 for e < count
__global__ __launch_bounds__(TB) void fill_ones_kernel(long count, double *out)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e < count) out[e] = 1.0;
}

// symmetric strength of A (device, with values) into freshly allocated S: S.p n + 1 offsets; *nnz: entries kept
template <bool SQ> int symmetric_strength_kernels(int n, double theta, const HbmCsr &A, long a_nnz, HbmCsr &S, long *nnz)
{
    const double theta2 = theta * theta;
    const int *p = A.p.i(), *j = A.j.i();
    const double *x = A.x.d();
    DBuf diags, count;
    CHK(diags.alloc(sizeof(double) * (size_t)n));
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(sym_diagonal_kernel<SQ>, grid_for(n), dim3(TB), 0, nullptr, n, p, j, x, diags.d());
    LAUNCH_CHECK("symmetric strength: diagonal launch");
    hipLaunchKernelGGL(sym_count_kernel<SQ>, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, theta2, p, j, x, (const double *)diags.d(),
                       count.i());
    LAUNCH_CHECK("symmetric strength: count launch");
    CHK(offsets_from_counts("symmetric strength", n, count.i(), a_nnz, S.p, nnz));
    CHK(S.j.alloc(sizeof(int) * (size_t)*nnz));
    CHK(S.x.alloc(sizeof(double) * (size_t)*nnz));
    hipLaunchKernelGGL(sym_fill_kernel<SQ>, grid_for(n), dim3(TB), 0, nullptr, n, theta2, p, j, x, (const double *)diags.d(),
                       (const int *)S.p.i(), S.j.i(), S.x.d());
    LAUNCH_CHECK("symmetric strength: fill launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// mode AMG_SA_STRENGTH_CSR: the values as stored; _SQUARED: their squares; _ONES: the pattern of A, in stored order,
// with every value 1.0 (what the host returns for a BSR operator with theta == 0, stored zeros included)
int symmetric_strength_resident(int n, double theta, const HbmCsr &A, long a_nnz, HbmCsr &S, long *nnz, int mode = AMG_SA_STRENGTH_CSR)
{
    if (mode == AMG_SA_STRENGTH_CSR) return symmetric_strength_kernels<false>(n, theta, A, a_nnz, S, nnz);
    if (mode == AMG_SA_STRENGTH_SQUARED) return symmetric_strength_kernels<true>(n, theta, A, a_nnz, S, nnz);
    CHK(S.p.alloc(sizeof(int) * ((size_t)n + 1)));
    CHK(S.j.alloc(sizeof(int) * (size_t)a_nnz));
    CHK(S.x.alloc(sizeof(double) * (size_t)a_nnz));
    AMG_HIP(hipMemcpy(S.p.p, A.p.p, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice));
    if (a_nnz > 0) {                        // (without entries S.j and S.x are the empty buffers just allocated)
        AMG_HIP(hipMemcpy(S.j.p, A.j.p, sizeof(int) * (size_t)a_nnz, hipMemcpyDeviceToDevice));
        hipLaunchKernelGGL(fill_ones_kernel, grid_for(a_nnz), dim3(TB), 0, nullptr, a_nnz, S.x.d());
        LAUNCH_CHECK("symmetric strength: ones launch");
    }
    AMG_HIP(hipDeviceSynchronize());
    *nnz = a_nnz;
    return 0;
}

// ------------------------------------------------------------------------------------------------ tentative prolongator
// node i's K1 x K2 block of B into its block of T (a node has at most one aggregate, so its block is number Tp[i])
__global__ __launch_bounds__(TB) void fit_copy_kernel(int n_fine, int bs, const int *Tp, const double *B, double *Tx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_fine) return;
    if (Tp[i + 1] == Tp[i]) return;
    const double *src = B + (long)i * bs;
    double *dst = Tx + (long)Tp[i] * bs;
    for (int t = 0; t < bs; ++t) dst[t] = src[t];
}

// Modified Gram-Schmidt of one aggregate by one lane, in place on the blocks of its members (Mp, Mj: AggOp^T, the members
// in ascending order): every norm and dot product a sequential sum from zero over the m * K1 rows.
__global__ __launch_bounds__(TB) void fit_mgs_kernel(int n_coarse, int K1, int K2, double tol, const int *Mp, const int *Mj, const int *Tp,
                                                     double *Tx, double *R)
{
    const int a = blockIdx.x * TB + threadIdx.x;
    if (a >= n_coarse) return;
    const long lo = Mp[a], hi = Mp[a + 1];
    const long bs = (long)K1 * K2;
    double *Ra = R + (long)a * K2 * K2;
    for (int bj = 0; bj < K2; ++bj) {
        double norm = 0.0;
        for (long e = lo; e < hi; ++e) {
            const double *q = Tx + (long)Tp[Mj[e]] * bs;
            for (int r = 0; r < K1; ++r) { const double v = q[r * K2 + bj]; norm = norm + v * v; }
        }
        norm = sqrt(norm);
        const double threshold = tol * norm;
        for (int bi = 0; bi < bj; ++bi) {
            double dot = 0.0;
            for (long e = lo; e < hi; ++e) {
                const double *q = Tx + (long)Tp[Mj[e]] * bs;
                for (int r = 0; r < K1; ++r) dot = dot + q[r * K2 + bi] * q[r * K2 + bj];
            }
            for (long e = lo; e < hi; ++e) {
                double *q = Tx + (long)Tp[Mj[e]] * bs;
                for (int r = 0; r < K1; ++r) q[r * K2 + bj] = q[r * K2 + bj] - dot * q[r * K2 + bi];
            }
            Ra[bi * K2 + bj] = dot;
        }
        norm = 0.0;
        for (long e = lo; e < hi; ++e) {
            const double *q = Tx + (long)Tp[Mj[e]] * bs;
            for (int r = 0; r < K1; ++r) { const double v = q[r * K2 + bj]; norm = norm + v * v; }
        }
        norm = sqrt(norm);
        double scale = 0.0;
        if (norm > threshold) { scale = 1.0 / norm; Ra[bj * K2 + bj] = norm; }
        else Ra[bj * K2 + bj] = 0.0;
        for (long e = lo; e < hi; ++e) {
            double *q = Tx + (long)Tp[Mj[e]] * bs;
            for (int r = 0; r < K1; ++r) q[r * K2 + bj] = q[r * K2 + bj] * scale;
        }
    }
}

// The tentative prolongator of AggOp (device: Tp, and Tj with nnz columns, at most one per row) and the candidates B
// (device) into freshly allocated Tx (nnz blocks) and R (zero where an aggregate has no members); AggOp^T is formed here.
int fit_candidates_resident(int n_fine, int n_coarse, int K1, int K2, const int *Tp, const int *Tj, long nnz, const double *B, double tol,
                            DBuf &Tx, DBuf &R)
{
    const size_t bs = (size_t)K1 * (size_t)K2;
    DBuf unused_values, Mp, Mj, Mx;
    CHK(Tx.alloc(sizeof(double) * (size_t)nnz * bs));
    CHK(R.zero(sizeof(double) * (size_t)n_coarse * (size_t)K2 * (size_t)K2));
    CHK(unused_values.zero(sizeof(double) * (size_t)nnz));      // transpose_device moves values too; only Mp and Mj are read
    TransposeRoute how;
    CHK(transpose_device(n_fine, n_coarse, nnz, Tp, Tj, unused_values.d(), Mp, Mj, Mx, how));
    hipLaunchKernelGGL(fit_copy_kernel, grid_for(n_fine), dim3(TB), 0, nullptr, n_fine, (int)bs, Tp, B, Tx.d());
    LAUNCH_CHECK("fit_candidates: copy launch");
    hipLaunchKernelGGL(fit_mgs_kernel, grid_for(n_coarse), dim3(TB), 0, nullptr, n_coarse, K1, K2, tol, (const int *)Mp.i(),
                       (const int *)Mj.i(), Tp, Tx.d(), R.d());
    LAUNCH_CHECK("fit_candidates: Gram-Schmidt launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// ------------------------------------------------------------------------------------------------ Jacobi smoothing
// W = w * (D^-1 S) as the host forms it: (S_ik * dinv_i) * w, two roundings
__global__ __launch_bounds__(TB) void jacobi_weight_kernel(int n, double w, const int *Sp, const double *Sx, const double *dinv, double *Wx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const double d = dinv[i];
    const long hi = Sp[i + 1];
    for (long jj = Sp[i]; jj < hi; ++jj) Wx[jj] = (Sx[jj] * d) * w;
}

// *canonical = 0 where a row's columns do not strictly increase (csr_has_canonical_format)
template <class Off>
__global__ __launch_bounds__(TB) void canonical_kernel(int n, const Off *Ap, const int *Aj, int *canonical)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long hi = Ap[i + 1];
    for (long jj = (long)Ap[i] + 1; jj < hi; ++jj)
        if (!(Aj[jj - 1] < Aj[jj])) { *canonical = 0; return; }
}

// One row of P - X as csr_minus_csr leaves it (scipy's csr_binop_csr, which bsr_minus_bsr calls for 1 x 1 blocks); no
// row of P or of X holds a column twice.  CANON (both operands canonical): the merge of the two sorted rows.  Otherwise
// the general routine's linked list, which comes out in reverse order of first touch: X's columns that P lacks from the
// row's last to its first, then P's from last to first.  An entry of P alone is p - 0, one of X alone 0 - x; results
// equal to zero are dropped.  FILL = false counts (lane n writes the scan's last addend), FILL = true writes from Op[i].
template <bool FILL, bool CANON>
__global__ __launch_bounds__(TB) void jacobi_subtract_kernel(int n, const int *Pp, const int *Pj, const double *Px, const long *Xp,
                                                             const int *Xj, const double *Xx, const int *Op, int *Oj, double *Ox, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (!FILL && i == n) { count[n] = 0; return; }
    if (i >= n) return;
    const long plo = Pp[i], phi = Pp[i + 1], xlo = Xp[i], xhi = Xp[i + 1];
    long at = FILL ? Op[i] : 0;
    int kept = 0;
    auto emit = [&](int j, double v) {
        if (v == 0.0) return;
        if (FILL) { Oj[at] = j; Ox[at] = v; ++at; }
        else ++kept;
    };
    if (CANON) {
        long q = plo, e = xlo;
        while (q < phi && e < xhi) {
            const int pj = Pj[q], xj = Xj[e];
            if (pj == xj) { emit(pj, Px[q] - Xx[e]); ++q; ++e; }
            else if (pj < xj) { emit(pj, Px[q] - 0.0); ++q; }
            else { emit(xj, 0.0 - Xx[e]); ++e; }
        }
        for (; q < phi; ++q) emit(Pj[q], Px[q] - 0.0);
        for (; e < xhi; ++e) emit(Xj[e], 0.0 - Xx[e]);
    } else {
        for (long e = xhi - 1; e >= xlo; --e) {
            const int j = Xj[e];
            bool in_p = false;
            for (long q = plo; q < phi && !in_p; ++q) in_p = Pj[q] == j;
            if (!in_p) emit(j, 0.0 - Xx[e]);
        }
        for (long q = phi - 1; q >= plo; --q) {
            const int j = Pj[q];
            double x = 0.0;
            for (long e = xlo; e < xhi; ++e)
                if (Xj[e] == j) { x = Xx[e]; break; }
            emit(j, Px[q] - x);
        }
    }
    if (!FILL) count[i] = kept;
}

// P <- P - X in HBM: P's three arrays are replaced, *p_nnz updated
int jacobi_subtract_device(int n, HbmCsr &P, long *p_nnz, const long *Xp, const int *Xj, const double *Xx, long x_nnz)
{
    if (*p_nnz + x_nnz >= (1L << 31)) { set_error("jacobi smoothing: the difference may hold 2^31 entries or more"); return AMG_ENOTIMPL; }
    DBuf flag, count;
    HbmCsr O;
    int canonical = 1;
    CHK(flag.from_host(&canonical, sizeof(int)));
    hipLaunchKernelGGL(canonical_kernel<int>, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)P.p.i(), (const int *)P.j.i(), flag.i());
    LAUNCH_CHECK("jacobi smoothing: canonical check of P");
    hipLaunchKernelGGL(canonical_kernel<long>, grid_for(n), dim3(TB), 0, nullptr, n, Xp, Xj, flag.i());
    LAUNCH_CHECK("jacobi smoothing: canonical check of X");
    CHK(flag.to_host(&canonical, sizeof(int)));
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    const int *pp = P.p.i(), *pj = P.j.i();
    const double *px = P.x.d();
    if (canonical)
        hipLaunchKernelGGL((jacobi_subtract_kernel<false, true>), grid_for((long)n + 1), dim3(TB), 0, nullptr, n, pp, pj, px, Xp, Xj, Xx,
                           (const int *)nullptr, (int *)nullptr, (double *)nullptr, count.i());
    else
        hipLaunchKernelGGL((jacobi_subtract_kernel<false, false>), grid_for((long)n + 1), dim3(TB), 0, nullptr, n, pp, pj, px, Xp, Xj, Xx,
                           (const int *)nullptr, (int *)nullptr, (double *)nullptr, count.i());
    LAUNCH_CHECK("jacobi smoothing: count launch");
    long nnz = 0;
    CHK(offsets_from_counts("jacobi smoothing", n, count.i(), *p_nnz + x_nnz, O.p, &nnz));
    CHK(O.j.alloc(sizeof(int) * (size_t)nnz));
    CHK(O.x.alloc(sizeof(double) * (size_t)nnz));
    if (canonical)
        hipLaunchKernelGGL((jacobi_subtract_kernel<true, true>), grid_for(n), dim3(TB), 0, nullptr, n, pp, pj, px, Xp, Xj, Xx,
                           (const int *)O.p.i(), O.j.i(), O.x.d(), (int *)nullptr);
    else
        hipLaunchKernelGGL((jacobi_subtract_kernel<true, false>), grid_for(n), dim3(TB), 0, nullptr, n, pp, pj, px, Xp, Xj, Xx,
                           (const int *)O.p.i(), O.j.i(), O.x.d(), (int *)nullptr);
    LAUNCH_CHECK("jacobi smoothing: fill launch");
    AMG_HIP(hipDeviceSynchronize());
    P = std::move(O);
    *p_nnz = nnz;
    return 0;
}

// Jacobi smoothing in HBM: P (n x n_coarse, *p_nnz entries, no column twice in a row) becomes P - W P, `degree` times,
// W = w * (dinv (.)rows S) on the pattern of S (n x n, s_nnz entries).  P's arrays are replaced, *p_nnz updated.
int jacobi_smoothing_resident(int n, int n_coarse, const HbmCsr &S, long s_nnz, const double *dinv, double w, int degree, HbmCsr &P,
                              long *p_nnz)
{
    DBuf Wx;
    CHK(Wx.alloc(sizeof(double) * (size_t)s_nnz));
    hipLaunchKernelGGL(jacobi_weight_kernel, grid_for(n), dim3(TB), 0, nullptr, n, w, (const int *)S.p.i(), (const double *)S.x.d(), dinv,
                       Wx.d());
    LAUNCH_CHECK("jacobi smoothing: weight launch");
    DevArr<long> Wp64;
    CHK(widen_rowptr_device(n, S.p.i(), Wp64));
    for (int step = 0; step < degree; ++step) {
        DevArr<long> Pp64, Xp;
        DevArr<int> Xj;
        DevArr<double> Xx;
        long x_nnz = 0;
        if (s_nnz > 0 && *p_nnz > 0) {
            CHK(widen_rowptr_device(n, P.p.i(), Pp64));
            const int rc = spgemm_device(n, n, n_coarse, s_nnz, Wp64, S.j.i(), Wx.d(), *p_nnz, Pp64, P.j.i(), P.x.d(), &x_nnz, Xp, Xj, Xx);
            if (rc == AMG_EINVAL) return AMG_ENOTIMPL;      // the product routes' refusal: the caller's host route
            CHK(rc);
        } else {                                            // a product without entries: nothing to launch
            AMG_HIP(Xp.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
            AMG_HIP(hipMemset(Xp.p, 0, sizeof(long) * ((size_t)n + 1)));
        }
        CHK(jacobi_subtract_device(n, P, p_nnz, Xp, Xj, Xx, x_nnz));
    }
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// ------------------------------------------------------------------------------------------------ the chained level
// *symmetric = 0 where a stored (i, j) has no stored (j, i): one lane per row, each entry walks row j
__global__ __launch_bounds__(TB) void pattern_symmetric_kernel(int n, const int *Sp, const int *Sj, int *symmetric)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long hi = Sp[i + 1];
    for (long jj = Sp[i]; jj < hi; ++jj) {
        const int j = Sj[jj];
        if (j == i) continue;
        bool back = false;
        const long jhi = Sp[j + 1];
        for (long e = Sp[j]; e < jhi && !back; ++e) back = Sj[e] == i;
        if (!back) { *symmetric = 0; return; }
    }
}

// AggOp from the aggregate of every vertex: a row holds its aggregate, or nothing where agg[i] is -1.  FILL = false
// counts (lane n writes the scan's last addend), FILL = true writes the column at Tp[i].
template <bool FILL>
__global__ __launch_bounds__(TB) void aggop_kernel(int n, const int *agg, const int *Tp, int *Tj, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (!FILL && i == n) { count[n] = 0; return; }
    if (i >= n) return;
    const int a = agg[i];
    if (!FILL) count[i] = a >= 0 ? 1 : 0;
    else if (a >= 0) Tj[Tp[i]] = a;
}

// The rows of a CSR operator sorted by column, out of place: an entry goes to the position its rank gives it, the number
// of columns of its row below its own.  No column is stored twice, so the ranks of a row are 0 .. length - 1, each once,
// and the result is the one sorted row there is.  A row of at most SORT_LANE_MAX entries is ranked by one lane, a longer
// one by one wave whose lanes take its entries side by side.
constexpr int SORT_LANE_MAX = 32;

__device__ __forceinline__ void sort_place(const int *Aj, const double *Ax, long lo, long hi, long e, int *Oj, double *Ox)
{
    const int j = Aj[e];
    long rank = 0;
    for (long k = lo; k < hi; ++k) rank += Aj[k] < j ? 1 : 0;
    Oj[lo + rank] = j;
    Ox[lo + rank] = Ax[e];
}

__global__ __launch_bounds__(TB) void sort_rows_lane_kernel(int n, const int *Ap, const int *Aj, const double *Ax, int *Oj, double *Ox,
                                                            int *long_rows)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long lo = Ap[i], hi = Ap[i + 1];
    if (hi - lo > SORT_LANE_MAX) { *long_rows = 1; return; }       // left to the wave kernel, which then has to run
    for (long e = lo; e < hi; ++e) sort_place(Aj, Ax, lo, hi, e, Oj, Ox);
}

__global__ __launch_bounds__(TB) void sort_rows_wave_kernel(int n, const int *Ap, const int *Aj, const double *Ax, int *Oj, double *Ox)
{
    const long i = (long)blockIdx.x * (TB / WAVE) + threadIdx.x / WAVE;
    if (i >= n) return;
    const long lo = Ap[i], hi = Ap[i + 1];
    if (hi - lo <= SORT_LANE_MAX) return;
    for (long e = lo + threadIdx.x % WAVE; e < hi; e += WAVE) sort_place(Aj, Ax, lo, hi, e, Oj, Ox);
}

// A (n rows, nnz entries, no column twice in a row) with its rows sorted by column into freshly allocated O
int sort_rows_device(int n, long nnz, const HbmCsr &A, HbmCsr &O)
{
    CHK(O.p.alloc(sizeof(int) * ((size_t)n + 1)));
    CHK(O.j.alloc(sizeof(int) * (size_t)nnz));
    CHK(O.x.alloc(sizeof(double) * (size_t)nnz));
    AMG_HIP(hipMemcpy(O.p.p, A.p.p, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice));
    int long_rows = 0;
    DBuf flag;
    CHK(flag.zero(sizeof(int)));
    hipLaunchKernelGGL(sort_rows_lane_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), O.j.i(), O.x.d(), flag.i());
    LAUNCH_CHECK("row sort: lane launch");
    CHK(flag.to_host(&long_rows, sizeof(int)));
    if (long_rows) {                        // (the lane kernel left at least one row: a wave per row over all of them)
        hipLaunchKernelGGL(sort_rows_wave_kernel, grid_for((long)n * WAVE), dim3(TB), 0, nullptr, n, (const int *)A.p.i(),
                           (const int *)A.j.i(), (const double *)A.x.d(), O.j.i(), O.x.d());
        LAUNCH_CHECK("row sort: wave launch");
    }
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// a copy of `bytes` bytes of src in a freshly allocated dst
int copy_device(const DBuf &src, size_t bytes, DBuf &dst)
{
    CHK(dst.alloc(bytes));
    if (bytes) AMG_HIP(hipMemcpy(dst.p, src.p, bytes, hipMemcpyDeviceToDevice));
    return 0;
}

// the facts (graph_dev.hpp) of an operator in HBM
int operator_facts_device(const char *what, int n, const HbmCsr &A, int *facts)
{
    DBuf found;
    CHK(found.zero(sizeof(int)));
    hipLaunchKernelGGL(operator_facts_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), found.i());
    LAUNCH_CHECK(what);
    AMG_HIP(hipMemcpy(facts, found.p, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int fetch_prolong(const char *who, amg_prolong *h, int *j, double *x, double *times_ms)
{
    if (!h) return AMG_EINVAL;
    std::unique_ptr<amg_prolong> own(h);
    if (h->nnz > 0 && (!j || !x)) return bad(who, "null array");
    LapClock timer;
    if (h->nnz > 0) {
        CHK(h->j.to_host(j, sizeof(int) * (size_t)h->nnz));
        CHK(h->x.to_host(x, sizeof(double) * (size_t)h->nnz));
    }
    if (times_ms) times_ms[2] = timer.lap();
    return 0;
}

}   // namespace
}   // namespace amg

extern "C" {

int amg_symmetric_strength_device(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int *Sp, amg_prolong **out,
                                  double *times_ms)
{
    using namespace amg;
    const char *who = "symmetric strength";
    if (!out || !Sp) return bad(who, "bad arguments");
    *out = nullptr;
    clear_times(times_ms);
    if (!(theta >= 0.0)) return bad(who, "expected a theta that is not negative");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    std::unique_ptr<amg_prolong> h(new amg_prolong);
    if (n == 0) {
        Sp[0] = 0;
        *out = h.release();
        return 0;
    }
    CHK(require_device());
    LapClock timer;
    HbmCsr A, S;
    CHK(A.upload(n, Ap, Aj, Ax, true));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    CHK(symmetric_strength_resident(n, theta, A, Ap[n], S, &h->nnz));
    const double hbm_ms = timer.lap();
    CHK(S.p.to_host(Sp, sizeof(int) * ((size_t)n + 1)));
    h->j = std::move(S.j);
    h->x = std::move(S.x);
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = hbm_ms; }
    *out = h.release();
    return 0;
}

int amg_symmetric_strength_fetch(amg_prolong *h, int *Sj, double *Sx, double *times_ms)
{
    return amg::fetch_prolong("symmetric strength fetch", h, Sj, Sx, times_ms);
}

int amg_fit_candidates_device(int n_fine, int n_coarse, int K1, int K2, const int *Tp, const int *Tj, const double *B, double tol,
                              double *Tx, double *R, double *times_ms)
{
    using namespace amg;
    const char *who = "fit_candidates";
    clear_times(times_ms);
    if (n_coarse < 0 || K1 < 1 || K2 < 1) return bad(who, "bad sizes");
    CHK(check_csr_arrays(who, n_fine, n_coarse, Tp, n_fine + 1, Tj, 0x7fffffff, nullptr, -1));
    for (int i = 0; i < n_fine; ++i)
        if (Tp[i + 1] - Tp[i] > 1) return bad(who, "a node belongs to more than one aggregate");
    const long nnz = n_fine > 0 ? Tp[n_fine] : 0;
    const size_t bs = (size_t)K1 * (size_t)K2;
    const size_t t_count = (size_t)nnz * bs, r_count = (size_t)n_coarse * (size_t)K2 * (size_t)K2, b_count = (size_t)n_fine * bs;
    if ((b_count > 0 && !B) || (t_count > 0 && !Tx) || (r_count > 0 && !R)) return bad(who, "null array");
    if (n_fine == 0 || r_count == 0) return 0;
    CHK(require_device());
    LapClock timer;
    HbmCsr T;
    DBuf dB, dTx, dR;
    CHK(T.upload(n_fine, Tp, Tj, nullptr));
    CHK(dB.from_host(B, sizeof(double) * b_count));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    CHK(fit_candidates_resident(n_fine, n_coarse, K1, K2, T.p.i(), T.j.i(), nnz, dB.d(), tol, dTx, dR));
    const double hbm_ms = timer.lap();
    CHK(dTx.to_host(Tx, sizeof(double) * t_count));
    CHK(dR.to_host(R, sizeof(double) * r_count));
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = hbm_ms; times_ms[2] = timer.lap(); }
    return 0;
}

int amg_jacobi_prolongation_device(int n, int n_coarse, const int *Sp, const int *Sj, const double *Sx, const double *dinv, double w,
                                   int degree, const int *Tp, const int *Tj, const double *Tx, int *Pp, amg_prolong **out, double *times_ms)
{
    using namespace amg;
    const char *who = "jacobi smoothing";
    if (!out || !Pp) return bad(who, "bad arguments");
    *out = nullptr;
    clear_times(times_ms);
    if (n_coarse < 0 || degree < 0) return bad(who, "bad sizes");
    CHK(check_csr_arrays(who, n, n, Sp, n + 1, Sj, 0x7fffffff, Sx, 0x7fffffff));
    CHK(check_csr_arrays(who, n, n_coarse, Tp, n + 1, Tj, 0x7fffffff, Tx, 0x7fffffff));
    if (n > 0 && !dinv) return bad(who, "null array");
    CHK(check_unique_columns(who, n, n_coarse, Tp, Tj));
    std::unique_ptr<amg_prolong> h(new amg_prolong);
    if (n == 0) {
        Pp[0] = 0;
        *out = h.release();
        return 0;
    }
    CHK(require_device());
    LapClock timer;
    HbmCsr S, P;
    DBuf ddinv;
    CHK(S.upload(n, Sp, Sj, Sx, true));
    CHK(ddinv.from_host(dinv, sizeof(double) * (size_t)n));
    CHK(P.upload(n, Tp, Tj, Tx, true));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    h->nnz = Tp[n];
    CHK(jacobi_smoothing_resident(n, n_coarse, S, Sp[n], ddinv.d(), w, degree, P, &h->nnz));
    const double hbm_ms = timer.lap();
    CHK(P.p.to_host(Pp, sizeof(int) * ((size_t)n + 1)));
    h->j = std::move(P.j);
    h->x = std::move(P.x);
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = hbm_ms; }
    *out = h.release();
    return 0;
}

int amg_jacobi_prolongation_fetch(amg_prolong *h, int *Pj, double *Px, double *times_ms)
{
    return amg::fetch_prolong("jacobi smoothing fetch", h, Pj, Px, times_ms);
}

// ---- the chain: A_l, S_l, the aggregates, T_l, P_l, R_l, R_l A_l, A_{l+1} and B_{l+1} stay in HBM from the upload of A_0 on

int amg_sa_chain_begin(int n, const int *Ap, const int *Aj, const double *Ax, const double *B, amg_sa_chain **out)
{
    using namespace amg;
    const char *who = "sa chain";
    if (!out) return bad(who, "bad arguments");
    *out = nullptr;
    if (n <= 0) return bad(who, "an empty operator");
    if (!B) return bad(who, "null array");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    CHK(check_unique_columns(who, n, n, Ap, Aj));       // the row sort and the right-hand operand of R * A both need it
    CHK(require_device());
    LapClock timer;
    std::unique_ptr<amg_sa_chain> c(new amg_sa_chain);
    CHK(c->A.upload(n, Ap, Aj, Ax, true));
    CHK(c->B.from_host(B, sizeof(double) * (size_t)n));
    int facts = 0;
    CHK(operator_facts_device("sa chain: operator facts launch", n, c->A, &facts));
    if (facts & VALUE_NOT_FINITE) { set_error("sa chain: the operator holds a value that is not finite"); return AMG_ENOTIMPL; }
    c->n = n;
    c->nnz = Ap[n];
    c->sorted = (facts & ROWS_UNSORTED) ? 0 : 1;
    c->upload_ms = timer.lap();
    *out = c.release();
    return 0;
}

int amg_sa_chain_level(amg_sa_chain *c, int n_rows, double theta, int strength_mode, const double *y, const double *dinv, double w, int degree,
                       const double *B, double tol, long *sizes, int *flags, int *rounds, double *times_ms)
{
    using namespace amg;
    const char *who = "sa chain";
    if (!c || !sizes || !flags || !y || !dinv) return bad(who, "bad arguments");
    if (c->n <= 0) return bad(who, "no resident operator");
    if (n_rows != c->n) return bad(who, "the caller's size is not the resident operator's");       // y, dinv and B are read by it
    if (!(theta >= 0.0)) return bad(who, "expected a theta that is not negative");
    if (strength_mode < AMG_SA_STRENGTH_CSR || strength_mode > AMG_SA_STRENGTH_ONES || degree < 0) return bad(who, "bad options");
    if (c->state != SA_IDLE) { set_error("sa chain: the level built last has not been fetched"); return AMG_ESTATE; }
    // The resident operator is not checked again.  A_0 passed begin's checks; a later one is a product of spgemm.hip,
    // which stores one entry per column, and its row order and finiteness came with the product's facts.
    const int n = c->n;
    std::fill(sizes, sizes + 5, 0L);
    std::fill(flags, flags + AMG_SA_CHAIN_FLAG_FIELDS, 0);
    if (rounds) *rounds = 0;
    LapClock timer;
    DBuf dy, ddinv, newB;
    CHK(dy.from_host(y, sizeof(double) * (size_t)n));
    CHK(ddinv.from_host(dinv, sizeof(double) * (size_t)n));
    if (B) CHK(newB.from_host(B, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    // an early return leaves the chain without a level, its resident operator and candidate as they were
    std::unique_ptr<amg_sa_chain, SaLevelDrop> drop(c);
    const double *dB = B ? newB.d() : c->B.d();
    std::fill(c->times_ms, c->times_ms + AMG_SA_CHAIN_STAGES, 0.0);
    c->times_ms[0] = c->upload_ms + timer.lap();
    c->s_nnz = c->t_nnz = c->p_nnz = c->c_nnz = 0;
    c->n_coarse = 0;
    c->c_facts = 0;

    // 1. strength, on the operator in the order its product left it
    CHK(symmetric_strength_resident(n, theta, c->A, c->nnz, c->S, &c->s_nnz, strength_mode));
    c->times_ms[1] = timer.lap();

    // 2. - 4. the pattern of S is symmetric; MIS(2) aggregation; AggOp
    int symmetric = 1, done = 0;
    {
        DBuf flag;
        CHK(flag.from_host(&symmetric, sizeof(int)));
        hipLaunchKernelGGL(pattern_symmetric_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)c->S.p.i(), (const int *)c->S.j.i(),
                           flag.i());
        LAUNCH_CHECK("sa chain: symmetry launch");
        CHK(flag.to_host(&symmetric, sizeof(int)));
    }
    flags[2] = symmetric;
    if (!symmetric) return bad(who, "expected a structurally symmetric pattern");
    DBuf cpts;
    CHK(mis_aggregation_resident(n, c->S.p.i(), c->S.j.i(), dy.d(), c->agg, cpts, &c->n_coarse, &done));
    if (rounds) *rounds = done;
    sizes[0] = c->s_nnz;
    auto stopped = [&](int why) {
        flags[3] = why;
        if (B) c->B = std::move(newB);
        c->upload_ms = 0.0;
        if (times_ms) std::copy(c->times_ms, c->times_ms + AMG_SA_CHAIN_STAGES - 1, times_ms);
        c->state = SA_STOPPED;
        drop.release();
        return 0;
    };
    if (c->n_coarse == 0) { c->times_ms[2] = timer.lap(); return stopped(AMG_SA_NO_AGGREGATE); }
    {
        DBuf count;
        CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
        hipLaunchKernelGGL(aggop_kernel<false>, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, (const int *)c->agg.i(), (const int *)nullptr,
                           (int *)nullptr, count.i());
        LAUNCH_CHECK("sa chain: AggOp count launch");
        CHK(offsets_from_counts(who, n, count.i(), n, c->T.p, &c->t_nnz));
        CHK(c->T.j.alloc(sizeof(int) * (size_t)c->t_nnz));
        hipLaunchKernelGGL(aggop_kernel<true>, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)c->agg.i(), (const int *)c->T.p.i(),
                           c->T.j.i(), (int *)nullptr);
        LAUNCH_CHECK("sa chain: AggOp fill launch");
    }
    c->times_ms[2] = timer.lap();

    // 5. the tentative prolongator and the coarse candidate
    CHK(fit_candidates_resident(n, c->n_coarse, 1, 1, c->T.p.i(), c->T.j.i(), c->t_nnz, dB, tol, c->T.x, c->Bc));
    c->times_ms[3] = timer.lap();

    // 6. everything after the strength sees sorted rows (the host sorts its copy where it takes the diagonal)
    if (!c->sorted) CHK(sort_rows_device(n, c->nnz, c->A, c->Asorted));
    const HbmCsr &As = c->sorted ? c->A : c->Asorted;
    if (!c->sorted) c->times_ms[4] = timer.lap();        // (exactly 0 where the facts said the rows are sorted)

    // 7. P = T, then the Jacobi steps
    const size_t tbytes = sizeof(int) * (size_t)c->t_nnz;
    CHK(copy_device(c->T.p, sizeof(int) * ((size_t)n + 1), c->P.p));
    CHK(copy_device(c->T.j, tbytes, c->P.j));
    CHK(copy_device(c->T.x, sizeof(double) * (size_t)c->t_nnz, c->P.x));
    c->p_nnz = c->t_nnz;
    sizes[1] = c->t_nnz;
    sizes[4] = c->n_coarse;
    {
        const int rc = jacobi_smoothing_resident(n, c->n_coarse, As, c->nnz, ddinv.d(), w, degree, c->P, &c->p_nnz);
        c->times_ms[5] = timer.lap();
        if (rc == AMG_ENOTIMPL) return stopped(AMG_SA_SMOOTHING_REFUSED);
        CHK(rc);
    }

    // 8. R = P^T
    TransposeRoute how;
    CHK(transpose_device(n, c->n_coarse, c->p_nnz, c->P.p.i(), c->P.j.i(), c->P.x.d(), c->Rp, c->Rj, c->Rx, how));
    c->times_ms[6] = timer.lap();

    // 9. A_c = (R * A) * P by the routes of spgemm.hip; R * A goes when the second product has run
    int tables[2] = {0, 0};
    int rc = 0;
    {
        DevArr<long> Ap64, Rp64, Pp64, RAp, Cp64;
        DevArr<int> RAj, Cj;
        DevArr<double> RAx, Cx;
        long ra_nnz = 0;
        int route[AMG_SPGEMM_ROUTE_FIELDS];
        CHK(widen_rowptr_device(n, As.p.i(), Ap64));
        CHK(widen_rowptr_device(c->n_coarse, c->Rp.i(), Rp64));
        CHK(widen_rowptr_device(n, c->P.p.i(), Pp64));
        rc = spgemm_device(c->n_coarse, n, n, c->p_nnz, Rp64, c->Rj.i(), c->Rx.d(), c->nnz, Ap64, As.j.i(), As.x.d(), &ra_nnz, RAp, RAj, RAx);
        amg_spgemm_last_route(route, AMG_SPGEMM_ROUTE_FIELDS);
        tables[0] = route[3];
        if (rc == 0) {
            rc = spgemm_device(c->n_coarse, n, c->n_coarse, ra_nnz, RAp, RAj, RAx, c->p_nnz, Pp64, c->P.j.i(), c->P.x.d(), &c->c_nnz, Cp64, Cj,
                               Cx);
            amg_spgemm_last_route(route, AMG_SPGEMM_ROUTE_FIELDS);
            tables[1] = route[3];
        }
        if (rc != 0 && rc != AMG_EINVAL) return rc;
        if (rc == 0) {
            CHK(c->Cp.alloc(sizeof(int) * ((size_t)c->n_coarse + 1)));
            CHK(narrow_rowptr_device(c->n_coarse, c->c_nnz, Cp64, c->Cp.i()));
            static_cast<DevArr<void> &>(c->Cj) = DevArr<void>(std::move(Cj));
            static_cast<DevArr<void> &>(c->Cx) = DevArr<void>(std::move(Cx));
        }
    }
    // 10. the row order and the finiteness of A_c in one pass over it, where it lies
    if (rc == 0) {
        DBuf facts;
        CHK(facts.zero(sizeof(int)));
        hipLaunchKernelGGL(operator_facts_kernel, grid_for(c->n_coarse), dim3(TB), 0, nullptr, c->n_coarse, (const int *)c->Cp.i(),
                           (const int *)c->Cj.i(), (const double *)c->Cx.d(), facts.i());
        LAUNCH_CHECK("sa chain: operator facts launch");
        AMG_HIP(hipMemcpy(&c->c_facts, facts.p, sizeof(int), hipMemcpyDeviceToHost));
    } else {
        c->c_nnz = 0;
    }
    c->times_ms[7] = timer.lap();

    sizes[2] = c->p_nnz;
    sizes[3] = c->c_nnz;
    flags[0] = rc == 0 && !(c->c_facts & ROWS_UNSORTED);
    flags[1] = rc == 0 && !(c->c_facts & VALUE_NOT_FINITE);
    flags[4] = tables[0];
    flags[5] = tables[1];
    flags[6] = how.launched; flags[7] = how.lane_rows; flags[8] = how.lds_rows; flags[9] = how.hbm_rows;
    if (B) c->B = std::move(newB);
    c->upload_ms = 0.0;
    if (times_ms) std::copy(c->times_ms, c->times_ms + AMG_SA_CHAIN_STAGES - 1, times_ms);
    c->state = rc == 0 ? SA_BUILT : SA_REFUSED;
    drop.release();
    return rc == 0 ? 0 : AMG_CHAIN_PRODUCT_REFUSED;
}

int amg_sa_chain_fetch(amg_sa_chain *c, int *Pp, int *Pj, double *Px, int *Rp, int *Rj, double *Rx, int *Cp, int *Cj, double *Cx,
                       double *Bc, int *Sp, int *Sj, double *Sx, int *agg, double *Tx, double *times_ms)
{
    using namespace amg;
    const char *who = "sa chain fetch";
    if (!c) return AMG_EINVAL;
    if (c->state == SA_IDLE) { set_error("sa chain fetch: no level has been built"); return AMG_ESTATE; }
    // the level's buffers go whatever happens below; A_c becomes the resident operator only after a complete fetch
    std::unique_ptr<amg_sa_chain, SaLevelDrop> drop(c);
    const int n = c->n;
    // whole: the level is built and its caller takes R and A_c; a caller that finishes a built level on the host (Rp or Cp
    // NULL) is treated like a refused product, and the chain ends
    const bool whole = c->state == SA_BUILT && Rp && Cp, stopped = c->state == SA_STOPPED;
    if (stopped && !Sp) return bad(who, "null array");
    if (!stopped && (!Pp || !Bc || (c->p_nnz > 0 && (!Pj || !Px)))) return bad(who, "null array");
    if (whole && ((c->p_nnz > 0 && (!Rj || !Rx)) || (c->c_nnz > 0 && (!Cj || !Cx)))) return bad(who, "null array");
    if (Sp && c->s_nnz > 0 && (!Sj || !Sx)) return bad(who, "null array");
    LapClock timer;
    if (Sp) {
        CHK(c->S.p.to_host(Sp, sizeof(int) * ((size_t)n + 1)));
        CHK(c->S.j.to_host(Sj, sizeof(int) * (size_t)c->s_nnz));
        CHK(c->S.x.to_host(Sx, sizeof(double) * (size_t)c->s_nnz));
    }
    if (!stopped) {
        if (agg) CHK(c->agg.to_host(agg, sizeof(int) * (size_t)n));
        if (Tx) CHK(c->T.x.to_host(Tx, sizeof(double) * (size_t)c->t_nnz));
        CHK(c->P.p.to_host(Pp, sizeof(int) * ((size_t)n + 1)));
        CHK(c->P.j.to_host(Pj, sizeof(int) * (size_t)c->p_nnz));
        CHK(c->P.x.to_host(Px, sizeof(double) * (size_t)c->p_nnz));
        CHK(c->Bc.to_host(Bc, sizeof(double) * (size_t)c->n_coarse));
    }
    if (whole) {
        const size_t cbytes = sizeof(int) * ((size_t)c->n_coarse + 1);
        CHK(c->Rp.to_host(Rp, cbytes));
        CHK(c->Rj.to_host(Rj, sizeof(int) * (size_t)c->p_nnz));
        CHK(c->Rx.to_host(Rx, sizeof(double) * (size_t)c->p_nnz));
        CHK(c->Cp.to_host(Cp, cbytes));
        CHK(c->Cj.to_host(Cj, sizeof(int) * (size_t)c->c_nnz));
        CHK(c->Cx.to_host(Cx, sizeof(double) * (size_t)c->c_nnz));
        c->A.p = std::move(c->Cp); c->A.j = std::move(c->Cj); c->A.x = std::move(c->Cx);
        c->B = std::move(c->Bc);
        c->n = c->n_coarse;
        c->nnz = c->c_nnz;
        c->sorted = (c->c_facts & ROWS_UNSORTED) ? 0 : 1;
    } else {                                // the level did not reach its coarse operator: the chain ends here
        c->A = HbmCsr{};
        c->B.reset();
        c->n = 0;
        c->nnz = 0;
    }
    if (times_ms) {
        std::copy(c->times_ms, c->times_ms + AMG_SA_CHAIN_STAGES - 1, times_ms);
        times_ms[AMG_SA_CHAIN_STAGES - 1] = timer.lap();
    }
    return 0;
}

void amg_sa_chain_free(amg_sa_chain *c) { delete c; }

}   // extern "C"
