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

namespace amg {
namespace {

// ------------------------------------------------------------------------------------------------ symmetric strength
// diags[i] = |sum of the stored diagonal entries of row i, in stored order from zero|
__global__ __launch_bounds__(TB) void sym_diagonal_kernel(int n, const int *Ap, const int *Aj, const double *Ax, double *diags)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj)
        if (Aj[jj] == i) d = d + Ax[jj];
    diags[i] = fabs(d);
}

__device__ __forceinline__ bool sym_keeps(int i, int j, double a, double eps, const double *diags)
{
    return j == i || a * a >= eps * diags[j];
}

// count pass: the entries row i keeps; lane n writes the scan's last addend
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
        if (sym_keeps(i, Aj[jj], Ax[jj], eps, diags)) ++kept;
    count[i] = kept;
}

// fill pass: the magnitudes of the kept entries from Sp[i] on, in stored order, then the row divided by its largest one
// (by 1 where that is 0)
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
        const double a = Ax[jj];
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

// symmetric strength of A (device, with values) into freshly allocated S: S.p n + 1 offsets; *nnz: entries kept
int symmetric_strength_resident(int n, double theta, const HbmCsr &A, long a_nnz, HbmCsr &S, long *nnz)
{
    const double theta2 = theta * theta;
    const int *p = A.p.i(), *j = A.j.i();
    const double *x = A.x.d();
    DBuf diags, count;
    CHK(diags.alloc(sizeof(double) * (size_t)n));
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(sym_diagonal_kernel, grid_for(n), dim3(TB), 0, nullptr, n, p, j, x, diags.d());
    LAUNCH_CHECK("symmetric strength: diagonal launch");
    hipLaunchKernelGGL(sym_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, theta2, p, j, x, (const double *)diags.d(), count.i());
    LAUNCH_CHECK("symmetric strength: count launch");
    CHK(offsets_from_counts("symmetric strength", n, count.i(), a_nnz, S.p, nnz));
    CHK(S.j.alloc(sizeof(int) * (size_t)*nnz));
    CHK(S.x.alloc(sizeof(double) * (size_t)*nnz));
    hipLaunchKernelGGL(sym_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, theta2, p, j, x, (const double *)diags.d(), (const int *)S.p.i(),
                       S.j.i(), S.x.d());
    LAUNCH_CHECK("symmetric strength: fill launch");
    AMG_HIP(hipDeviceSynchronize());
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

}   // extern "C"
