// The parallel C/F splittings of the classical setup on the device: Luby's maximal independent set run to completion
// (amg_core/graph.h:90-156 with max_iters == -1, the loop under PMIS and PMISc) and the CLJP selection loop
// (amg_core/ruge_stuben.h:373-478).  Both return the integers of the reference's sequential sweeps (DESIGN.md
// section 8h): every decision below is a function of the state at a kernel boundary, or is one that a stale read can
// only postpone.  State arrays hold one int per vertex; offsets are widened to 64 bits inside the kernels.
// Below them, the stages that turn a splitting into a level: classical strength, direct and extended+i interpolation
//  and the level chained in HBM, which runs the two loops above on buffers its earlier stages
// left there.
#include "graph_dev.hpp"
#include "hier.hpp"

#include <cfloat>
#include <string>

using namespace amg;

namespace {

__device__ __forceinline__ int peek(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void poke(int *p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// ------------------------------------------------------------------------------------------------ Luby's MIS
// Step 1 of a round, one lane per vertex: an active vertex without a C neighbour that no active neighbour beats
// ((y, index) compared, the larger index wins a tie) joins the set.  x is read while other lanes write C into it: a
// neighbour seen as C or still as active blocks the reader either way, because a vertex only joins when it beats
// every active neighbour.  Self loops are stepped over.  Lane 0 clears the round's flag for step 2.
__global__ __launch_bounds__(TB) void mis_select_kernel(int n, const int *Ap, const int *Aj, const double *y, int active, int C,
                                                        int *x, int *still_active)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i == 0) *still_active = 0;
    if (i >= n || peek(&x[i]) != active) return;
    const double yi = y[i];
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj) {
        const int j = Aj[jj];
        if (j == i) continue;
        const int xj = peek(&x[j]);
        if (xj == C) return;
        if (xj == active) {
            const double yj = y[j];
            if (yj > yi || (yj == yi && j > i)) return;
        }
    }
    poke(&x[i], C);
}

// Step 2: an active vertex with a C neighbour becomes F (only then: C entries do not change during this kernel); a
// vertex that stays active asks for another round.
__global__ __launch_bounds__(TB) void mis_retire_kernel(int n, const int *Ap, const int *Aj, int active, int C, int F, int *x,
                                                        int *still_active)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n || peek(&x[i]) != active) return;
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj)
        if (peek(&x[Aj[jj]]) == C) { poke(&x[i], F); return; }
    *still_active = 1;
}

// ------------------------------------------------------------------------------------------------ CLJP
constexpr int F_NODE = 0, C_NODE = 1, U_NODE = 2;

// row of entry e: the last row whose offset is <= e (empty rows are stepped over)
__global__ __launch_bounds__(TB) void entry_rows_kernel(int n, long nnz, const int *Sp, int *Srow)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    int lo = 0, hi = n;                     // invariant: Sp[lo] <= e < Sp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((long)Sp[mid] <= e) lo = mid; else hi = mid;
    }
    Srow[e] = lo;
}

// The pass's independent set D against the state the pass starts from: an undecided vertex that no undecided
// neighbour, along S or along T, outweighs.  Equal weights do not exclude each other.  One lane per vertex.
__global__ __launch_bounds__(TB) void cljp_select_kernel(int n, const int *Sp, const int *Sj, const int *Tp, const int *Tj,
                                                         const double *weight, const int *splitting, int *D, int *has_D, int *unassigned)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i == 0) *unassigned = 0;
    if (i >= n) return;
    has_D[i] = 0;
    int top = splitting[i] == U_NODE;
    const double wi = weight[i];
    const long s_hi = Sp[i + 1], t_hi = Tp[i + 1];
    for (long jj = Sp[i]; top && jj < s_hi; ++jj) {
        const int j = Sj[jj];
        if (splitting[j] == U_NODE && weight[j] > wi) top = 0;
    }
    for (long jj = Tp[i]; top && jj < t_hi; ++jj) {
        const int j = Tj[jj];
        if (splitting[j] == U_NODE && weight[j] > wi) top = 0;
    }
    D[i] = top;
}

// P5, one lane per edge e = (c, j) of S: when c is in D and j stays undecided, the edge goes and j loses one.  Each
// edge has one lane, so its mark needs no ownership.  The same lane notes that row c of S holds a column in D (for P6).
// "Undecided" is judged as U and not in D: the members of D turn C in the kernel after this one.
__global__ __launch_bounds__(TB) void cljp_p5_kernel(long nnz, const int *Srow, const int *Sj, const int *D, const int *splitting,
                                                     int *mark, int *dec, int *has_D)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    const int c = Srow[e], j = Sj[e];
    if (D[j]) has_D[c] = 1;
    if (D[c] && !D[j] && splitting[j] == U_NODE && mark[e]) {
        mark[e] = 0;
        atomicAdd(&dec[j], 1);
    }
}

// The decrements of one step, one lane per vertex: weight[i]-- once per lost edge, each on a weight >= 1 and so exact;
// below 1 the vertex becomes F and the rest of its count no longer matters.  A vertex nobody decremented keeps its
// state whatever its weight.  MARK_C: the members of D become C first.  COUNT: the undecided vertices left are summed
// per block and added to *unassigned.
template <bool MARK_C, bool COUNT>
__global__ __launch_bounds__(TB) void cljp_apply_kernel(int n, const int *D, double *weight, int *splitting, int *dec, int *unassigned)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    int open = 0;
    if (i < n) {
        if (MARK_C && D[i]) splitting[i] = C_NODE;
        else if (splitting[i] == U_NODE) {
            const int lost = dec[i];
            open = 1;
            if (lost > 0) {
                double w = weight[i];
                for (int t = 0; t < lost && open; ++t) {
                    w -= 1.0;
                    if (w < 1.0) open = 0;
                }
                weight[i] = w;
                if (!open) splitting[i] = F_NODE;
            }
        }
        dec[i] = 0;
    }
    if (COUNT) {
        const int total = __syncthreads_count(open);
        if (threadIdx.x == 0 && total > 0) atomicAdd(unassigned, total);
    }
}

// P6, one lane per edge e = (j, k) of S that is still marked and whose k is undecided: the edge goes when rows j and
// k of S share a column c in D (j and k both depend on the new C point c).  However many such c there are, the edge
// has this one lane, so it is removed once.  Rows are scanned as stored (no order assumed).
__global__ __launch_bounds__(TB) void cljp_p6_kernel(long nnz, const int *Sp, const int *Srow, const int *Sj, const int *D,
                                                     const int *has_D, const int *splitting, int *mark, int *dec)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz || !mark[e]) return;
    const int j = Srow[e], k = Sj[e];
    if (splitting[k] != U_NODE || !has_D[j] || !has_D[k]) return;
    const long j_hi = Sp[j + 1], k_lo = Sp[k], k_hi = Sp[k + 1];
    for (long aa = Sp[j]; aa < j_hi; ++aa) {
        const int c = Sj[aa];
        if (!D[c]) continue;
        for (long bb = k_lo; bb < k_hi; ++bb)
            if (Sj[bb] == c) {
                mark[e] = 0;
                atomicAdd(&dec[k], 1);
                return;
            }
    }
}

__global__ __launch_bounds__(TB) void fill_int_kernel(long count, int value, int *out)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e < count) out[e] = value;
}

// The two selection loops on buffers that are already in HBM: amg_mis_device and amg_cljp_device below run them on what
// they uploaded, the chained classical level at the end of this file on what its earlier stages left there.
// mis_rounds_device: x: the states, in place; flag: one int of device memory; *rounds: rounds run.
// cljp_passes_device: S holds nnz entries, T = S^T in any row order; weight: the start weights, changed in place;
// splitting: n ints, written (1 = C, 0 = F); *passes: passes run.

int mis_rounds_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F, int *x, int *flag, int *rounds)
{
    int done = 0, again = 1;
    while (again) {
        if (done > n) { set_error("mis: no vertex was decided in a round"); return AMG_ESTATE; }    // a round decides >= 1
        hipLaunchKernelGGL(mis_select_kernel, grid_for(n), dim3(TB), 0, nullptr, n, Ap, Aj, y, active, C, x, flag);
        LAUNCH_CHECK("mis: selection launch");
        hipLaunchKernelGGL(mis_retire_kernel, grid_for(n), dim3(TB), 0, nullptr, n, Ap, Aj, active, C, F, x, flag);
        LAUNCH_CHECK("mis: retirement launch");
        AMG_HIP(hipMemcpy(&again, flag, sizeof(int), hipMemcpyDeviceToHost));
        ++done;
    }
    *rounds = done;
    return 0;
}

int cljp_passes_device(int n, long nnz, const int *Sp, const int *Sj, const int *Tp, const int *Tj, double *weight, int *splitting,
                       int *passes)
{
    const size_t vbytes = sizeof(int) * (size_t)n, ebytes = sizeof(int) * (size_t)nnz;
    DBuf dSrow, dD, dhas, ddec, dmark, dopen;
    CHK(dSrow.alloc(ebytes)); CHK(dmark.alloc(ebytes));
    CHK(dD.alloc(vbytes)); CHK(dhas.alloc(vbytes)); CHK(ddec.alloc(vbytes));
    CHK(dopen.alloc(sizeof(int)));
    hipLaunchKernelGGL(fill_int_kernel, grid_for(n), dim3(TB), 0, nullptr, (long)n, U_NODE, splitting);
    LAUNCH_CHECK("cljp: state launch");
    hipLaunchKernelGGL(fill_int_kernel, grid_for(n), dim3(TB), 0, nullptr, (long)n, 0, ddec.i());
    LAUNCH_CHECK("cljp: count launch");
    if (nnz > 0) {
        hipLaunchKernelGGL(fill_int_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, 1, dmark.i());
        LAUNCH_CHECK("cljp: edge mark launch");
        hipLaunchKernelGGL(entry_rows_kernel, grid_for(nnz), dim3(TB), 0, nullptr, n, nnz, Sp, dSrow.i());
        LAUNCH_CHECK("cljp: edge row launch");
    }
    int done = 0, open = n;
    while (open > 0) {
        if (done >= n) { set_error("cljp: no vertex was selected in a pass"); return AMG_ESTATE; }  // a pass selects >= 1
        hipLaunchKernelGGL(cljp_select_kernel, grid_for(n), dim3(TB), 0, nullptr, n, Sp, Sj, Tp, Tj, (const double *)weight,
                           (const int *)splitting, dD.i(), dhas.i(), dopen.i());
        LAUNCH_CHECK("cljp: selection launch");
        if (nnz > 0) {
            hipLaunchKernelGGL(cljp_p5_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, (const int *)dSrow.i(), Sj, (const int *)dD.i(),
                               (const int *)splitting, dmark.i(), ddec.i(), dhas.i());
            LAUNCH_CHECK("cljp: P5 launch");
        }
        hipLaunchKernelGGL((cljp_apply_kernel<true, false>), grid_for(n), dim3(TB), 0, nullptr, n, (const int *)dD.i(), weight, splitting,
                           ddec.i(), dopen.i());
        LAUNCH_CHECK("cljp: P5 weights launch");
        if (nnz > 0) {
            hipLaunchKernelGGL(cljp_p6_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, Sp, (const int *)dSrow.i(), Sj, (const int *)dD.i(),
                               (const int *)dhas.i(), (const int *)splitting, dmark.i(), ddec.i());
            LAUNCH_CHECK("cljp: P6 launch");
        }
        hipLaunchKernelGGL((cljp_apply_kernel<false, true>), grid_for(n), dim3(TB), 0, nullptr, n, (const int *)dD.i(), weight, splitting,
                           ddec.i(), dopen.i());
        LAUNCH_CHECK("cljp: P6 weights launch");
        AMG_HIP(hipMemcpy(&open, dopen.p, sizeof(int), hipMemcpyDeviceToHost));
        ++done;
    }
    *passes = done;
    return 0;
}

}   // namespace

extern "C" {

int amg_mis_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F, int *x, int *rounds,
                   double *times_ms)
{
    if (n < 0 || (n > 0 && (!y || !x))) { set_error("mis: bad arguments"); return AMG_EINVAL; }
    if (active == C || active == F) { set_error("mis: the active value must differ from C and F"); return AMG_EINVAL; }
    if (rounds) *rounds = 0;
    if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0.0;
    if (n == 0) return 0;
    CHK(check_graph("mis", n, Ap, Aj));
    CHK(require_device());
    LapClock timer;
    const size_t nnz = (size_t)Ap[n];
    DBuf dp, dj, dy, dx, dflag;
    CHK(dp.from_host(Ap, sizeof(int) * ((size_t)n + 1)));
    CHK(dj.from_host(Aj, sizeof(int) * nnz));
    CHK(dy.from_host(y, sizeof(double) * (size_t)n));
    CHK(dx.from_host(x, sizeof(int) * (size_t)n));
    CHK(dflag.alloc(sizeof(int)));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    int done = 0;
    CHK(mis_rounds_device(n, dp.i(), dj.i(), dy.d(), active, C, F, dx.i(), dflag.i(), &done));
    const double rounds_ms = timer.lap();
    CHK(dx.to_host(x, sizeof(int) * (size_t)n));
    if (rounds) *rounds = done;
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = rounds_ms; times_ms[2] = timer.lap(); }
    return 0;
}

int amg_cljp_device(int n, const int *Sp, const int *Sj, const int *Tp, const int *Tj, const double *weight0, int *splitting,
                    int *passes, double *times_ms)
{
    if (n < 0 || (n > 0 && (!weight0 || !splitting))) { set_error("cljp: bad arguments"); return AMG_EINVAL; }
    if (passes) *passes = 0;
    if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0.0;
    if (n == 0) return 0;
    CHK(check_graph("cljp: S", n, Sp, Sj));
    CHK(check_graph("cljp: T", n, Tp, Tj));
    if (Sp[n] != Tp[n]) { set_error("cljp: S and its transpose differ in size"); return AMG_EINVAL; }
    CHK(require_device());
    LapClock timer;
    const long nnz = Sp[n];
    const size_t vbytes = sizeof(int) * (size_t)n, ebytes = sizeof(int) * (size_t)nnz;
    DBuf dSp, dSj, dTp, dTj, dw, dsplit;
    CHK(dSp.from_host(Sp, sizeof(int) * ((size_t)n + 1)));
    CHK(dSj.from_host(Sj, ebytes));
    CHK(dTp.from_host(Tp, sizeof(int) * ((size_t)n + 1)));
    CHK(dTj.from_host(Tj, ebytes));
    CHK(dw.from_host(weight0, sizeof(double) * (size_t)n));
    CHK(dsplit.alloc(vbytes));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    int done = 0;
    CHK(cljp_passes_device(n, nnz, dSp.i(), dSj.i(), dTp.i(), dTj.i(), dw.d(), dsplit.i(), &done));
    const double rounds_ms = timer.lap();
    CHK(dsplit.to_host(splitting, vbytes));
    if (passes) *passes = done;
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = rounds_ms; times_ms[2] = timer.lap(); }
    return 0;
}

}   // extern "C"

// ================================================================================================ classical levels
// Second part of this file: the row-parallel stages of the classical (Ruge-Stuben) setup on the device (DESIGN.md
// section 8i): classical strength of connection (amg_core/ruge_stuben.h:46-93), maximum_row_value (:110-130) and the
// two passes of direct interpolation (:497-595), as flat amg_core entries and chained into one level that stays in HBM from the upload of A
// to the download of the splitting and P (amg_classical_level_device / amg_classical_level_fetch).
//
// Every kernel gives one lane a whole row and walks it in stored order, so each sum is the reference's sequence of
// additions and the compaction (count, exclusive scan, fill) keeps the reference's entry order.  Nothing is contracted
// (-ffp-contract=off), nothing is guarded: infinities and NaNs are stored as they come.  Offsets are widened to 64 bits
// inside the kernels; every count fits an int because nnz < 2^31 is checked before the first launch.
namespace {

enum { KIND_PMIS = 0, KIND_CLJP = 1 };
enum { INTERP_DIRECT = 0, INTERP_EXTENDED_I = 1 };

// std::max(m, |a|) from numeric_limits<double>::min() over a row, the entries of column `skip` left out: a NaN never
// replaces the maximum (m < NaN is false)
__device__ __forceinline__ double row_maximum(const int *Aj, const double *Ax, long lo, long hi, int skip)
{
    double m = DBL_MIN;
    for (long jj = lo; jj < hi; ++jj) {
        if (Aj[jj] == skip) continue;
        const double a = fabs(Ax[jj]);
        if (m < a) m = a;
    }
    return m;
}

// Strength, count pass: threshold[i] = theta * max and the number of entries row i keeps (every stored diagonal entry,
// and the off-diagonals with |a| >= threshold).  Lane n writes the scan's last addend.
__global__ __launch_bounds__(TB) void strength_count_kernel(int n, double theta, const int *Ap, const int *Aj, const double *Ax,
                                                            double *threshold, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0; return; }
    const long lo = Ap[i], hi = Ap[i + 1];
    const double t = theta * row_maximum(Aj, Ax, lo, hi, i);
    int kept = 0;
    for (long jj = lo; jj < hi; ++jj)
        if (Aj[jj] == i || fabs(Ax[jj]) >= t) ++kept;
    threshold[i] = t;
    count[i] = kept;
}

// Strength, fill pass: the kept entries of row i from Sp[i] on, in stored order
__global__ __launch_bounds__(TB) void strength_fill_kernel(int n, const int *Ap, const int *Aj, const double *Ax, const double *threshold,
                                                           const int *Sp, int *Sj, double *Sx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long hi = Ap[i + 1];
    const double t = threshold[i];
    long at = Sp[i];
    for (long jj = Ap[i]; jj < hi; ++jj) {
        const int j = Aj[jj];
        const double a = Ax[jj];
        if (j == i || fabs(a) >= t) { Sj[at] = j; Sx[at] = a; ++at; }
    }
}

__global__ __launch_bounds__(TB) void maximum_row_value_kernel(int n, const int *Ap, const int *Aj, const double *Ax, double *x)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) x[i] = row_maximum(Aj, Ax, Ap[i], Ap[i + 1], -1);
}

// Interpolation, pass 1: a C row holds one entry, an F row its strong C neighbours
__global__ __launch_bounds__(TB) void interpolation_count_kernel(int n, const int *Sp, const int *Sj, const int *splitting, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0; return; }
    int kept = 1;
    if (splitting[i] != C_NODE) {
        kept = 0;
        const long hi = Sp[i + 1];
        for (long jj = Sp[i]; jj < hi; ++jj) {
            const int j = Sj[jj];
            if (splitting[j] == C_NODE && j != i) ++kept;
        }
    }
    count[i] = kept;
}

// Interpolation, pass 2 (:533-595).  coarse[j]: the exclusive scan of splitting, the coarse number of C point j.
// step: +1 walks row i of S as stored, -1 from its last entry to its first (the S the caller would have handed in with
// every row reversed); A's rows are always walked as stored.
__global__ __launch_bounds__(TB) void interpolation_fill_kernel(int n, const int *Ap, const int *Aj, const double *Ax, const int *Sp,
                                                                const int *Sj, const double *Sx, const int *splitting, const int *coarse,
                                                                const int *Bp, int *Bj, double *Bx, int step)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    long at = Bp[i];
    if (splitting[i] == C_NODE) {
        Bj[at] = coarse[i];
        Bx[at] = 1.0;
        return;
    }
    const long s_len = (long)Sp[i + 1] - Sp[i], s_first = step > 0 ? Sp[i] : (long)Sp[i + 1] - 1, a_hi = Ap[i + 1];
    double sum_strong_pos = 0.0, sum_strong_neg = 0.0;
    for (long k = 0, jj = s_first; k < s_len; ++k, jj += step) {
        const int j = Sj[jj];
        if (splitting[j] == C_NODE && j != i) {
            const double s = Sx[jj];
            if (s < 0) sum_strong_neg += s; else sum_strong_pos += s;
        }
    }
    double sum_all_pos = 0.0, sum_all_neg = 0.0, diag = 0.0;
    for (long jj = Ap[i]; jj < a_hi; ++jj) {
        const double a = Ax[jj];
        if (Aj[jj] == i) diag += a;
        else if (a < 0) sum_all_neg += a;
        else sum_all_pos += a;
    }
    const double alpha = sum_all_neg / sum_strong_neg;
    double beta = sum_all_pos / sum_strong_pos;
    if (sum_strong_pos == 0) { diag += sum_all_pos; beta = 0.0; }
    const double neg_coeff = -alpha / diag, pos_coeff = -beta / diag;
    for (long k = 0, jj = s_first; k < s_len; ++k, jj += step) {
        const int j = Sj[jj];
        if (splitting[j] == C_NODE && j != i) {
            const double s = Sx[jj];
            Bj[at] = coarse[j];
            Bx[at] = s < 0 ? neg_coeff * s : pos_coeff * s;
            ++at;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the chained level
// The strength graph without its diagonal, counted: entries per row of G, and per column the rows that depend on it
__global__ __launch_bounds__(TB) void graph_count_kernel(int n, const int *Sp, const int *Sj, int *count, int *indegree)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0; return; }
    const long hi = Sp[i + 1];
    int kept = 0;
    for (long jj = Sp[i]; jj < hi; ++jj) {
        const int j = Sj[jj];
        if (j != i) { ++kept; atomicAdd(&indegree[j], 1); }
    }
    count[i] = kept;
}

// G's rows in S's order; T's rows in the order the atomics hand out their slots (cursor starts at 0)
__global__ __launch_bounds__(TB) void graph_fill_kernel(int n, const int *Sp, const int *Sj, const int *Gp, int *Gj, const int *Tp,
                                                        int *cursor, int *Tj)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long hi = Sp[i + 1];
    long at = Gp[i];
    for (long jj = Sp[i]; jj < hi; ++jj) {
        const int j = Sj[jj];
        if (j == i) continue;
        Gj[at++] = j;
        Tj[(long)Tp[j] + atomicAdd(&cursor[j], 1)] = i;
    }
}

// PMIS: double(in-degree) + r, one addition.  CLJP: r, then + 1.0 once per dependent.
__global__ __launch_bounds__(TB) void start_weights_kernel(int n, int kind, const int *indegree, const double *r, double *weight)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int k = indegree[i];
    double w;
    if (kind == KIND_PMIS) w = (double)k + r[i];
    else {
        w = r[i];
        for (int t = 0; t < k; ++t) w += 1.0;
    }
    weight[i] = w;
}

// The graph Luby's rounds run on: row i of G followed by row i of T (a neighbour listed twice is only looked at twice)
__global__ __launch_bounds__(TB) void union_offsets_kernel(int n, const int *Gp, const int *Tp, int *Up)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i <= n) Up[i] = Gp[i] + Tp[i];
}

__global__ __launch_bounds__(TB) void union_fill_kernel(int n, const int *Gp, const int *Gj, const int *Tp, const int *Tj, const int *Up,
                                                        int *Uj)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    long at = Up[i];
    for (long jj = Gp[i], hi = Gp[i + 1]; jj < hi; ++jj) Uj[at++] = Gj[jj];
    for (long jj = Tp[i], hi = Tp[i + 1]; jj < hi; ++jj) Uj[at++] = Tj[jj];
}

__global__ __launch_bounds__(TB) void fill_kernel(long count, int value, int *out)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e < count) out[e] = value;
}

// |S| with every row divided by its largest entry (a row whose largest entry is 0 is divided by 1), in place
__global__ __launch_bounds__(TB) void scale_rows_kernel(int n, const int *Sp, double *Sx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long lo = Sp[i], hi = Sp[i + 1];
    double m = 0.0;
    for (long jj = lo; jj < hi; ++jj) {
        const double a = fabs(Sx[jj]);
        if (m < a) m = a;
    }
    if (m == 0.0) m = 1.0;
    for (long jj = lo; jj < hi; ++jj) Sx[jj] = fabs(Sx[jj]) / m;
}

int last_offset(const int *offsets, int n, long *out)
{
    int v = 0;
    AMG_HIP(hipMemcpy(&v, offsets + n, sizeof(int), hipMemcpyDeviceToHost));
    *out = v;
    return 0;
}

int bad(const char *who, const char *what)
{
    set_error(std::string(who) + ": " + what);
    return AMG_EINVAL;
}

// n + 1 offsets from 0 up that never decrease, every column in [0, n_col), arrays as long as the offsets say.  The last
// offset is an int, so nnz < 2^31.
int check_csr_arrays(const char *who, int n, int n_col, const int *p, int p_size, const int *j, int j_size, const void *x, int x_size)
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

int check_splitting(const char *who, int n, const int *splitting, int size)
{
    if (size < n || (n > 0 && !splitting)) return bad(who, "splitting shorter than n");
    for (int i = 0; i < n; ++i)
        if (splitting[i] != 0 && splitting[i] != 1) return bad(who, "splitting holds a value other than 0 and 1");
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

// strength of A (device) into Sp (n + 1 offsets) and freshly allocated Sj, Sx; *nnz: entries kept
int strength_device(int n, double theta, const HbmCsr &A, long a_nnz, DBuf &Sp, DBuf &Sj, DBuf &Sx, long *nnz)
{
    DBuf threshold, count;
    CHK(threshold.alloc(sizeof(double) * (size_t)n));
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    CHK(Sp.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(strength_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, theta, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), threshold.d(), count.i());
    LAUNCH_CHECK("classical strength: count launch");
    CHK(exclusive_scan(count.i(), Sp.i(), (size_t)n + 1));
    CHK(last_offset(Sp.i(), n, nnz));
    if (*nnz < 0 || *nnz > a_nnz) { set_error("classical strength: the scan left the matrix"); return AMG_ESTATE; }
    CHK(Sj.alloc(sizeof(int) * (size_t)*nnz));
    CHK(Sx.alloc(sizeof(double) * (size_t)*nnz));
    hipLaunchKernelGGL(strength_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), (const double *)threshold.d(), (const int *)Sp.i(), Sj.i(), Sx.d());
    LAUNCH_CHECK("classical strength: fill launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// pass 1 and its scan: Bp (n + 1 offsets, allocated here); *nnz: entries of the prolongator
int interpolation_offsets_device(int n, const int *Sp, const int *Sj, const int *splitting, DBuf &Bp, long *nnz)
{
    DBuf count;
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    CHK(Bp.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(interpolation_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, Sp, Sj, splitting, count.i());
    LAUNCH_CHECK("direct interpolation: count launch");
    CHK(exclusive_scan(count.i(), Bp.i(), (size_t)n + 1));
    return last_offset(Bp.i(), n, nnz);
}

// the scan of splitting and pass 2 into Bj, Bx (device, Bp[n] entries each)
int interpolation_fill_device(int n, const HbmCsr &A, const int *Sp, const int *Sj, const double *Sx, const int *splitting, const int *Bp,
                              int *Bj, double *Bx, int step)
{
    DBuf coarse;
    CHK(coarse.alloc(sizeof(int) * (size_t)n));
    if (n > 0) CHK(exclusive_scan(splitting, coarse.i(), (size_t)n));
    hipLaunchKernelGGL(interpolation_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), Sp, Sj, Sx, splitting, (const int *)coarse.i(), Bp, Bj, Bx, step);
    LAUNCH_CHECK("direct interpolation: fill launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// ------------------------------------------------------------------------------------------------ extended+i
// Distance-two interpolation.  A wave owns an F row i.  Its candidates -- row i of S and the rows
// of S of its strong F neighbours, one slot per stored entry, a slot that holds no C point set to NO_POINT -- are
// gathered into LDS (up to EXT_CAP slots) or into the row's segment of a workspace in HBM (more), duplicates struck
// out and the rest ranked into the ascending list C_hat.  Every sum the definition orders is a wave-uniform register
// that takes its addends in lane order, a chunk of 64 stored entries at a time; w lives beside C_hat, one slot per
// member, and a strong F neighbour touches each slot at most once (no duplicate columns), the neighbours one after
// the other.  Lanes of a wave run in lockstep and their LDS and memory operations complete in program order, so a
// wavefront fence and barrier is all that separates a phase that writes the row's slots from one that reads them.
constexpr int WAVE = 64, EXT_ROWS = TB / WAVE, EXT_CAP = 256, NO_POINT = 0x7fffffff;

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// acc + v of every flagged lane, in lane order; the same value in every lane
__device__ __forceinline__ double ordered_add(double acc, double v, bool flag)
{
    unsigned long long mask = __ballot(flag);
    while (mask) {
        acc += __shfl(v, __ffsll((long long)mask) - 1);
        mask &= mask - 1;
    }
    return acc;
}

// the stored entry of column col in entries [lo, hi), 0.0 where there is none; the same value in every lane
__device__ __forceinline__ double wave_lookup(const int *Aj, const double *Ax, long lo, long hi, int col, int lane)
{
    for (long base = lo; base < hi; base += WAVE) {
        const long e = base + lane;
        const bool hit = e < hi && Aj[e] == col;
        const double x = hit ? Ax[e] : 0.0;
        const unsigned long long mask = __ballot(hit);
        if (mask) return __shfl(x, __ffsll((long long)mask) - 1);
    }
    return 0.0;
}

// position of col in the ascending list cs[0, m), -1 where it is not there
__device__ __forceinline__ int list_find(const int *cs, int m, int col)
{
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cs[mid] < col) lo = mid + 1; else hi = mid;
    }
    return (lo < m && cs[lo] == col) ? lo : -1;
}

__device__ __forceinline__ double sign_filtered(double akk, double v) { return ((akk >= 0 && v < 0) || (akk < 0 && v > 0)) ? v : 0.0; }

// The slots of F row i (its bound): |row i of S| + the rows of S of its strong F neighbours.  big[i]: the bound where
// it exceeds EXT_CAP, 0 otherwise; its scan places the workspace segments.
__global__ __launch_bounds__(TB) void extended_bound_kernel(int n, const int *Sp, const int *Sj, const int *splitting, long *big)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    long slots = 0;
    if (i < n && splitting[i] != C_NODE) {
        const long lo = Sp[i], hi = Sp[i + 1];
        slots = hi - lo;
        for (long jj = lo; jj < hi; ++jj) {
            const int k = Sj[jj];
            if (k != i && splitting[k] != C_NODE) slots += (long)Sp[k + 1] - Sp[k];
        }
    }
    big[i] = slots > EXT_CAP ? slots : 0;
}

// gather and strike out: on return cand[0, slots) holds every member of C_hat once and NO_POINT elsewhere.  A slot is
// struck out when an earlier slot holds its value; the first slot of a value is never written, so a reader that meets a
// slot before or after it was struck out decides the same (relaxed accesses, as in Luby's rounds above).
__device__ __forceinline__ long extended_candidates(int i, const int *Sp, const int *Sj, const int *splitting, int *cand, int lane)
{
    const long lo = Sp[i], hi = Sp[i + 1];
    for (long e = lo + lane; e < hi; e += WAVE) {
        const int j = Sj[e];
        cand[e - lo] = (j != i && splitting[j] == C_NODE) ? j : NO_POINT;
    }
    long slots = hi - lo;
    for (long jj = lo; jj < hi; ++jj) {
        const int k = Sj[jj];
        if (k == i || splitting[k] == C_NODE) continue;
        const long klo = Sp[k], khi = Sp[k + 1];
        for (long e = klo + lane; e < khi; e += WAVE) {
            const int c = Sj[e];
            cand[slots + (e - klo)] = splitting[c] == C_NODE ? c : NO_POINT;
        }
        slots += khi - klo;
    }
    wave_sync();
    for (long p = lane; p < slots; p += WAVE) {
        const int v = peek(&cand[p]);
        if (v == NO_POINT) continue;
        for (long q = 0; q < p; ++q)
            if (peek(&cand[q]) == v) { poke(&cand[p], NO_POINT); break; }
    }
    wave_sync();
    return slots;
}

// count pass: |C_hat| of every F row, 1 for a C row, 0 for the scan's last addend; *total: their sum
__global__ __launch_bounds__(TB) void extended_count_kernel(int n, const int *Sp, const int *Sj, const int *splitting, const long *Wp,
                                                            int *wcand, int *count, unsigned long long *total)
{
    __shared__ int lds_cand[EXT_ROWS][EXT_CAP];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long row = (long)blockIdx.x * EXT_ROWS + wave;
    if (row > n) return;
    const int i = (int)row;
    if (i == n || splitting[i] == C_NODE) {
        if (lane == 0) {
            count[i] = i < n ? 1 : 0;
            if (i < n) atomicAdd(total, 1ULL);
        }
        return;
    }
    int *cand = Wp[i + 1] > Wp[i] ? wcand + Wp[i] : lds_cand[wave];
    const long slots = extended_candidates(i, Sp, Sj, splitting, cand, lane);
    int members = 0;
    for (long base = 0; base < slots; base += WAVE) {
        const long p = base + lane;
        members += __popcll(__ballot(p < slots && cand[p] != NO_POINT));
    }
    if (lane == 0) {
        count[i] = members;
        atomicAdd(total, (unsigned long long)members);
    }
}

__global__ __launch_bounds__(TB) void diagonal_kernel(int n, const int *Ap, const int *Aj, const double *Ax, double *diag)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (long jj = Ap[i], hi = Ap[i + 1]; jj < hi; ++jj)
        if (Aj[jj] == i) { d = Ax[jj]; break; }
    diag[i] = d;
}

// fill pass: the row's columns (coarse numbers, ascending) and values from Pp[i] on
__global__ __launch_bounds__(TB) void extended_fill_kernel(int n, const int *Ap, const int *Aj, const double *Ax, const double *diag,
                                                           const int *Sp, const int *Sj, const int *splitting, const int *coarse,
                                                           const long *Wp, int *wcand, int *wlist, double *wsum, const int *Pp, int *Pj,
                                                           double *Px)
{
    __shared__ int lds_cand[EXT_ROWS][EXT_CAP];
    __shared__ int lds_list[EXT_ROWS][EXT_CAP];
    __shared__ double lds_sum[EXT_ROWS][EXT_CAP];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long row = (long)blockIdx.x * EXT_ROWS + wave;
    if (row >= n) return;
    const int i = (int)row;
    const long at = Pp[i];
    if (splitting[i] == C_NODE) {
        if (lane == 0) { Pj[at] = coarse[i]; Px[at] = 1.0; }
        return;
    }
    const int m = Pp[i + 1] - Pp[i];
    if (m == 0) return;
    const bool wide = Wp[i + 1] > Wp[i];
    int *cand = wide ? wcand + Wp[i] : lds_cand[wave];
    int *cs = wide ? wlist + Wp[i] : lds_list[wave];
    double *w = wide ? wsum + Wp[i] : lds_sum[wave];
    const long slots = extended_candidates(i, Sp, Sj, splitting, cand, lane);
    // C_hat: a member's position is the number of members below it
    for (long p = lane; p < slots; p += WAVE) {
        const int v = cand[p];
        if (v == NO_POINT) continue;
        int below = 0;
        for (long q = 0; q < slots; ++q) below += cand[q] < v ? 1 : 0;
        if (below < m) cs[below] = v;
    }
    wave_sync();
    for (int t = lane; t < m; t += WAVE) {
        w[t] = 0.0;
        Pj[at + t] = coarse[cs[t]];
    }
    wave_sync();
    // row i of A: step 1 of the weights, and what is neither interpolatory nor a strong F neighbour goes to D
    const long alo = Ap[i], ahi = Ap[i + 1], slo = Sp[i], shi = Sp[i + 1];
    double D = diag[i];
    for (long base = alo; base < ahi; base += WAVE) {
        const long e = base + lane;
        bool lump = false;
        double v = 0.0;
        if (e < ahi && Aj[e] != i) {
            const int j = Aj[e];
            v = Ax[e];
            if (splitting[j] == C_NODE) {
                const int t = list_find(cs, m, j);
                if (t >= 0) w[t] = v; else lump = true;
            } else {
                lump = true;
                for (long jj = slo; jj < shi; ++jj)
                    if (Sj[jj] == j) { lump = false; break; }
            }
        }
        D = ordered_add(D, v, lump);
    }
    wave_sync();
    // step 2: the strong F neighbours in S's stored order
    for (long jj = slo; jj < shi; ++jj) {
        const int k = Sj[jj];
        if (k == i || splitting[k] == C_NODE) continue;
        const double a = wave_lookup(Aj, Ax, alo, ahi, k, lane), akk = diag[k];
        const long klo = Ap[k], khi = Ap[k + 1];
        double d = 0.0;
        for (long base = klo; base < khi; base += WAVE) {
            const long e = base + lane;
            bool take = false;
            double v = 0.0;
            if (e < khi) {
                const int l = Aj[e];
                v = Ax[e];
                take = sign_filtered(akk, v) != 0.0 && (l == i || (splitting[l] == C_NODE && list_find(cs, m, l) >= 0));
            }
            d = ordered_add(d, v, take);
        }
        if (d == 0.0) { D += a; continue; }
        for (long base = klo; base < khi; base += WAVE) {
            const long e = base + lane;
            bool to_D = false;
            double c = 0.0;
            if (e < khi && sign_filtered(akk, Ax[e]) != 0.0) {
                const int l = Aj[e];
                c = (a * Ax[e]) / d;
                if (l == i) to_D = true;
                else if (splitting[l] == C_NODE) {
                    const int t = list_find(cs, m, l);
                    if (t >= 0) w[t] += c;
                }
            }
            D = ordered_add(D, c, to_D);
        }
        wave_sync();
    }
    for (int t = lane; t < m; t += WAVE) Px[at + t] = (-w[t]) / D;
}

// Truncation (section 8j): a row of more than q entries, all finite, keeps the q of largest magnitude (ties: the smaller
// column) times sum(all) / sum(kept).  One lane per row; an entry's rank is counted, nothing is sorted or stored.
__device__ __forceinline__ bool truncation_applies(const double *x, int m, int q)
{
    if (m <= q) return false;
    for (int u = 0; u < m; ++u)
        if (!isfinite(x[u])) return false;
    return true;
}

__device__ __forceinline__ bool truncation_keeps(const double *x, int m, int t, int q)
{
    const double mag = fabs(x[t]);
    int rank = 0;
    for (int u = 0; u < m; ++u) {
        const double other = fabs(x[u]);
        rank += (other > mag || (other == mag && u < t)) ? 1 : 0;
    }
    return rank < q;
}

__global__ __launch_bounds__(TB) void truncate_count_kernel(int n, int q, const int *Pp, const double *Px, int *count)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    if (i == n) { count[n] = 0; return; }
    const int m = Pp[i + 1] - Pp[i];
    count[i] = truncation_applies(Px + Pp[i], m, q) ? q : m;
}

__global__ __launch_bounds__(TB) void truncate_fill_kernel(int n, int q, const int *Pp, const int *Pj, const double *Px, const int *Tp,
                                                           int *Tj, double *Tx)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int m = Pp[i + 1] - Pp[i];
    const int *j = Pj + Pp[i];
    const double *x = Px + Pp[i];
    long at = Tp[i];
    if (Tp[i + 1] - Tp[i] == m) {
        for (int t = 0; t < m; ++t, ++at) { Tj[at] = j[t]; Tx[at] = x[t]; }
        return;
    }
    double s_all = 0.0, s_kept = 0.0;
    for (int t = 0; t < m; ++t) s_all += x[t];
    for (int t = 0; t < m; ++t)
        if (truncation_keeps(x, m, t, q)) s_kept += x[t];
    const double scale = s_all / s_kept;
    for (int t = 0; t < m; ++t)
        if (truncation_keeps(x, m, t, q)) {
            Tj[at] = j[t];
            Tx[at] = s_kept != 0.0 ? x[t] * scale : x[t];
            ++at;
        }
}

int exclusive_scan_long(const long *in, long *out, size_t count)
{
    size_t bytes = 0;
    AMG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0L, count, rocprim::plus<long>(), nullptr));
    DBuf tmp;
    CHK(tmp.alloc(bytes));
    AMG_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, 0L, count, rocprim::plus<long>(), nullptr));
    return 0;
}

// no column twice in a row (host arrays that check_csr_arrays has passed)
int check_unique_columns(const char *who, int n, const int *p, const int *j)
{
    std::vector<int> seen((size_t)n, -1);
    for (int i = 0; i < n; ++i)
        for (int e = p[i]; e < p[i + 1]; ++e) {
            if (seen[(size_t)j[e]] == i) return bad(who, "a column is stored twice in a row");
            seen[(size_t)j[e]] = i;
        }
    return 0;
}

// Extended+i interpolation of A on the pattern of S (all on the device) into Pp (n + 1 offsets) and freshly allocated
// Pj, Px, truncated to max_per_row entries per row where that is > 0; *nnz: entries of the prolongator
int extended_interpolation_device(int n, const HbmCsr &A, const int *Sp, const int *Sj, const int *splitting, int max_per_row, DBuf &Pp,
                                  DBuf &Pj, DBuf &Px, long *nnz)
{
    const size_t pbytes = sizeof(int) * ((size_t)n + 1);
    const int wave_blocks = (int)(((long)n + 1 + EXT_ROWS - 1) / EXT_ROWS);
    DBuf big, Wp, count, total, coarse, diag, wcand, wlist, wsum;
    CHK(big.alloc(sizeof(long) * ((size_t)n + 1)));
    CHK(Wp.alloc(sizeof(long) * ((size_t)n + 1)));
    CHK(count.alloc(pbytes));
    CHK(total.zero(sizeof(unsigned long long)));
    CHK(Pp.alloc(pbytes));
    hipLaunchKernelGGL(extended_bound_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, Sp, Sj, splitting, big.as<long>());
    LAUNCH_CHECK("extended interpolation: bound launch");
    CHK(exclusive_scan_long(big.as<long>(), Wp.as<long>(), (size_t)n + 1));
    long wide = 0;
    AMG_HIP(hipMemcpy(&wide, Wp.as<long>() + n, sizeof(long), hipMemcpyDeviceToHost));
    if (wide < 0) { set_error("extended interpolation: the workspace scan went negative"); return AMG_ESTATE; }
    CHK(wcand.alloc(sizeof(int) * (size_t)wide));
    hipLaunchKernelGGL(extended_count_kernel, dim3(wave_blocks), dim3(TB), 0, nullptr, n, Sp, Sj, splitting, (const long *)Wp.as<long>(),
                       wcand.i(), count.i(), total.as<unsigned long long>());
    LAUNCH_CHECK("extended interpolation: count launch");
    unsigned long long entries = 0;
    AMG_HIP(hipMemcpy(&entries, total.p, sizeof(entries), hipMemcpyDeviceToHost));
    if (entries > 0x7fffffffULL) { set_error("extended interpolation: the prolongator has 2^31 entries or more"); return AMG_ENOTIMPL; }
    CHK(exclusive_scan(count.i(), Pp.i(), (size_t)n + 1));
    CHK(last_offset(Pp.i(), n, nnz));
    if (*nnz != (long)entries) { set_error("extended interpolation: the scan and the count disagree"); return AMG_ESTATE; }
    CHK(Pj.alloc(sizeof(int) * (size_t)*nnz));
    CHK(Px.alloc(sizeof(double) * (size_t)*nnz));
    CHK(wlist.alloc(sizeof(int) * (size_t)wide));
    CHK(wsum.alloc(sizeof(double) * (size_t)wide));
    CHK(coarse.alloc(sizeof(int) * (size_t)n));
    CHK(diag.alloc(sizeof(double) * (size_t)n));
    CHK(exclusive_scan(splitting, coarse.i(), (size_t)n));
    hipLaunchKernelGGL(diagonal_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), diag.d());
    LAUNCH_CHECK("extended interpolation: diagonal launch");
    hipLaunchKernelGGL(extended_fill_kernel, dim3(wave_blocks), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), (const double *)diag.d(), Sp, Sj, splitting, (const int *)coarse.i(),
                       (const long *)Wp.as<long>(), wcand.i(), wlist.i(), wsum.d(), (const int *)Pp.i(), Pj.i(), Px.d());
    LAUNCH_CHECK("extended interpolation: fill launch");
    if (max_per_row > 0) {
        DBuf Tp, Tj, Tx;
        long kept = 0;
        CHK(Tp.alloc(pbytes));
        hipLaunchKernelGGL(truncate_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, max_per_row, (const int *)Pp.i(),
                           (const double *)Px.d(), count.i());
        LAUNCH_CHECK("extended interpolation: truncation count launch");
        CHK(exclusive_scan(count.i(), Tp.i(), (size_t)n + 1));
        CHK(last_offset(Tp.i(), n, &kept));
        if (kept < 0 || kept > *nnz) { set_error("extended interpolation: the truncation scan left the prolongator"); return AMG_ESTATE; }
        CHK(Tj.alloc(sizeof(int) * (size_t)kept));
        CHK(Tx.alloc(sizeof(double) * (size_t)kept));
        hipLaunchKernelGGL(truncate_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, max_per_row, (const int *)Pp.i(), (const int *)Pj.i(),
                           (const double *)Px.d(), (const int *)Tp.i(), Tj.i(), Tx.d());
        LAUNCH_CHECK("extended interpolation: truncation fill launch");
        AMG_HIP(hipDeviceSynchronize());
        Pp = std::move(Tp); Pj = std::move(Tj); Px = std::move(Tx);
        *nnz = kept;
    }
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// ------------------------------------------------------------------------------------------------ R = P^T
// The transpose of a CSR matrix with the bits and the order of scipy's csr_tocsc: row c of R
// holds the entries of column c of P in the order in which a walk over P's stored arrays meets them.  An entry's
// position k in P's arrays is unique and increases along that walk, so "row c of R ascending by k" is the whole
// definition.  Columns are counted with integer atomics and scanned; every entry then takes the next free slot of its
// column (an integer atomic again) and leaves k there.  Which slot an entry gets depends on scheduling; the multiset of
// keys in a row does not, and ordering every row by key removes the difference.  The row of R and the value follow by
// gather from the ordered keys: Rj is the row of P that holds position k (bisection of Pp), Rx the 64 bits of Px[k].
// Three forms order a row, by its length:
//   lane   at most TR_LANE_MAX entries: one lane per row, insertion sort where the keys lie;
//   lds    at most TR_LDS_MAX: one wave per row, the row in LDS, a sorting network;
//   hbm    longer (a hub that is the only C point): one workgroup per row, the same network on the row's keys in HBM.
// The network is the bitonic one in its flip/disperse form, in which every exchange leaves the smaller key at the
// smaller index: a row is padded to a power of two by slots that are never touched (they stand for keys larger than
// all others and no exchange would move them).
constexpr int TR_LANE_MAX = 32, TR_LDS_MAX = 2048, TR_HBM_THREADS = 256;

__global__ __launch_bounds__(TB) void transpose_count_kernel(long nnz, const int *Pj, int *count)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e < nnz) atomicAdd(&count[Pj[e]], 1);
}

__global__ __launch_bounds__(TB) void transpose_place_kernel(long nnz, const int *Pj, const int *Rp, int *cursor, int *key)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    const int c = Pj[e];
    key[(long)Rp[c] + atomicAdd(&cursor[c], 1)] = (int)e;
}

// the rows of the lds and hbm forms, listed in any order (each row is ordered on its own); counts: their numbers
__global__ __launch_bounds__(TB) void transpose_classify_kernel(int n_col, const int *Rp, int *lds_rows, int *hbm_rows, int *counts)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= n_col) return;
    const int len = Rp[c + 1] - Rp[c];
    if (len > TR_LDS_MAX) hbm_rows[atomicAdd(&counts[1], 1)] = c;
    else if (len > TR_LANE_MAX) lds_rows[atomicAdd(&counts[0], 1)] = c;
}

__global__ __launch_bounds__(TB) void transpose_order_lane_kernel(int n_col, const int *Rp, int *key)
{
    const int c = blockIdx.x * TB + threadIdx.x;
    if (c >= n_col) return;
    const long lo = Rp[c], hi = Rp[c + 1];
    if (hi - lo > TR_LANE_MAX) return;
    for (long a = lo + 1; a < hi; ++a) {
        const int v = key[a];
        long b = a;
        while (b > lo && key[b - 1] > v) { key[b] = key[b - 1]; --b; }
        key[b] = v;
    }
}

// a[0, len) ascending, by the THREADS lanes of one workgroup; every lane of the workgroup calls it
template <int THREADS>
__device__ __forceinline__ void order_row(int *a, int len)
{
    int padded = 1;
    while (padded < len) padded <<= 1;
    const int pairs = padded >> 1;
    for (int k = 2; k <= padded; k <<= 1) {
        const int half = k >> 1;                                // flip: i in the lower half of its block of k, mirrored partner
        for (int t = threadIdx.x; t < pairs; t += THREADS) {
            const int i = ((t & ~(half - 1)) << 1) | (t & (half - 1)), l = i ^ (k - 1);
            if (l < len) {
                const int x = a[i], y = a[l];
                if (x > y) { a[i] = y; a[l] = x; }
            }
        }
        __syncthreads();
        for (int j = k >> 2; j >= 1; j >>= 1) {                 // disperse: partner at distance j
            for (int t = threadIdx.x; t < pairs; t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                if (l < len) {
                    const int x = a[i], y = a[l];
                    if (x > y) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(WAVE) void transpose_order_lds_kernel(const int *rows, const int *Rp, int *key)
{
    __shared__ int slot[TR_LDS_MAX];
    const int c = rows[blockIdx.x];
    const long lo = Rp[c];
    const int len = Rp[c + 1] - Rp[c];                          // TR_LANE_MAX < len <= TR_LDS_MAX by the classification
    for (int t = threadIdx.x; t < len; t += WAVE) slot[t] = key[lo + t];
    __syncthreads();
    order_row<WAVE>(slot, len);
    for (int t = threadIdx.x; t < len; t += WAVE) key[lo + t] = slot[t];
}

__global__ __launch_bounds__(TR_HBM_THREADS) void transpose_order_hbm_kernel(const int *rows, const int *Rp, int *key)
{
    const int c = rows[blockIdx.x];
    order_row<TR_HBM_THREADS>(key + Rp[c], Rp[c + 1] - Rp[c]);
}

// one lane per entry of R: the row of P that holds position k = key[e], and the value there bit for bit
__global__ __launch_bounds__(TB) void transpose_gather_kernel(int n_row, long nnz, const int *Pp, const unsigned long long *Px,
                                                              const int *key, int *Rj, unsigned long long *Rx)
{
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= nnz) return;
    const int k = key[e];
    int lo = 0, hi = n_row;                 // invariant: Pp[lo] <= k < Pp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (Pp[mid] <= k) lo = mid; else hi = mid;
    }
    Rj[e] = lo;
    Rx[e] = Px[k];
}

// what the calling thread's most recent transpose did (amg_transpose_last_route)
struct TransposeRoute { int launched = 0, lane_rows = 0, lds_rows = 0, hbm_rows = 0; };
thread_local TransposeRoute last_transpose;

// R = P^T for P (n_row x n_col, nnz entries, columns inside the matrix) in HBM into Rp (n_col + 1 offsets) and freshly
// allocated Rj, Rx.  Without entries or rows: the offsets are zeroed and nothing is launched.
int transpose_device(int n_row, int n_col, long nnz, const int *Pp, const int *Pj, const double *Px, DBuf &Rp, DBuf &Rj, DBuf &Rx)
{
    last_transpose = TransposeRoute{};
    const size_t cbytes = sizeof(int) * ((size_t)n_col + 1);
    CHK(Rj.alloc(sizeof(int) * (size_t)nnz));
    CHK(Rx.alloc(sizeof(double) * (size_t)nnz));
    if (n_row <= 0 || nnz <= 0) return Rp.zero(cbytes);
    DBuf count, key, lds_rows, hbm_rows, counts;
    const long lds_most = std::min<long>(n_col, nnz / (TR_LANE_MAX + 1)), hbm_most = std::min<long>(n_col, nnz / (TR_LDS_MAX + 1));
    CHK(count.zero(cbytes));
    CHK(Rp.alloc(cbytes));
    CHK(key.alloc(sizeof(int) * (size_t)nnz));
    CHK(lds_rows.alloc(sizeof(int) * (size_t)lds_most));
    CHK(hbm_rows.alloc(sizeof(int) * (size_t)hbm_most));
    CHK(counts.zero(sizeof(int) * 2));
    hipLaunchKernelGGL(transpose_count_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, Pj, count.i());
    LAUNCH_CHECK("transpose: count launch");
    CHK(exclusive_scan(count.i(), Rp.i(), (size_t)n_col + 1));
    long total = 0;
    CHK(last_offset(Rp.i(), n_col, &total));
    if (total != nnz) { set_error("transpose: the scan and the entries disagree"); return AMG_ESTATE; }
    AMG_HIP(hipMemsetAsync(count.p, 0, cbytes, nullptr));
    hipLaunchKernelGGL(transpose_place_kernel, grid_for(nnz), dim3(TB), 0, nullptr, nnz, Pj, (const int *)Rp.i(), count.i(), key.i());
    LAUNCH_CHECK("transpose: placement launch");
    hipLaunchKernelGGL(transpose_classify_kernel, grid_for(n_col), dim3(TB), 0, nullptr, n_col, (const int *)Rp.i(), lds_rows.i(),
                       hbm_rows.i(), counts.i());
    LAUNCH_CHECK("transpose: classification launch");
    hipLaunchKernelGGL(transpose_order_lane_kernel, grid_for(n_col), dim3(TB), 0, nullptr, n_col, (const int *)Rp.i(), key.i());
    LAUNCH_CHECK("transpose: lane form launch");
    int longer[2] = {0, 0};
    AMG_HIP(hipMemcpy(longer, counts.p, sizeof(longer), hipMemcpyDeviceToHost));
    if (longer[0] < 0 || longer[0] > lds_most || longer[1] < 0 || longer[1] > hbm_most) {
        set_error("transpose: the classification left its lists");
        return AMG_ESTATE;
    }
    if (longer[0] > 0) {
        hipLaunchKernelGGL(transpose_order_lds_kernel, dim3((unsigned)longer[0]), dim3(WAVE), 0, nullptr, (const int *)lds_rows.i(),
                           (const int *)Rp.i(), key.i());
        LAUNCH_CHECK("transpose: LDS form launch");
    }
    if (longer[1] > 0) {
        hipLaunchKernelGGL(transpose_order_hbm_kernel, dim3((unsigned)longer[1]), dim3(TR_HBM_THREADS), 0, nullptr,
                           (const int *)hbm_rows.i(), (const int *)Rp.i(), key.i());
        LAUNCH_CHECK("transpose: HBM form launch");
    }
    hipLaunchKernelGGL(transpose_gather_kernel, grid_for(nnz), dim3(TB), 0, nullptr, n_row, nnz, Pp, (const unsigned long long *)Px,
                       (const int *)key.i(), Rj.i(), Rx.as<unsigned long long>());
    LAUNCH_CHECK("transpose: gather launch");
    AMG_HIP(hipDeviceSynchronize());
    last_transpose = TransposeRoute{1, n_col - longer[0] - longer[1], longer[0], longer[1]};
    return 0;
}

// One bit per fact about a CSR operator in HBM, by one lane per row: ROWS_UNSORTED where a row is not strictly
// ascending, VALUE_NOT_FINITE where a value is an infinity or a NaN.  Integer atomics: the result does not depend on order.
constexpr int ROWS_UNSORTED = 1, VALUE_NOT_FINITE = 2;

__global__ __launch_bounds__(TB) void operator_facts_kernel(int n, const int *Ap, const int *Aj, const double *Ax, int *facts)
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

__global__ __launch_bounds__(TB) void count_ones_kernel(int n, const int *splitting, int *total)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    const int ones = __syncthreads_count(i < n && splitting[i] == 1);
    if (threadIdx.x == 0 && ones > 0) atomicAdd(total, ones);
}

}   // namespace

// the columns and values of a prolongator, held for amg_extended_interpolation_fetch
struct amg_interpolation {
    long nnz = 0;
    DBuf Pj, Px;
};

// the result of one chained level, held for amg_classical_level_fetch
struct amg_classical {
    int n = 0;
    long s_nnz = 0, p_nnz = 0;
    DBuf Sp, Sj, Sx, splitting, Pp, Pj, Px;
    double times_ms[5] = {0, 0, 0, 0, 0};
};

// the columns and values of a transpose, held for amg_csr_transpose_fetch
struct amg_transpose {
    long nnz = 0;
    DBuf Rj, Rx;
};

// A chain of classical levels.  It owns the resident operator A (n x n, nnz entries, `reversed` as the level entries
// take it) and, between amg_classical_chain_level and amg_classical_chain_fetch, the level built from it: S, the
// splitting and P in `level`, R and the coarse operator C beside it.  The fetch moves C into A and drops the rest.
enum { CHAIN_IDLE = 0, CHAIN_BUILT = 1, CHAIN_REFUSED = 2 };
struct amg_classical_chain {
    int n = 0, reversed = 0, state = CHAIN_IDLE;
    long nnz = 0;
    HbmCsr A;
    double upload_ms = 0.0;         // of A_0: reported with the first level
    amg_classical level;
    int n_coarse = 0, c_facts = 0;
    long c_nnz = 0;
    DBuf Rp, Rj, Rx, Cp, Cj, Cx;
    double times_ms[AMG_CHAIN_STAGES] = {0, 0, 0, 0, 0, 0, 0, 0};
    void drop_level()
    {
        level = amg_classical{};
        Rp.reset(); Rj.reset(); Rx.reset(); Cp.reset(); Cj.reset(); Cx.reset();
        state = CHAIN_IDLE;
    }
};

// One level from an operator that is already in HBM (A: n x n with a_nnz entries; dr: the n start values): strength, the
// strength graph, the start weights, the splitting and the interpolation into h, h.times_ms[1 .. 4] from timer's laps.
// amg_classical_level_build runs it on what it uploaded, the chain (below) on the product its last level left.
static int classical_level_resident(int n, const HbmCsr &A, long a_nnz, double theta, int kind, int reversed, const DBuf &dr,
                                    int interpolation, int max_per_row, amg_classical &h, int *rounds, LapClock &timer)
{
    const size_t vbytes = sizeof(int) * (size_t)n, pbytes = sizeof(int) * ((size_t)n + 1);
    h.n = n;

    // 1. strength
    CHK(strength_device(n, theta, A, a_nnz, h.Sp, h.Sj, h.Sx, &h.s_nnz));
    h.times_ms[1] = timer.lap();

    // 2. G = S without its diagonal, the pattern of T = G^T and the in-degrees
    DBuf count, indegree, cursor, Gp, Gj, Tp, Tj;
    CHK(count.alloc(pbytes)); CHK(indegree.zero(pbytes)); CHK(cursor.zero(vbytes));
    CHK(Gp.alloc(pbytes)); CHK(Tp.alloc(pbytes));
    hipLaunchKernelGGL(graph_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, (const int *)h.Sp.i(), (const int *)h.Sj.i(),
                       count.i(), indegree.i());
    LAUNCH_CHECK("classical level: graph count launch");
    CHK(exclusive_scan(count.i(), Gp.i(), (size_t)n + 1));
    CHK(exclusive_scan(indegree.i(), Tp.i(), (size_t)n + 1));
    long g_nnz = 0, t_nnz = 0;
    CHK(last_offset(Gp.i(), n, &g_nnz));
    CHK(last_offset(Tp.i(), n, &t_nnz));
    if (g_nnz < 0 || g_nnz > h.s_nnz || t_nnz != g_nnz) { set_error("classical level: the graph scans disagree"); return AMG_ESTATE; }
    CHK(Gj.alloc(sizeof(int) * (size_t)g_nnz)); CHK(Tj.alloc(sizeof(int) * (size_t)g_nnz));
    hipLaunchKernelGGL(graph_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)h.Sp.i(), (const int *)h.Sj.i(),
                       (const int *)Gp.i(), Gj.i(), (const int *)Tp.i(), cursor.i(), Tj.i());
    LAUNCH_CHECK("classical level: graph fill launch");

    // 3. the start weights
    DBuf weight;
    CHK(weight.alloc(sizeof(double) * (size_t)n));
    hipLaunchKernelGGL(start_weights_kernel, grid_for(n), dim3(TB), 0, nullptr, n, kind, (const int *)indegree.i(), (const double *)dr.d(),
                       weight.d());
    LAUNCH_CHECK("classical level: weight launch");
    AMG_HIP(hipDeviceSynchronize());
    h.times_ms[2] = timer.lap();

    // 4. the splitting
    CHK(h.splitting.alloc(vbytes));
    int done = 0;
    if (kind == KIND_PMIS) {
        DBuf Up, Uj, flag;
        CHK(Up.alloc(pbytes)); CHK(Uj.alloc(sizeof(int) * 2 * (size_t)g_nnz)); CHK(flag.alloc(sizeof(int)));
        hipLaunchKernelGGL(union_offsets_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, (const int *)Gp.i(), (const int *)Tp.i(),
                           Up.i());
        LAUNCH_CHECK("classical level: union offsets launch");
        hipLaunchKernelGGL(union_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)Gp.i(), (const int *)Gj.i(),
                           (const int *)Tp.i(), (const int *)Tj.i(), (const int *)Up.i(), Uj.i());
        LAUNCH_CHECK("classical level: union fill launch");
        hipLaunchKernelGGL(fill_kernel, grid_for(n), dim3(TB), 0, nullptr, (long)n, -1, h.splitting.i());
        LAUNCH_CHECK("classical level: state launch");
        CHK(mis_rounds_device(n, Up.i(), Uj.i(), weight.d(), -1, 1, 0, h.splitting.i(), flag.i(), &done));
    } else {
        CHK(cljp_passes_device(n, g_nnz, Gp.i(), Gj.i(), Tp.i(), Tj.i(), weight.d(), h.splitting.i(), &done));
    }
    AMG_HIP(hipDeviceSynchronize());
    h.times_ms[3] = timer.lap();

    // 5. interpolation on S's pattern: extended+i reads the pattern as the strength kernel stored it, direct
    // interpolation also the values written beside it
    if (interpolation == INTERP_EXTENDED_I) {
        CHK(extended_interpolation_device(n, A, h.Sp.i(), h.Sj.i(), h.splitting.i(), max_per_row, h.Pp, h.Pj, h.Px, &h.p_nnz));
    } else {
        CHK(interpolation_offsets_device(n, h.Sp.i(), h.Sj.i(), h.splitting.i(), h.Pp, &h.p_nnz));
        if (h.p_nnz < 0 || h.p_nnz > h.s_nnz + n) { set_error("classical level: the interpolation scan left the matrix"); return AMG_ESTATE; }
        CHK(h.Pj.alloc(sizeof(int) * (size_t)h.p_nnz));
        CHK(h.Px.alloc(sizeof(double) * (size_t)h.p_nnz));
        CHK(interpolation_fill_device(n, A, h.Sp.i(), h.Sj.i(), h.Sx.d(), h.splitting.i(), h.Pp.i(), h.Pj.i(), h.Px.d(), reversed ? -1 : 1));
    }
    h.times_ms[4] = timer.lap();

    *rounds = done;
    return 0;
}

extern "C" {

int amgcore_classical_strength_of_connection_f64(int n_row, double theta, const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                                 const double Ax[], int Ax_size, int Sp[], int Sp_size, int Sj[], int Sj_size, double Sx[],
                                                 int Sx_size)
{
    const char *who = "classical_strength_of_connection";
    CHK(check_csr_arrays(who, n_row, n_row, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size));
    if (!Sp || Sp_size < n_row + 1) return bad(who, "Sp shorter than n_row + 1");
    if (n_row == 0) { Sp[0] = 0; return 0; }
    CHK(require_device());
    HbmCsr A;
    CHK(A.upload(n_row, Ap, Aj, Ax));
    DBuf dSp, dSj, dSx;
    long nnz = 0;
    CHK(strength_device(n_row, theta, A, Ap[n_row], dSp, dSj, dSx, &nnz));
    if (nnz > Sj_size || nnz > Sx_size || (nnz > 0 && (!Sj || !Sx))) return bad(who, "Sj / Sx shorter than the entries kept");
    CHK(dSp.to_host(Sp, sizeof(int) * ((size_t)n_row + 1)));
    CHK(dSj.to_host(Sj, sizeof(int) * (size_t)nnz));
    return dSx.to_host(Sx, sizeof(double) * (size_t)nnz);
}

int amgcore_maximum_row_value_f64(int n_row, double x[], int x_size, const int Ap[], int Ap_size, const int Aj[], int Aj_size,
                                  const double Ax[], int Ax_size)
{
    const char *who = "maximum_row_value";
    if (n_row < 0) return bad(who, "negative size");
    // the reference never reads Aj here: its columns only have to be there
    CHK(check_csr_arrays(who, n_row, 0x7fffffff, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size));
    if (x_size < n_row || (n_row > 0 && !x)) return bad(who, "x shorter than n_row");
    if (n_row == 0) return 0;
    CHK(require_device());
    HbmCsr A;
    CHK(A.upload(n_row, Ap, Aj, Ax));
    DBuf dx;
    CHK(dx.alloc(sizeof(double) * (size_t)n_row));
    hipLaunchKernelGGL(maximum_row_value_kernel, grid_for(n_row), dim3(TB), 0, nullptr, n_row, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), dx.d());
    LAUNCH_CHECK("maximum_row_value launch");
    AMG_HIP(hipDeviceSynchronize());
    return dx.to_host(x, sizeof(double) * (size_t)n_row);
}

int amgcore_rs_direct_interpolation_pass1_f64(int n_nodes, const int Sp[], int Sp_size, const int Sj[], int Sj_size, const int splitting[],
                                              int splitting_size, int Bp[], int Bp_size)
{
    const char *who = "rs_direct_interpolation_pass1";
    CHK(check_csr_arrays(who, n_nodes, n_nodes, Sp, Sp_size, Sj, Sj_size, nullptr, -1));
    CHK(check_splitting(who, n_nodes, splitting, splitting_size));
    if (!Bp || Bp_size < n_nodes + 1) return bad(who, "Bp shorter than n_nodes + 1");
    if (n_nodes == 0) { Bp[0] = 0; return 0; }
    CHK(require_device());
    HbmCsr S;
    CHK(S.upload(n_nodes, Sp, Sj, nullptr));
    DBuf dsplit, dBp;
    CHK(dsplit.from_host(splitting, sizeof(int) * (size_t)n_nodes));
    long nnz = 0;
    CHK(interpolation_offsets_device(n_nodes, S.p.i(), S.j.i(), dsplit.i(), dBp, &nnz));
    return dBp.to_host(Bp, sizeof(int) * ((size_t)n_nodes + 1));
}

int amgcore_rs_direct_interpolation_pass2_f64(int n_nodes, const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[],
                                              int Ax_size, const int Sp[], int Sp_size, const int Sj[], int Sj_size, const double Sx[],
                                              int Sx_size, const int splitting[], int splitting_size, const int Bp[], int Bp_size, int Bj[],
                                              int Bj_size, double Bx[], int Bx_size)
{
    const char *who = "rs_direct_interpolation_pass2";
    CHK(check_csr_arrays(who, n_nodes, n_nodes, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size));
    CHK(check_csr_arrays(who, n_nodes, n_nodes, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size));
    CHK(check_splitting(who, n_nodes, splitting, splitting_size));
    if (!Bp || Bp_size < n_nodes + 1) return bad(who, "Bp shorter than n_nodes + 1");
    if (Bp[0] != 0) return bad(who, "Bp does not start at 0");
    // every row writes exactly what pass 1 counted for it: Bp has to be pass 1's answer
    for (int i = 0; i < n_nodes; ++i) {
        int kept = 1;
        if (splitting[i] != C_NODE) {
            kept = 0;
            for (int jj = Sp[i]; jj < Sp[i + 1]; ++jj)
                if (splitting[Sj[jj]] == C_NODE && Sj[jj] != i) ++kept;
        }
        if (Bp[i + 1] - Bp[i] != kept) return bad(who, "Bp is not the result of pass 1");
    }
    if (n_nodes == 0) return 0;
    const long nnz = Bp[n_nodes];
    if (nnz > Bj_size || nnz > Bx_size || (nnz > 0 && (!Bj || !Bx))) return bad(who, "Bj / Bx shorter than Bp[n_nodes]");
    CHK(require_device());
    HbmCsr A, S;
    CHK(A.upload(n_nodes, Ap, Aj, Ax));
    CHK(S.upload(n_nodes, Sp, Sj, Sx));
    DBuf dsplit, dBp, dBj, dBx;
    CHK(dsplit.from_host(splitting, sizeof(int) * (size_t)n_nodes));
    CHK(dBp.from_host(Bp, sizeof(int) * ((size_t)n_nodes + 1)));
    CHK(dBj.alloc(sizeof(int) * (size_t)nnz));
    CHK(dBx.alloc(sizeof(double) * (size_t)nnz));
    CHK(interpolation_fill_device(n_nodes, A, S.p.i(), S.j.i(), S.x.d(), dsplit.i(), dBp.i(), dBj.i(), dBx.d(), 1));
    CHK(dBj.to_host(Bj, sizeof(int) * (size_t)nnz));
    return dBx.to_host(Bx, sizeof(double) * (size_t)nnz);
}

int amg_extended_interpolation_device(int n, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj,
                                      const int *splitting, int max_per_row, int *Pp, amg_interpolation **out, double *times_ms)
{
    const char *who = "extended interpolation";
    if (!out || !Pp) return bad(who, "bad arguments");
    *out = nullptr;
    if (max_per_row < 0) return bad(who, "max_per_row is 0 (no truncation) or positive");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    CHK(check_csr_arrays(who, n, n, Sp, n + 1, Sj, 0x7fffffff, nullptr, -1));
    CHK(check_splitting(who, n, splitting, n));
    CHK(check_unique_columns(who, n, Ap, Aj));
    CHK(check_unique_columns(who, n, Sp, Sj));
    if (times_ms) times_ms[0] = times_ms[1] = 0.0;
    struct Guard {
        amg_interpolation *h;
        ~Guard() { delete h; }
    } guard{new amg_interpolation};
    amg_interpolation &h = *guard.h;
    if (n == 0) {
        Pp[0] = 0;
        *out = guard.h;
        guard.h = nullptr;
        return 0;
    }
    CHK(require_device());
    LapClock timer;
    HbmCsr A, S;
    DBuf dsplit, dPp;
    CHK(A.upload(n, Ap, Aj, Ax));
    CHK(S.upload(n, Sp, Sj, nullptr));
    CHK(dsplit.from_host(splitting, sizeof(int) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    CHK(extended_interpolation_device(n, A, S.p.i(), S.j.i(), dsplit.i(), max_per_row, dPp, h.Pj, h.Px, &h.nnz));
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = timer.lap(); }
    CHK(dPp.to_host(Pp, sizeof(int) * ((size_t)n + 1)));
    *out = guard.h;
    guard.h = nullptr;
    return 0;
}

int amg_extended_interpolation_fetch(amg_interpolation *h, int *Pj, double *Px)
{
    if (!h) return AMG_EINVAL;
    struct Guard {
        amg_interpolation *h;
        ~Guard() { delete h; }
    } guard{h};
    if (h->nnz > 0 && (!Pj || !Px)) return bad("extended interpolation fetch", "null array");
    CHK(h->Pj.to_host(Pj, sizeof(int) * (size_t)h->nnz));
    return h->Px.to_host(Px, sizeof(double) * (size_t)h->nnz);
}

int amg_classical_level_device(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int kind, int reversed,
                               const double *r, amg_classical **out, long *sizes, int *rounds, double *times_ms)
{
    return amg_classical_level_build(n, Ap, Aj, Ax, theta, kind, reversed, r, 0, 0, out, sizes, rounds, times_ms);
}

int amg_classical_level_build(int n, const int *Ap, const int *Aj, const double *Ax, double theta, int kind, int reversed,
                              const double *r, int interpolation, int max_per_row, amg_classical **out, long *sizes, int *rounds,
                              double *times_ms)
{
    const char *who = "classical level";
    if (!out || !sizes) return bad(who, "bad arguments");
    *out = nullptr;
    if (kind != KIND_PMIS && kind != KIND_CLJP) return bad(who, "the splitting is 0 (PMIS) or 1 (CLJP)");
    if (interpolation != INTERP_DIRECT && interpolation != INTERP_EXTENDED_I)
        return bad(who, "the interpolation is 0 (direct) or 1 (extended+i)");
    if (max_per_row < 0 || (max_per_row > 0 && interpolation == INTERP_DIRECT))
        return bad(who, "max_per_row is 0, or positive with extended+i");
    if (n <= 0 || !r) return bad(who, "an empty operator or no start values");
    if (!(theta >= 0.0 && theta <= 1.0)) return bad(who, "expected theta in [0, 1]");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    if (interpolation == INTERP_EXTENDED_I) CHK(check_unique_columns(who, n, Ap, Aj));
    CHK(require_device());
    LapClock timer;
    HbmCsr A;
    CHK(A.upload(n, Ap, Aj, Ax));
    DBuf dr;
    CHK(dr.from_host(r, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    // the handle owns what outlives this call; an early return frees it with everything it holds by then
    struct Guard {
        amg_classical *h;
        ~Guard() { delete h; }
    } guard{new amg_classical};
    amg_classical &h = *guard.h;
    h.times_ms[0] = timer.lap();
    int done = 0;
    CHK(classical_level_resident(n, A, Ap[n], theta, kind, reversed, dr, interpolation, max_per_row, h, &done, timer));

    sizes[0] = h.s_nnz;
    sizes[1] = h.p_nnz;
    if (rounds) *rounds = done;
    if (times_ms) std::copy(h.times_ms, h.times_ms + 5, times_ms);
    *out = guard.h;
    guard.h = nullptr;
    return 0;
}

int amg_classical_level_fetch(amg_classical *h, int *splitting, int *Pp, int *Pj, double *Px, int *Sp, int *Sj, double *Sx,
                              double *times_ms)
{
    if (!h) return AMG_EINVAL;
    struct Guard {
        amg_classical *h;
        ~Guard() { delete h; }
    } guard{h};
    if (!splitting || !Pp || (h->p_nnz > 0 && (!Pj || !Px))) return bad("classical level fetch", "null array");
    LapClock timer;
    const size_t pbytes = sizeof(int) * ((size_t)h->n + 1);
    CHK(h->splitting.to_host(splitting, sizeof(int) * (size_t)h->n));
    CHK(h->Pp.to_host(Pp, pbytes));
    CHK(h->Pj.to_host(Pj, sizeof(int) * (size_t)h->p_nnz));
    CHK(h->Px.to_host(Px, sizeof(double) * (size_t)h->p_nnz));
    if (Sp) {
        if (h->s_nnz > 0 && (!Sj || !Sx)) return bad("classical level fetch", "null array");
        hipLaunchKernelGGL(scale_rows_kernel, grid_for(h->n), dim3(TB), 0, nullptr, h->n, (const int *)h->Sp.i(), h->Sx.d());
        LAUNCH_CHECK("classical level: scaling launch");
        CHK(h->Sp.to_host(Sp, pbytes));
        CHK(h->Sj.to_host(Sj, sizeof(int) * (size_t)h->s_nnz));
        CHK(h->Sx.to_host(Sx, sizeof(double) * (size_t)h->s_nnz));
    }
    if (times_ms) {
        std::copy(h->times_ms, h->times_ms + 5, times_ms);
        times_ms[5] = timer.lap();
    }
    return 0;
}

// ---- R = P^T as a flat entry: host arrays in, the offsets out at once, columns and values through a handle

int amg_csr_transpose_device(int n_row, int n_col, const int *Pp, const int *Pj, const double *Px, int *Rp, amg_transpose **out)
{
    const char *who = "transpose";
    if (!out || !Rp) return bad(who, "bad arguments");
    *out = nullptr;
    if (n_col < 0) return bad(who, "negative size");
    CHK(check_csr_arrays(who, n_row, n_col, Pp, n_row + 1, Pj, 0x7fffffff, Px, 0x7fffffff));
    last_transpose = TransposeRoute{};
    struct Guard {
        amg_transpose *h;
        ~Guard() { delete h; }
    } guard{new amg_transpose};
    amg_transpose &h = *guard.h;
    h.nnz = n_row > 0 ? Pp[n_row] : 0;
    if (h.nnz == 0) {                       // no rows or no entries: the empty result, without a launch
        std::fill(Rp, Rp + (size_t)n_col + 1, 0);
        *out = guard.h;
        guard.h = nullptr;
        return 0;
    }
    CHK(require_device());
    HbmCsr P;
    DBuf dRp;
    CHK(P.upload(n_row, Pp, Pj, Px));
    CHK(transpose_device(n_row, n_col, h.nnz, P.p.i(), P.j.i(), P.x.d(), dRp, h.Rj, h.Rx));
    CHK(dRp.to_host(Rp, sizeof(int) * ((size_t)n_col + 1)));
    *out = guard.h;
    guard.h = nullptr;
    return 0;
}

int amg_csr_transpose_fetch(amg_transpose *h, int *Rj, double *Rx)
{
    if (!h) return AMG_EINVAL;
    struct Guard {
        amg_transpose *h;
        ~Guard() { delete h; }
    } guard{h};
    if (h->nnz > 0 && (!Rj || !Rx)) return bad("transpose fetch", "null array");
    if (h->nnz == 0) return 0;
    CHK(h->Rj.to_host(Rj, sizeof(int) * (size_t)h->nnz));
    return h->Rx.to_host(Rx, sizeof(double) * (size_t)h->nnz);
}

int amg_transpose_last_route(int *out, int n)
{
    const int f[AMG_TRANSPOSE_ROUTE_FIELDS] = {last_transpose.launched, last_transpose.lane_rows, last_transpose.lds_rows,
                                               last_transpose.hbm_rows};
    for (int q = 0; out && q < n && q < AMG_TRANSPOSE_ROUTE_FIELDS; ++q) out[q] = f[q];
    return AMG_TRANSPOSE_ROUTE_FIELDS;
}

// ---- the chain: A_l, P_l, R_l, R_l A_l and A_{l+1} stay in HBM from the upload of A_0 on

int amg_classical_chain_begin(int n, const int *Ap, const int *Aj, const double *Ax, int reversed, amg_classical_chain **out)
{
    const char *who = "classical chain";
    if (!out) return bad(who, "bad arguments");
    *out = nullptr;
    if (n <= 0) return bad(who, "an empty operator");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    CHK(check_unique_columns(who, n, Ap, Aj));       // extended+i and the right-hand operand of R * A both need it
    CHK(require_device());
    LapClock timer;
    struct Guard {
        amg_classical_chain *c;
        ~Guard() { delete c; }
    } guard{new amg_classical_chain};
    amg_classical_chain &c = *guard.c;
    CHK(c.A.upload(n, Ap, Aj, Ax));
    AMG_HIP(hipDeviceSynchronize());
    c.n = n;
    c.nnz = Ap[n];
    c.reversed = reversed ? 1 : 0;
    c.upload_ms = timer.lap();
    *out = guard.c;
    guard.c = nullptr;
    return 0;
}

int amg_classical_chain_level(amg_classical_chain *c, double theta, int kind, const double *r, int interpolation, int max_per_row,
                              long *sizes, int *flags, int *rounds, double *times_ms)
{
    const char *who = "classical chain";
    if (!c || !sizes || !flags) return bad(who, "bad arguments");
    if (kind != KIND_PMIS && kind != KIND_CLJP) return bad(who, "the splitting is 0 (PMIS) or 1 (CLJP)");
    if (interpolation != INTERP_DIRECT && interpolation != INTERP_EXTENDED_I)
        return bad(who, "the interpolation is 0 (direct) or 1 (extended+i)");
    if (max_per_row < 0 || (max_per_row > 0 && interpolation == INTERP_DIRECT))
        return bad(who, "max_per_row is 0, or positive with extended+i");
    if (c->n <= 0 || !r) return bad(who, "no resident operator or no start values");
    if (!(theta >= 0.0 && theta <= 1.0)) return bad(who, "expected theta in [0, 1]");
    if (c->state != CHAIN_IDLE) { set_error("classical chain: the level built last has not been fetched"); return AMG_ESTATE; }
    // The resident operator is not checked again.  A_0 passed begin's checks; a later one is a product of spgemm.hip,
    // which stores one entry per column and drops exact zeros, so of what the host route vets only the row order and the
    // finiteness of the values are open, and those came with the product's facts (below).
    const int n = c->n;
    LapClock timer;
    DBuf dr;
    CHK(dr.from_host(r, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    // an early return leaves the chain without a level, its resident operator as it was
    struct Drop {
        amg_classical_chain *c;
        ~Drop() { if (c) c->drop_level(); }
    } drop{c};
    amg_classical &h = c->level;
    std::fill(c->times_ms, c->times_ms + AMG_CHAIN_STAGES, 0.0);
    c->times_ms[0] = c->upload_ms + timer.lap();
    c->upload_ms = 0.0;
    int done = 0;
    CHK(classical_level_resident(n, c->A, c->nnz, theta, kind, c->reversed, dr, interpolation, max_per_row, h, &done, timer));
    std::copy(h.times_ms + 1, h.times_ms + 5, c->times_ms + 1);

    // 6. R = P^T; the coarse size is the number of C points
    DBuf total;
    CHK(total.zero(sizeof(int)));
    hipLaunchKernelGGL(count_ones_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)h.splitting.i(), total.i());
    LAUNCH_CHECK("classical chain: coarse size launch");
    AMG_HIP(hipMemcpy(&c->n_coarse, total.p, sizeof(int), hipMemcpyDeviceToHost));
    if (c->n_coarse < 0 || c->n_coarse > n) { set_error("classical chain: the coarse size left the level"); return AMG_ESTATE; }
    CHK(transpose_device(n, c->n_coarse, h.p_nnz, h.Pp.i(), h.Pj.i(), h.Px.d(), c->Rp, c->Rj, c->Rx));
    const TransposeRoute how = last_transpose;
    c->times_ms[5] = timer.lap();

    // 7. A_c = (R * A) * P by the routes of spgemm.hip; R * A goes when the second product has run
    int tables[2] = {0, 0};
    int rc = 0;
    c->c_nnz = 0;
    {
        DevArr<long> Ap64, Rp64, Pp64, RAp, Cp64;
        DevArr<int> RAj, Cj;
        DevArr<double> RAx, Cx;
        long ra_nnz = 0;
        int route[AMG_SPGEMM_ROUTE_FIELDS];
        CHK(widen_rowptr_device(n, c->A.p.i(), Ap64));
        CHK(widen_rowptr_device(c->n_coarse, c->Rp.i(), Rp64));
        CHK(widen_rowptr_device(n, h.Pp.i(), Pp64));
        rc = spgemm_device(c->n_coarse, n, n, h.p_nnz, Rp64, c->Rj.i(), c->Rx.d(), c->nnz, Ap64, c->A.j.i(), c->A.x.d(), &ra_nnz, RAp, RAj,
                           RAx);
        amg_spgemm_last_route(route, AMG_SPGEMM_ROUTE_FIELDS);
        tables[0] = route[3];
        if (rc == 0) {
            rc = spgemm_device(c->n_coarse, n, c->n_coarse, ra_nnz, RAp, RAj, RAx, h.p_nnz, Pp64, h.Pj.i(), h.Px.d(), &c->c_nnz, Cp64, Cj,
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
    c->c_facts = 0;
    if (rc == 0) {
        // the row order and the finiteness of A_c in one pass over it, where it lies
        DBuf facts;
        CHK(facts.zero(sizeof(int)));
        hipLaunchKernelGGL(operator_facts_kernel, grid_for(c->n_coarse), dim3(TB), 0, nullptr, c->n_coarse, (const int *)c->Cp.i(),
                           (const int *)c->Cj.i(), (const double *)c->Cx.d(), facts.i());
        LAUNCH_CHECK("classical chain: operator facts launch");
        AMG_HIP(hipMemcpy(&c->c_facts, facts.p, sizeof(int), hipMemcpyDeviceToHost));
    }
    c->times_ms[6] = timer.lap();

    sizes[0] = h.s_nnz;
    sizes[1] = h.p_nnz;
    sizes[2] = h.p_nnz;
    sizes[3] = c->c_nnz;
    sizes[4] = c->n_coarse;
    flags[0] = rc == 0 && !(c->c_facts & ROWS_UNSORTED);
    flags[1] = rc == 0 && !(c->c_facts & VALUE_NOT_FINITE);
    flags[2] = tables[0];
    flags[3] = tables[1];
    flags[4] = how.launched; flags[5] = how.lane_rows; flags[6] = how.lds_rows; flags[7] = how.hbm_rows;
    if (rounds) *rounds = done;
    if (times_ms) std::copy(c->times_ms, c->times_ms + AMG_CHAIN_STAGES - 1, times_ms);
    c->state = rc == 0 ? CHAIN_BUILT : CHAIN_REFUSED;
    drop.c = nullptr;
    return rc == 0 ? 0 : AMG_CHAIN_PRODUCT_REFUSED;
}

int amg_classical_chain_fetch(amg_classical_chain *c, int *splitting, int *Pp, int *Pj, double *Px, int *Rp, int *Rj, double *Rx,
                              int *Cp, int *Cj, double *Cx, int *Sp, int *Sj, double *Sx, double *times_ms)
{
    const char *who = "classical chain fetch";
    if (!c) return AMG_EINVAL;
    if (c->state == CHAIN_IDLE) { set_error("classical chain fetch: no level has been built"); return AMG_ESTATE; }
    // the level's buffers go whatever happens below; A_c becomes the resident operator only after a complete fetch
    struct Drop {
        amg_classical_chain *c;
        ~Drop() { c->drop_level(); }
    } drop{c};
    const bool whole = c->state == CHAIN_BUILT;
    amg_classical &h = c->level;
    if (!splitting || !Pp || (h.p_nnz > 0 && (!Pj || !Px))) return bad(who, "null array");
    const bool want_R = whole && Rp, want_C = whole && Cp;      // a caller that finishes the level on the host wants neither
    if ((want_R && h.p_nnz > 0 && (!Rj || !Rx)) || (want_C && c->c_nnz > 0 && (!Cj || !Cx))) return bad(who, "null array");
    LapClock timer;
    const size_t pbytes = sizeof(int) * ((size_t)h.n + 1), cbytes = sizeof(int) * ((size_t)c->n_coarse + 1);
    CHK(h.splitting.to_host(splitting, sizeof(int) * (size_t)h.n));
    CHK(h.Pp.to_host(Pp, pbytes));
    CHK(h.Pj.to_host(Pj, sizeof(int) * (size_t)h.p_nnz));
    CHK(h.Px.to_host(Px, sizeof(double) * (size_t)h.p_nnz));
    if (want_R) {
        CHK(c->Rp.to_host(Rp, cbytes));
        CHK(c->Rj.to_host(Rj, sizeof(int) * (size_t)h.p_nnz));
        CHK(c->Rx.to_host(Rx, sizeof(double) * (size_t)h.p_nnz));
    }
    if (want_C) {
        CHK(c->Cp.to_host(Cp, cbytes));
        CHK(c->Cj.to_host(Cj, sizeof(int) * (size_t)c->c_nnz));
        CHK(c->Cx.to_host(Cx, sizeof(double) * (size_t)c->c_nnz));
    }
    if (Sp) {
        if (h.s_nnz > 0 && (!Sj || !Sx)) return bad(who, "null array");
        hipLaunchKernelGGL(scale_rows_kernel, grid_for(h.n), dim3(TB), 0, nullptr, h.n, (const int *)h.Sp.i(), h.Sx.d());
        LAUNCH_CHECK("classical chain: scaling launch");
        CHK(h.Sp.to_host(Sp, pbytes));
        CHK(h.Sj.to_host(Sj, sizeof(int) * (size_t)h.s_nnz));
        CHK(h.Sx.to_host(Sx, sizeof(double) * (size_t)h.s_nnz));
    }
    if (whole) {
        c->A.p = std::move(c->Cp); c->A.j = std::move(c->Cj); c->A.x = std::move(c->Cx);
        c->n = c->n_coarse;
        c->nnz = c->c_nnz;
        c->reversed = (c->c_facts & ROWS_UNSORTED) ? 1 : 0;
    } else {                                // the product was refused: the chain ends here, its caller begins another
        c->A = HbmCsr{};
        c->n = 0;
        c->nnz = 0;
    }
    if (times_ms) {
        std::copy(c->times_ms, c->times_ms + AMG_CHAIN_STAGES - 1, times_ms);
        times_ms[AMG_CHAIN_STAGES - 1] = timer.lap();
    }
    return 0;
}

void amg_classical_chain_free(amg_classical_chain *c) { delete c; }

}   // extern "C"

// ================================================================================================ MIS(2) aggregation
// Third part of this translation unit, kept in a file of its own: the distance-k independent set and the MIS(2)
// aggregation, amg_mis_k_device and amg_mis_aggregation_device.
#include "misagg.hpp"
