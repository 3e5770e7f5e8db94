// The parallel C/F splittings of the classical setup on the device: Luby's maximal independent set run to completion
// (amg_core/graph.h:90-156 with max_iters == -1, the loop under PMIS and PMISc) and the CLJP selection loop
// (amg_core/ruge_stuben.h:373-478).  Both return the integers of the reference's sequential sweeps (DESIGN.md
// section 8h): every decision below is a function of the state at a kernel boundary, or is one that a stale read can
// only postpone.  State arrays hold one int per vertex; offsets are widened to 64 bits inside the kernels.
// The level chained in HBM (classical.hip) runs the same two loops on buffers its earlier stages left there.
#include "graph_dev.hpp"

using namespace amg;

namespace {

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

}   // namespace

// The two selection loops on buffers that are already in HBM: amg_mis_device and amg_cljp_device below run them on what
// they uploaded, the chained classical level (classical.hip) on what its earlier stages left there.
// mis_rounds_device: x: the states, in place; flag: one int of device memory; *rounds: rounds run.
// cljp_passes_device: S holds nnz entries, T = S^T in any row order; weight: the start weights, changed in place;
// splitting: n ints, written (1 = C, 0 = F); *passes: passes run.

int amg::fill_int_device(const char *what, long count, int value, int *out)
{
    hipLaunchKernelGGL(fill_int_kernel, grid_for(count), dim3(TB), 0, nullptr, count, value, out);
    LAUNCH_RETURN(what);
}

int amg::mis_rounds_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F, int *x, int *flag, int *rounds)
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

int amg::cljp_passes_device(int n, long nnz, const int *Sp, const int *Sj, const int *Tp, const int *Tj, double *weight, int *splitting,
                       int *passes)
{
    const size_t vbytes = sizeof(int) * (size_t)n, ebytes = sizeof(int) * (size_t)nnz;
    DBuf dSrow, dD, dhas, ddec, dmark, dopen;
    CHK(dSrow.alloc(ebytes)); CHK(dmark.alloc(ebytes));
    CHK(dD.alloc(vbytes)); CHK(dhas.alloc(vbytes)); CHK(ddec.alloc(vbytes));
    CHK(dopen.alloc(sizeof(int)));
    CHK(fill_int_device("cljp: state launch", n, U_NODE, splitting));
    CHK(fill_int_device("cljp: count launch", n, 0, ddec.i()));
    if (nnz > 0) {
        CHK(fill_int_device("cljp: edge mark launch", nnz, 1, dmark.i()));
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

extern "C" {

int amg_mis_device(int n, const int *Ap, const int *Aj, const double *y, int active, int C, int F, int *x, int *rounds,
                   double *times_ms)
{
    if (n < 0 || (n > 0 && (!y || !x))) { set_error("mis: bad arguments"); return AMG_EINVAL; }
    if (active == C || active == F) { set_error("mis: the active value must differ from C and F"); return AMG_EINVAL; }
    if (rounds) *rounds = 0;
    clear_times(times_ms);
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
    clear_times(times_ms);
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
