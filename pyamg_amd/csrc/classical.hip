// The row-parallel stages of the classical (Ruge-Stuben) setup on the device: classical strength
// of connection (amg_core/ruge_stuben.h:46-93), maximum_row_value (:110-130) and the two passes of direct interpolation
// (:497-595), as flat amg_core entries and chained into one level that stays in HBM from the upload of A to the download
// of the splitting and P (amg_classical_level_device / amg_classical_level_fetch).
// Every kernel gives one lane a whole row and walks it in stored order, so each sum is the reference's sequence of
// additions and the compaction (count, exclusive scan, fill) keeps the reference's entry order.  Nothing is contracted
// (-ffp-contract=off), nothing is guarded: infinities and NaNs are stored as they come.  Offsets are widened to 64 bits
// inside the kernels; every count fits an int because nnz < 2^31 is checked before the first launch.
// Below them extended+i interpolation (section 8j) and the chain of levels that stays in HBM (section 8k); the splitting
// loops are split.hip's, the transpose is transpose.hip's.
#include "graph_dev.hpp"
#include "hier.hpp"

#include <cfloat>
#include <memory>
#include <string>

using namespace amg;

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

// strength of A (device) into Sp (n + 1 offsets) and freshly allocated Sj, Sx; *nnz: entries kept
int strength_device(int n, double theta, const HbmCsr &A, long a_nnz, DBuf &Sp, DBuf &Sj, DBuf &Sx, long *nnz)
{
    DBuf threshold, count;
    CHK(threshold.alloc(sizeof(double) * (size_t)n));
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(strength_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, theta, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), threshold.d(), count.i());
    LAUNCH_CHECK("classical strength: count launch");
    CHK(offsets_from_counts("classical strength", n, count.i(), a_nnz, Sp, nnz));
    CHK(Sj.alloc(sizeof(int) * (size_t)*nnz));
    CHK(Sx.alloc(sizeof(double) * (size_t)*nnz));
    hipLaunchKernelGGL(strength_fill_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)A.p.i(), (const int *)A.j.i(),
                       (const double *)A.x.d(), (const double *)threshold.d(), (const int *)Sp.i(), Sj.i(), Sx.d());
    LAUNCH_CHECK("classical strength: fill launch");
    AMG_HIP(hipDeviceSynchronize());
    return 0;
}

// pass 1 and its scan: Bp (n + 1 offsets, allocated here); *nnz: the prolongator's entries, no bound (a lone C row stores one)
int interpolation_offsets_device(int n, const int *Sp, const int *Sj, const int *splitting, DBuf &Bp, long *nnz)
{
    DBuf count;
    CHK(count.alloc(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(interpolation_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, Sp, Sj, splitting, count.i());
    LAUNCH_CHECK("direct interpolation: count launch");
    return offsets_from_counts("direct interpolation", n, count.i(), -1, Bp, nnz);
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
constexpr int EXT_ROWS = TB / WAVE, EXT_CAP = 256, NO_POINT = 0x7fffffff;

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
    CHK(exclusive_scan(big.as<long>(), Wp.as<long>(), (size_t)n + 1));
    long wide = 0;
    CHK(last_offset(Wp.as<long>(), n, &wide));
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
        hipLaunchKernelGGL(truncate_count_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, max_per_row, (const int *)Pp.i(),
                           (const double *)Px.d(), count.i());
        LAUNCH_CHECK("extended interpolation: truncation count launch");
        CHK(offsets_from_counts("extended interpolation: truncation", n, count.i(), *nnz, Tp, &kept));
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

// (operator_facts_kernel, the pass over a product for its row order and its finiteness, is graph_dev.hpp's)
__global__ __launch_bounds__(TB) void count_ones_kernel(int n, const int *splitting, int *total)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    const int ones = __syncthreads_count(i < n && splitting[i] == 1);
    if (threadIdx.x == 0 && ones > 0) atomicAdd(total, ones);
}

}   // namespace

// The handles are hidden types: what the standard library instantiates on them stays out of the dynamic symbols.
// the columns and values of a prolongator, held for amg_extended_interpolation_fetch
struct __attribute__((visibility("hidden"))) amg_interpolation {
    long nnz = 0;
    DBuf Pj, Px;
};

// the result of one chained level, held for amg_classical_level_fetch
struct __attribute__((visibility("hidden"))) amg_classical {
    int n = 0;
    long s_nnz = 0, p_nnz = 0;
    DBuf Sp, Sj, Sx, splitting, Pp, Pj, Px;
    double times_ms[5] = {0, 0, 0, 0, 0};
};

// A chain of classical levels.  It owns the resident operator A (n x n, nnz entries, `reversed` as the level entries
// take it) and, between amg_classical_chain_level and amg_classical_chain_fetch, the level built from it: S, the
// splitting and P in `level`, R and the coarse operator C beside it.  The fetch moves C into A and drops the rest.
enum { CHAIN_IDLE = 0, CHAIN_BUILT = 1, CHAIN_REFUSED = 2 };
struct __attribute__((visibility("hidden"))) amg_classical_chain {
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
// the deleter of "drop the level on the way out": std::unique_ptr<amg_classical_chain, LevelDrop>
struct LevelDrop {
    void operator()(amg_classical_chain *c) const { c->drop_level(); }
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
        CHK(fill_int_device("classical level: state launch", n, -1, h.splitting.i()));
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

// what both level builders ask of their options before anything is uploaded
static int check_level_options(const char *who, int kind, int interpolation, int max_per_row, double theta, const double *r)
{
    if (kind != KIND_PMIS && kind != KIND_CLJP) return bad(who, "the splitting is 0 (PMIS) or 1 (CLJP)");
    if (interpolation != INTERP_DIRECT && interpolation != INTERP_EXTENDED_I)
        return bad(who, "the interpolation is 0 (direct) or 1 (extended+i)");
    if (max_per_row < 0 || (max_per_row > 0 && interpolation == INTERP_DIRECT))
        return bad(who, "max_per_row is 0, or positive with extended+i");
    if (!r) return bad(who, "no start values");
    if (!(theta >= 0.0 && theta <= 1.0)) return bad(who, "expected theta in [0, 1]");
    return 0;
}

// A level's splitting and P to the host and, where Sp is given, S as |S| with every row scaled by its largest entry
static int fetch_level(const char *who, amg_classical &h, int *splitting, int *Pp, int *Pj, double *Px, int *Sp, int *Sj, double *Sx)
{
    const size_t pbytes = sizeof(int) * ((size_t)h.n + 1);
    CHK(h.splitting.to_host(splitting, sizeof(int) * (size_t)h.n));
    CHK(h.Pp.to_host(Pp, pbytes));
    CHK(h.Pj.to_host(Pj, sizeof(int) * (size_t)h.p_nnz));
    CHK(h.Px.to_host(Px, sizeof(double) * (size_t)h.p_nnz));
    if (!Sp) return 0;
    if (h.s_nnz > 0 && (!Sj || !Sx)) return bad(who, "null array");
    hipLaunchKernelGGL(scale_rows_kernel, grid_for(h.n), dim3(TB), 0, nullptr, h.n, (const int *)h.Sp.i(), h.Sx.d());
    LAUNCH_CHECK("classical level: scaling launch");
    CHK(h.Sp.to_host(Sp, pbytes));
    CHK(h.Sj.to_host(Sj, sizeof(int) * (size_t)h.s_nnz));
    return h.Sx.to_host(Sx, sizeof(double) * (size_t)h.s_nnz);
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
    CHK(check_unique_columns(who, n, n, Ap, Aj));
    CHK(check_unique_columns(who, n, n, Sp, Sj));
    clear_times(times_ms, 2);
    std::unique_ptr<amg_interpolation> h(new amg_interpolation);
    if (n == 0) {
        Pp[0] = 0;
        *out = h.release();
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
    CHK(extended_interpolation_device(n, A, S.p.i(), S.j.i(), dsplit.i(), max_per_row, dPp, h->Pj, h->Px, &h->nnz));
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = timer.lap(); }
    CHK(dPp.to_host(Pp, sizeof(int) * ((size_t)n + 1)));
    *out = h.release();
    return 0;
}

int amg_extended_interpolation_fetch(amg_interpolation *h, int *Pj, double *Px)
{
    if (!h) return AMG_EINVAL;
    std::unique_ptr<amg_interpolation> own(h);
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
    if (n <= 0) return bad(who, "an empty operator");
    CHK(check_level_options(who, kind, interpolation, max_per_row, theta, r));
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    if (interpolation == INTERP_EXTENDED_I) CHK(check_unique_columns(who, n, n, Ap, Aj));
    CHK(require_device());
    LapClock timer;
    HbmCsr A;
    CHK(A.upload(n, Ap, Aj, Ax));
    DBuf dr;
    CHK(dr.from_host(r, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    // the handle owns what outlives this call; an early return frees it with everything it holds by then
    std::unique_ptr<amg_classical> own(new amg_classical);
    amg_classical &h = *own;
    h.times_ms[0] = timer.lap();
    int done = 0;
    CHK(classical_level_resident(n, A, Ap[n], theta, kind, reversed, dr, interpolation, max_per_row, h, &done, timer));

    sizes[0] = h.s_nnz;
    sizes[1] = h.p_nnz;
    if (rounds) *rounds = done;
    if (times_ms) std::copy(h.times_ms, h.times_ms + 5, times_ms);
    *out = own.release();
    return 0;
}

int amg_classical_level_fetch(amg_classical *h, int *splitting, int *Pp, int *Pj, double *Px, int *Sp, int *Sj, double *Sx,
                              double *times_ms)
{
    if (!h) return AMG_EINVAL;
    const char *who = "classical level fetch";
    std::unique_ptr<amg_classical> own(h);
    if (!splitting || !Pp || (h->p_nnz > 0 && (!Pj || !Px))) return bad(who, "null array");
    LapClock timer;
    CHK(fetch_level(who, *h, splitting, Pp, Pj, Px, Sp, Sj, Sx));
    if (times_ms) {
        std::copy(h->times_ms, h->times_ms + 5, times_ms);
        times_ms[5] = timer.lap();
    }
    return 0;
}

// ---- the chain: A_l, P_l, R_l, R_l A_l and A_{l+1} stay in HBM from the upload of A_0 on

int amg_classical_chain_begin(int n, const int *Ap, const int *Aj, const double *Ax, int reversed, amg_classical_chain **out)
{
    const char *who = "classical chain";
    if (!out) return bad(who, "bad arguments");
    *out = nullptr;
    if (n <= 0) return bad(who, "an empty operator");
    CHK(check_csr_arrays(who, n, n, Ap, n + 1, Aj, 0x7fffffff, Ax, 0x7fffffff));
    CHK(check_unique_columns(who, n, n, Ap, Aj));       // extended+i and the right-hand operand of R * A both need it
    CHK(require_device());
    LapClock timer;
    std::unique_ptr<amg_classical_chain> c(new amg_classical_chain);
    CHK(c->A.upload(n, Ap, Aj, Ax));
    AMG_HIP(hipDeviceSynchronize());
    c->n = n;
    c->nnz = Ap[n];
    c->reversed = reversed ? 1 : 0;
    c->upload_ms = timer.lap();
    *out = c.release();
    return 0;
}

int amg_classical_chain_level(amg_classical_chain *c, double theta, int kind, const double *r, int interpolation, int max_per_row,
                              long *sizes, int *flags, int *rounds, double *times_ms)
{
    const char *who = "classical chain";
    if (!c || !sizes || !flags) return bad(who, "bad arguments");
    if (c->n <= 0) return bad(who, "no resident operator");
    CHK(check_level_options(who, kind, interpolation, max_per_row, theta, r));
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
    std::unique_ptr<amg_classical_chain, LevelDrop> drop(c);
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
    TransposeRoute how;
    CHK(transpose_device(n, c->n_coarse, h.p_nnz, h.Pp.i(), h.Pj.i(), h.Px.d(), c->Rp, c->Rj, c->Rx, how));
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
    drop.release();
    return rc == 0 ? 0 : AMG_CHAIN_PRODUCT_REFUSED;
}

int amg_classical_chain_fetch(amg_classical_chain *c, int *splitting, int *Pp, int *Pj, double *Px, int *Rp, int *Rj, double *Rx,
                              int *Cp, int *Cj, double *Cx, int *Sp, int *Sj, double *Sx, double *times_ms)
{
    const char *who = "classical chain fetch";
    if (!c) return AMG_EINVAL;
    if (c->state == CHAIN_IDLE) { set_error("classical chain fetch: no level has been built"); return AMG_ESTATE; }
    // the level's buffers go whatever happens below; A_c becomes the resident operator only after a complete fetch
    std::unique_ptr<amg_classical_chain, LevelDrop> drop(c);
    const bool whole = c->state == CHAIN_BUILT;
    amg_classical &h = c->level;
    if (!splitting || !Pp || (h.p_nnz > 0 && (!Pj || !Px))) return bad(who, "null array");
    const bool want_R = whole && Rp, want_C = whole && Cp;      // a caller that finishes the level on the host wants neither
    if ((want_R && h.p_nnz > 0 && (!Rj || !Rx)) || (want_C && c->c_nnz > 0 && (!Cj || !Cx))) return bad(who, "null array");
    LapClock timer;
    const size_t cbytes = sizeof(int) * ((size_t)c->n_coarse + 1);
    CHK(fetch_level(who, h, splitting, Pp, Pj, Px, Sp, Sj, Sx));
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
