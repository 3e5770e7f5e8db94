// Energy-minimisation prolongation smoothing with CG (pyamg/aggregation/smooth.py:283-457 and :904-1177,
// amg_core/smoothed_aggregation.h:556-869) on the device, float64.
//
// Part 1: the flat entries incomplete_mat_mult_bsr, satisfy_constraints_helper and calc_BtB of
// include/amgcore_hip.h section 1.  One lane owns one scalar of the output and adds that scalar's products in the
// order the reference's loops reach them (its gemm, linalg.h:360-449, for the transpose flags of each call site);
// multiply and add round separately, nothing is added with atomics.
//
// Part 2: the whole CG iteration in HBM (amg_energy_smooth_device / amg_energy_fetch): R, Z, P, AP and T are value
// arrays on ONE fixed block pattern with sorted, unique rows.  Per iteration two reads come back to the host:
// (<R, Z>, the number of non-zero scalars of R) and <P, AP>.  DESIGN.md section 8f states the arithmetic.
// Root-node smoothing (amg_energy_smooth_rootnode_device) is that iteration with two additions:
// an initial fit T <- T - (T B_c - B_f) BtBinv B_c^T, and the single block of every root row set to the identity after
// the fit and after every update of T.
//
// Part 3: the flat entry truncate_rows_csr (smoothed_aggregation.h:898-960): one lane per row runs the reference's
// quicksort sequence on an explicit stack.
#include "graph_dev.hpp"

#include <memory>
#include <string>

using namespace amg;

namespace {

// block row of block e: the last row whose offset is <= e (empty rows are stepped over)
__device__ __forceinline__ int row_of_block(const int *Sp, int n_row, int e)
{
    int lo = 0, hi = n_row;                 // invariant: Sp[lo] <= e < Sp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (Sp[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- the three kernels
// smoothed_aggregation.h:797-869.  Lane = scalar (r, c) of block e of S, in block row i.  It adds, for jj ascending
// through row i of A and kk ascending through row Aj[jj] of B with Bj[kk] == Sj[e], the products A[jj](r, m) *
// B[kk](m, c) for m ascending, onto what Sx holds.  The reference keeps one pointer per column, set by the row's slots
// in order: where a row of S stores a column twice the later slot receives everything, so a lane whose column comes
// again later in its row leaves its scalar alone.  SORTED: the rows of B are sorted and unique (bisection);
// otherwise every entry of the row of B is compared.  Srow: the block row of every block, or null (bisection on Sp).
template <bool SORTED>
__global__ __launch_bounds__(TB) void imm_bsr_kernel(const int *Ap, const int *Aj, const double *Ax, const int *Bp, const int *Bj,
                                                      const double *Bx, const int *Sp, const int *Sj, const int *Srow, double *Sx,
                                                      int n_brow, int R, int N, int Cc, long n_scalar)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n_scalar) return;
    const int bs = R * Cc;
    const int e = (int)(t / bs), within = (int)(t % bs), r = within / Cc, c = within % Cc;
    const int i = Srow ? Srow[e] : row_of_block(Sp, n_brow, e);
    const int k = Sj[e];
    if (!SORTED) {
        for (int later = e + 1; later < Sp[i + 1]; ++later)
            if (Sj[later] == k) return;
    }
    double sum = Sx[t];
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
        const int j = Aj[jj];
        const double *a = Ax + ((long)jj * R + r) * N;
        const int lo = Bp[j], hi = Bp[j + 1];
        if (SORTED) {
            int l = lo, h = hi;                             // first kk in [lo, hi) with Bj[kk] >= k
            while (l < h) {
                const int mid = l + (h - l) / 2;
                if (Bj[mid] < k) l = mid + 1; else h = mid;
            }
            if (l < hi && Bj[l] == k) {
                const double *b = Bx + (long)l * N * Cc + c;
                for (int m = 0; m < N; ++m) sum += a[m] * b[(long)m * Cc];
            }
        } else {
            for (int kk = lo; kk < hi; ++kk) {
                if (Bj[kk] != k) continue;
                const double *b = Bx + (long)kk * N * Cc + c;
                for (int m = 0; m < N; ++m) sum += a[m] * b[(long)m * Cc];
            }
        }
    }
    Sx[t] = sum;
}

// UB = U * B for a BSR matrix U on the pattern and a dense row-major B (n_bcol * Cc rows, ND columns): lane = (scalar
// row, candidate d); from 0.0, blocks left to right, the columns of a block left to right.  FIT: the finished sum loses
// sub[t] in one subtraction (diff = T B_c - B_f of the initial fit).
template <bool FIT>
__global__ __launch_bounds__(TB) void block_row_product_kernel(const int *Sp, const int *Sj, const double *Ux, const double *B, double *UB,
                                                                const double *sub, int R, int Cc, int ND, long n_out)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n_out) return;
    const int d = (int)(t % ND);
    const long row = t / ND;
    const int i = (int)(row / R), r = (int)(row % R);
    double sum = 0.0;
    for (int jj = Sp[i]; jj < Sp[i + 1]; ++jj) {
        const double *u = Ux + ((long)jj * R + r) * Cc;
        const double *b = B + (long)Sj[jj] * Cc * ND + d;
        for (int c = 0; c < Cc; ++c) sum += u[c] * b[(long)c * ND];
    }
    UB[t] = FIT ? sum - sub[t] : sum;
}

// The single block of every root row becomes the identity (T = I_F * T + P_I on the fixed pattern): lane = one scalar
// of the n_bcol root blocks, root_at[j] being the block of column j's root row.  Square blocks of R x R.
__global__ __launch_bounds__(TB) void root_identity_kernel(const int *root_at, double *Tx, int R, long n)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n) return;
    const int bs = R * R;
    const int j = (int)(t / bs), within = (int)(t % bs);
    Tx[(long)root_at[j] * bs + within] = (within / R == within % R) ? 1.0 : 0.0;
}

// smoothed_aggregation.h:898-960.  Lane = row.  A row longer than k goes through the reference's quicksort on
// magnitudes: the middle element is moved to the left as pivot, entries strictly smaller than it are collected behind
// it, the pivot is put after them; the column indices move with the values.  The two parts are independent, so the
// recursion is a stack of ranges: the larger part is pushed and the smaller one is taken next, which bounds the stack
// by log2(len) + 1 <= 32 ranges for any row an int can index.  Then the first len - k entries become 0.0.
__global__ __launch_bounds__(TB) void truncate_rows_kernel(int n_row, int k, const int *Sp, int *Sj, double *Sx)
{
    const long row = (long)blockIdx.x * TB + threadIdx.x;
    if (row >= n_row) return;
    const int rowstart = Sp[row], rowend = Sp[row + 1];
    if (rowend - rowstart <= k) return;
    int stack_lo[32], stack_hi[32], top = 0;
    int left = rowstart, right = rowend - 1;
    for (;;) {
        while (left < right) {
            const int mid = (int)(((long)left + right) / 2);
            double tx = Sx[left]; Sx[left] = Sx[mid]; Sx[mid] = tx;
            int tj = Sj[left]; Sj[left] = Sj[mid]; Sj[mid] = tj;
            const double pivot = fabs(Sx[left]);
            int last = left;
            for (int i = left + 1; i <= right; ++i) {
                if (fabs(Sx[i]) < pivot) {
                    ++last;
                    tx = Sx[last]; Sx[last] = Sx[i]; Sx[i] = tx;
                    tj = Sj[last]; Sj[last] = Sj[i]; Sj[i] = tj;
                }
            }
            tx = Sx[left]; Sx[left] = Sx[last]; Sx[last] = tx;
            tj = Sj[left]; Sj[left] = Sj[last]; Sj[last] = tj;
            if (last - left < right - last) {
                if (top < 32) { stack_lo[top] = last + 1; stack_hi[top] = right; ++top; }
                right = last - 1;
            } else {
                if (top < 32) { stack_lo[top] = left; stack_hi[top] = last - 1; ++top; }
                left = last + 1;
            }
        }
        if (top == 0) break;
        --top;
        left = stack_lo[top]; right = stack_hi[top];
    }
    for (int jj = rowstart; jj < rowend - k; ++jj) Sx[jj] = 0.0;
}

// smoothed_aggregation.h:556-605.  Lane = scalar (r, c) of block e in block row i:
//   Cm(d, c) = sum_k BtBinv[i](d, k) * B[Sj[e] * Cc + c, k]          (k ascending from 0.0)
//   Sx -= sum_d UB[i](r, d) * Cm(d, c)                                (d ascending from 0.0)
// Bt is the conjugate of B, which for real values is B itself.
__global__ __launch_bounds__(TB) void satisfy_constraints_kernel(int R, int Cc, int n_brow, int ND, const double *Bt, const double *UB,
                                                                  const double *BtBinv, const int *Sp, const int *Sj, const int *Srow,
                                                                  double *Sx, long n_scalar)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n_scalar) return;
    const int bs = R * Cc;
    const int e = (int)(t / bs), within = (int)(t % bs), r = within / Cc, c = within % Cc;
    const int i = Srow ? Srow[e] : row_of_block(Sp, n_brow, e);
    const double *binv = BtBinv + (long)i * ND * ND;
    const double *b = Bt + ((long)Sj[e] * Cc + c) * ND;
    const double *ub = UB + ((long)i * R + r) * ND;
    double update = 0.0;
    for (int d = 0; d < ND; ++d) {
        double cm = 0.0;
        for (int k = 0; k < ND; ++k) cm += binv[d * ND + k] * b[k];
        update += ub[d] * cm;
    }
    Sx[t] = Sx[t] - update;
}

// smoothed_aggregation.h:656-734.  Lane = scalar (a, b) of BtB[i]; with m = min(a, b), n = max(a, b) it adds column
// off(m) + (n - m) of Bsq, off(m) = sum_{t < m} (ND - t), over the scalar columns of the row's blocks in stored order,
// from 0.0.  (Column-major or row-major is the same for the symmetric real block.)
__global__ __launch_bounds__(TB) void calc_BtB_kernel(int ND, int n_node, int Cc, const double *Bsq, int BsqCols, double *BtB, const int *Sp,
                                                       const int *Sj, long n_out)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n_out) return;
    const int sq = ND * ND;
    const int i = (int)(t / sq), within = (int)(t % sq), a = within / ND, b = within % ND;
    const int m = a < b ? a : b, n = a < b ? b : a;
    const int src = m * ND - (m * (m - 1)) / 2 + (n - m);
    double sum = 0.0;
    for (int jj = Sp[i]; jj < Sp[i + 1]; ++jj) {
        const long first = (long)Sj[jj] * Cc;
        for (int k = 0; k < Cc; ++k) sum += Bsq[(first + k) * BsqCols + src];
    }
    BtB[t] = sum;
}

// ---------------------------------------------------------------------------------------------- argument checks
bool rows_sorted_unique(const int *p, const int *j, int n)
{
    for (int i = 0; i < n; ++i)
        for (int e = p[i] + 1; e < p[i + 1]; ++e)
            if (j[e] <= j[e - 1]) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------- the CG iteration
// Elementwise steps; every scalar takes one multiply and one add, rounded separately.
__global__ __launch_bounds__(TB) void negate_kernel(double *x, long n)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t < n) x[t] = x[t] * -1.0;
}

// Z = R with scalar row s scaled by Dinv[s] (scale_rows)
__global__ __launch_bounds__(TB) void scale_rows_kernel(const double *Rx, const double *Dinv, const int *Srow, double *Zx, int R, int Cc,
                                                         long n)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n) return;
    const int bs = R * Cc;
    const int e = (int)(t / bs), r = (int)(t % bs) / Cc;
    Zx[t] = Rx[t] * Dinv[(long)Srow[e] * R + r];
}

// y = x + a * y  (P = Z + beta P)
__global__ __launch_bounds__(TB) void xpay_kernel(const double *x, double a, double *y, long n)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n) return;
    const double s = a * y[t];
    y[t] = x[t] + s;
}

// y = y + a * x  (T = T + alpha P;  R = R - alpha AP as y - (alpha x) with negative = 1)
__global__ __launch_bounds__(TB) void axpy_kernel(double a, const double *x, double *y, int negative, long n)
{
    const long t = (long)blockIdx.x * TB + threadIdx.x;
    if (t >= n) return;
    const double s = a * x[t];
    y[t] = negative ? y[t] - s : y[t] + s;
}

// The Frobenius inner product <X, Y> of two value arrays on the pattern, and the number of non-zero scalars of X.
// Level 0: lane = block row; its products are added in stored order from 0.0.  Then, at this and every further level,
// 256 consecutive values (0.0 past the end) are added by halving: v[t] += v[t + 128], v[t] += v[t + 64], ... v[0] +=
// v[1].  The launcher repeats the level until one value is left, so the order depends on the number of block rows
// alone.  in == null marks level 0.
__global__ __launch_bounds__(TB) void inner_product_level_kernel(const int *Sp, int bs, const double *X, const double *Y, const double *in,
                                                                  long n_in, double *out)
{
    __shared__ double v[TB], w[TB];
    const long item = (long)blockIdx.x * TB + threadIdx.x;
    double s = 0.0, nz = 0.0;
    if (item < n_in) {
        if (in) {
            s = in[2 * item];
            nz = in[2 * item + 1];
        } else {
            const long lo = (long)Sp[item] * bs, hi = (long)Sp[item + 1] * bs;
            for (long q = lo; q < hi; ++q) {
                const double x = X[q];
                s += x * Y[q];
                if (x != 0.0) nz += 1.0;
            }
        }
    }
    v[threadIdx.x] = s;
    w[threadIdx.x] = nz;
    __syncthreads();
    for (int stride = TB / 2; stride >= 1; stride /= 2) {
        if ((int)threadIdx.x < stride) {
            v[threadIdx.x] += v[threadIdx.x + stride];
            w[threadIdx.x] += w[threadIdx.x + stride];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[2 * (long)blockIdx.x] = v[0];
        out[2 * (long)blockIdx.x + 1] = w[0];
    }
}

}   // namespace

struct __attribute__((visibility("hidden"))) amg_energy {
    DBuf T;
    long n_scalar = 0;
};

namespace {

struct Smoother {
    int n_brow, n_bcol, R, Cc, ND, n_block;
    long n_scalar;
    DBuf Ap, Aj, Ax, Sp, Sj, Srow, Bc, BtBinv, Dinv, Rx, Zx, Px, APx, UB, part0, part1;
    DBuf RootAt, Bf;                // root-node smoothing: the root block of every column; the fine candidates of the fit
    bool rooted = false, fit = false;

    // <X, Y> and the count of non-zero scalars of X to the host: one read of two doubles
    int inner_product(const double *X, const double *Y, double host[2])
    {
        long n_in = n_brow;
        const double *in = nullptr;
        double *out = part0.d();
        for (;;) {
            const long n_out = (n_in + TB - 1) / TB;
            hipLaunchKernelGGL(inner_product_level_kernel, dim3((unsigned)n_out), dim3(TB), 0, nullptr, (const int *)Sp.i(), R * Cc, X, Y, in,
                               n_in, out);
            LAUNCH_CHECK("energy smoothing: inner product launch");
            if (n_out == 1) break;
            in = out;
            out = (out == part0.d()) ? part1.d() : part0.d();
            n_in = n_out;
        }
        AMG_HIP(hipMemcpy(host, out, 2 * sizeof(double), hipMemcpyDeviceToHost));
        return 0;
    }

    // U <- U - (U B_c) BtBinv B_c^T restricted to the pattern (Satisfy_Constraints, smooth.py:21-64)
    int project(double *Ux)
    {
        const long n_ub = (long)n_brow * R * ND;
        hipLaunchKernelGGL(block_row_product_kernel<false>, grid_for(n_ub), dim3(TB), 0, nullptr, (const int *)Sp.i(), (const int *)Sj.i(),
                           (const double *)Ux, (const double *)Bc.d(), UB.d(), (const double *)nullptr, R, Cc, ND, n_ub);
        LAUNCH_CHECK("energy smoothing: block-row product launch");
        hipLaunchKernelGGL(satisfy_constraints_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, R, Cc, n_brow, ND, (const double *)Bc.d(),
                           (const double *)UB.d(), (const double *)BtBinv.d(), (const int *)Sp.i(), (const int *)Sj.i(),
                           (const int *)Srow.i(), Ux, n_scalar);
        LAUNCH_CHECK("energy smoothing: constraint launch");
        return 0;
    }

    // the single block of every root row of T becomes the identity
    int root_identity(double *Tx)
    {
        const long n = (long)n_bcol * R * R;
        hipLaunchKernelGGL(root_identity_kernel, grid_for(n), dim3(TB), 0, nullptr, (const int *)RootAt.i(), Tx, R, n);
        LAUNCH_CHECK("energy smoothing: root identity launch");
        return 0;
    }

    // the initial fit of smooth.py:1142-1146 on the pattern: diff = T B_c - B_f, T <- T - diff BtBinv B_c^T
    int initial_fit(double *Tx)
    {
        const long n_ub = (long)n_brow * R * ND;
        hipLaunchKernelGGL(block_row_product_kernel<true>, grid_for(n_ub), dim3(TB), 0, nullptr, (const int *)Sp.i(), (const int *)Sj.i(),
                           (const double *)Tx, (const double *)Bc.d(), UB.d(), (const double *)Bf.d(), R, Cc, ND, n_ub);
        LAUNCH_CHECK("energy smoothing: fit difference launch");
        hipLaunchKernelGGL(satisfy_constraints_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, R, Cc, n_brow, ND, (const double *)Bc.d(),
                           (const double *)UB.d(), (const double *)BtBinv.d(), (const int *)Sp.i(), (const int *)Sj.i(),
                           (const int *)Srow.i(), Tx, n_scalar);
        LAUNCH_CHECK("energy smoothing: fit constraint launch");
        return 0;
    }

    // Sx += A * X on the pattern; X lives on the same pattern
    int product(const double *Xx, double *Sx)
    {
        hipLaunchKernelGGL(imm_bsr_kernel<true>, grid_for(n_scalar), dim3(TB), 0, nullptr, (const int *)Ap.i(), (const int *)Aj.i(),
                           (const double *)Ax.d(), (const int *)Sp.i(), (const int *)Sj.i(), Xx, (const int *)Sp.i(), (const int *)Sj.i(),
                           (const int *)Srow.i(), Sx, n_brow, R, R, Cc, n_scalar);
        LAUNCH_CHECK("energy smoothing: incomplete product launch");
        return 0;
    }

    // smooth.py:362-457 on the fixed pattern.  trace (or null): 2 values per started iteration, <R, Z> and <P, AP>.
    int run(double *Tx, int maxiter, double tol, int *iterations, double *trace)
    {
        const size_t bytes = sizeof(double) * (size_t)n_scalar;
        if (fit) {
            CHK(initial_fit(Tx));
            if (rooted) CHK(root_identity(Tx));
        }
        AMG_HIP(hipMemset(Rx.p, 0, bytes));
        CHK(product(Tx, Rx.d()));
        hipLaunchKernelGGL(negate_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, Rx.d(), n_scalar);
        LAUNCH_CHECK("energy smoothing: negation launch");
        CHK(project(Rx.d()));
        int it = 0;
        double oldsum = 0.0;
        while (it < maxiter) {
            hipLaunchKernelGGL(scale_rows_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, (const double *)Rx.d(), (const double *)Dinv.d(),
                               (const int *)Srow.i(), Zx.d(), R, Cc, n_scalar);
            LAUNCH_CHECK("energy smoothing: row scaling launch");
            double rz[2];
            CHK(inner_product(Rx.d(), Zx.d(), rz));
            const double newsum = rz[0];
            if (trace) { trace[2 * it] = newsum; trace[2 * it + 1] = 0.0; }
            if (rz[1] == 0.0) break;                        // R holds no non-zero
            if (newsum < tol) break;
            if (it == 0) {
                AMG_HIP(hipMemcpy(Px.p, Zx.p, bytes, hipMemcpyDeviceToDevice));
            } else {
                hipLaunchKernelGGL(xpay_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, (const double *)Zx.d(), newsum / oldsum, Px.d(),
                                   n_scalar);
                LAUNCH_CHECK("energy smoothing: direction launch");
            }
            oldsum = newsum;
            AMG_HIP(hipMemset(APx.p, 0, bytes));
            CHK(product(Px.d(), APx.d()));
            CHK(project(APx.d()));
            double pap[2];
            CHK(inner_product(Px.d(), APx.d(), pap));
            if (trace) trace[2 * it + 1] = pap[0];
            const double alpha = newsum / pap[0];
            hipLaunchKernelGGL(axpy_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, alpha, (const double *)Px.d(), Tx, 0, n_scalar);
            LAUNCH_CHECK("energy smoothing: update launch");
            if (rooted) CHK(root_identity(Tx));     // R, Z, P and AP keep what the arithmetic leaves in the root rows
            hipLaunchKernelGGL(axpy_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, alpha, (const double *)APx.d(), Rx.d(), 1, n_scalar);
            LAUNCH_CHECK("energy smoothing: update launch");
            ++it;
        }
        if (iterations) *iterations = it;
        AMG_HIP(hipDeviceSynchronize());
        return 0;
    }
};

}   // namespace

extern "C" {

// A (n_brow block rows, brow_A x bcol_A blocks), B (bcol_A x bcol_B blocks, Bp_size - 1 block rows) and S (brow_A x
// bcol_B blocks, n_bcol block columns) in BSR, rows in any order.  Sx += A * B on the pattern of S.  A row of S that
// stores a column twice: as in the reference, the later slot receives everything and the earlier one stays as it was.
int amgcore_incomplete_mat_mult_bsr_f64(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const double Ax[], int Ax_size,
                                        const int Bp[], int Bp_size, const int Bj[], int Bj_size, const double Bx[], int Bx_size,
                                        const int Sp[], int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size, int n_brow,
                                        int n_bcol, int brow_A, int bcol_A, int bcol_B)
{
    const std::string name = "incomplete_mat_mult_bsr";
    CHK(require_device());
    if (n_brow < 0 || n_bcol < 0 || brow_A < 1 || bcol_A < 1 || bcol_B < 1) { set_error(name + ": bad sizes"); return AMG_EINVAL; }
    const long bsA = (long)brow_A * bcol_A, bsB = (long)bcol_A * bcol_B, bsS = (long)brow_A * bcol_B;
    const int n_brow_B = Bp_size - 1;
    CHK(check_csr_offsets((name + ": A").c_str(), n_brow, Ap, Ap_size, Aj_size, Ax_size, bsA));
    CHK(check_csr_offsets((name + ": S").c_str(), n_brow, Sp, Sp_size, Sj_size, Sx_size, bsS));
    if (n_brow == 0 || Sp[n_brow] == 0) return 0;
    CHK(check_csr_offsets((name + ": B").c_str(), std::max(n_brow_B, 0), Bp, Bp_size, Bj_size, Bx_size, bsB));
    CHK(check_csr_columns((name + ": A").c_str(), n_brow, n_brow_B, Ap, Aj));
    CHK(check_csr_columns((name + ": B").c_str(), n_brow_B, n_bcol, Bp, Bj));
    CHK(check_csr_columns((name + ": S").c_str(), n_brow, n_bcol, Sp, Sj));
    const size_t na = (size_t)Ap[n_brow], nb = (size_t)Bp[n_brow_B], ns = (size_t)Sp[n_brow];
    if (!Sx || (na && !Ax) || (nb && !Bx)) { set_error(name + ": null array"); return AMG_EINVAL; }
    if ((long)ns * bsS >= 2147483647L) { set_error(name + ": S exceeds int32 indices"); return AMG_EINVAL; }
    DBuf dAp, dAj, dAx, dBp, dBj, dBx, dSp, dSj, dSx;
    CHK(dAp.from_host(Ap, sizeof(int) * ((size_t)n_brow + 1))); CHK(dAj.from_host(Aj, sizeof(int) * na));
    CHK(dAx.from_host(Ax, sizeof(double) * na * (size_t)bsA));
    CHK(dBp.from_host(Bp, sizeof(int) * ((size_t)n_brow_B + 1))); CHK(dBj.from_host(Bj, sizeof(int) * nb));
    CHK(dBx.from_host(Bx, sizeof(double) * nb * (size_t)bsB));
    CHK(dSp.from_host(Sp, sizeof(int) * ((size_t)n_brow + 1))); CHK(dSj.from_host(Sj, sizeof(int) * ns));
    CHK(dSx.from_host(Sx, sizeof(double) * ns * (size_t)bsS));
    const long n_scalar = (long)ns * bsS;
    hipLaunchKernelGGL(imm_bsr_kernel<false>, grid_for(n_scalar), dim3(TB), 0, nullptr, (const int *)dAp.i(), (const int *)dAj.i(),
                       (const double *)dAx.d(), (const int *)dBp.i(), (const int *)dBj.i(), (const double *)dBx.d(), (const int *)dSp.i(),
                       (const int *)dSj.i(), (const int *)nullptr, dSx.d(), n_brow, brow_A, bcol_A, bcol_B, n_scalar);
    LAUNCH_CHECK("incomplete_mat_mult_bsr launch");
    AMG_HIP(hipDeviceSynchronize());
    return dSx.to_host(Sx, sizeof(double) * (size_t)n_scalar);
}

// x = conj(B) (rows of NullDim values, one row per scalar column of S), y = U * B (num_block_rows * RowsPerBlock rows of
// NullDim values), z = BtBinv (num_block_rows blocks of NullDim x NullDim); Sx -= y_i * (z_i * x_j^T) block by block
int amgcore_satisfy_constraints_helper_f64(int RowsPerBlock, int ColsPerBlock, int num_block_rows, int NullDim, const double x[],
                                           int x_size, const double y[], int y_size, const double z[], int z_size, const int Sp[],
                                           int Sp_size, const int Sj[], int Sj_size, double Sx[], int Sx_size)
{
    const std::string name = "satisfy_constraints_helper";
    CHK(require_device());
    if (RowsPerBlock < 1 || ColsPerBlock < 1 || num_block_rows < 0 || NullDim < 1) { set_error(name + ": bad sizes"); return AMG_EINVAL; }
    const long bs = (long)RowsPerBlock * ColsPerBlock;
    CHK(check_csr_offsets((name + ": S").c_str(), num_block_rows, Sp, Sp_size, Sj_size, Sx_size, bs));
    if (num_block_rows == 0 || Sp[num_block_rows] == 0) return 0;
    const long per_col = (long)ColsPerBlock * NullDim;
    if (x_size < 0 || !x) { set_error(name + ": null array"); return AMG_EINVAL; }
    CHK(check_csr_columns((name + ": S").c_str(), num_block_rows, (int)std::min<long>(x_size / per_col, 2147483647L), Sp, Sj));
    if ((long)num_block_rows * RowsPerBlock * NullDim > y_size || (long)num_block_rows * NullDim * NullDim > z_size) {
        set_error(name + ": y or z shorter than the block rows need");
        return AMG_EINVAL;
    }
    if (!y || !z || !Sx) { set_error(name + ": null array"); return AMG_EINVAL; }
    const size_t ns = (size_t)Sp[num_block_rows];
    const long n_scalar = (long)ns * bs;
    if (n_scalar >= 2147483647L) { set_error(name + ": S exceeds int32 indices"); return AMG_EINVAL; }
    DBuf dx, dy, dz, dSp, dSj, dSx;
    CHK(dx.from_host(x, sizeof(double) * (size_t)x_size));
    CHK(dy.from_host(y, sizeof(double) * (size_t)num_block_rows * RowsPerBlock * NullDim));
    CHK(dz.from_host(z, sizeof(double) * (size_t)num_block_rows * NullDim * NullDim));
    CHK(dSp.from_host(Sp, sizeof(int) * ((size_t)num_block_rows + 1))); CHK(dSj.from_host(Sj, sizeof(int) * ns));
    CHK(dSx.from_host(Sx, sizeof(double) * (size_t)n_scalar));
    hipLaunchKernelGGL(satisfy_constraints_kernel, grid_for(n_scalar), dim3(TB), 0, nullptr, RowsPerBlock, ColsPerBlock, num_block_rows,
                       NullDim, (const double *)dx.d(), (const double *)dy.d(), (const double *)dz.d(), (const int *)dSp.i(),
                       (const int *)dSj.i(), (const int *)nullptr, dSx.d(), n_scalar);
    LAUNCH_CHECK("satisfy_constraints_helper launch");
    AMG_HIP(hipDeviceSynchronize());
    return dSx.to_host(Sx, sizeof(double) * (size_t)n_scalar);
}

// b = Bsq (one row of BsqCols = NullDim (NullDim + 1) / 2 products per scalar column of S); x[i] = B_i^T B_i over the
// columns of block row i of S, NullDim x NullDim
int amgcore_calc_BtB_f64(int NullDim, int Nnodes, int ColsPerBlock, const double b[], int b_size, int BsqCols, double x[], int x_size,
                         const int Sp[], int Sp_size, const int Sj[], int Sj_size)
{
    const std::string name = "calc_BtB";
    CHK(require_device());
    if (NullDim < 1 || Nnodes < 0 || ColsPerBlock < 1 || BsqCols != NullDim * (NullDim + 1) / 2) {
        set_error(name + ": bad sizes (BsqCols must be NullDim (NullDim + 1) / 2)");
        return AMG_EINVAL;
    }
    CHK(check_csr_offsets((name + ": S").c_str(), Nnodes, Sp, Sp_size, Sj_size, -1, 0));
    const long n_out = (long)Nnodes * NullDim * NullDim;
    if (n_out > x_size) { set_error(name + ": x shorter than Nnodes * NullDim * NullDim"); return AMG_EINVAL; }
    if (Nnodes == 0) return 0;
    if (!x || b_size < 0 || (Sp[Nnodes] > 0 && !b)) { set_error(name + ": null array"); return AMG_EINVAL; }
    CHK(check_csr_columns((name + ": S").c_str(), Nnodes, (int)std::min<long>(b_size / ((long)ColsPerBlock * BsqCols), 2147483647L), Sp, Sj));
    const size_t ns = (size_t)Sp[Nnodes];
    DBuf db, dx, dSp, dSj;
    CHK(db.from_host(b, sizeof(double) * (size_t)b_size));
    CHK(dx.alloc(sizeof(double) * (size_t)n_out));
    CHK(dSp.from_host(Sp, sizeof(int) * ((size_t)Nnodes + 1))); CHK(dSj.from_host(Sj, sizeof(int) * ns));
    hipLaunchKernelGGL(calc_BtB_kernel, grid_for(n_out), dim3(TB), 0, nullptr, NullDim, Nnodes, ColsPerBlock, (const double *)db.d(), BsqCols,
                       dx.d(), (const int *)dSp.i(), (const int *)dSj.i(), n_out);
    LAUNCH_CHECK("calc_BtB launch");
    AMG_HIP(hipDeviceSynchronize());
    return dx.to_host(x, sizeof(double) * (size_t)n_out);
}

// CG energy minimisation of smooth.py:283-457 for a real float64 operator.  A: n_brow x n_brow blocks of R x R (BSR on
// the host).  The pattern Sp/Sj: n_brow x n_bcol blocks of R x Cc, rows sorted and unique.  Tx: the tentative
// prolongator's values on the pattern.  Bc: the coarse candidates, n_bcol * Cc rows of ND values.  BtBinv: n_brow blocks
// of ND x ND.  Dinv: n_brow * R row weights.  Runs up to maxiter iterations, stopping when <R, Z> < tol or R holds no
// non-zero.  *out then holds the smoothed values for amg_energy_fetch; *iterations the finished iterations; trace (or
// null, else 2 * maxiter doubles): <R, Z> and <P, AP> of every started iteration; times_ms (or null): [0] upload,
// [1] the iterations.
// amg_energy_smooth_rootnode_device: the same with the root-node rules.  root_row: n_bcol entries, the block row of
// column j's root node -- distinct, in range, and the pattern's row there holds exactly one block, column j (AMG_EINVAL
// otherwise, before any launch); R == Cc.  Bf (or null: no initial fit): the fine candidates, n_brow * R rows of ND
// values; with it T <- T - (T B_c - B_f) BtBinv B_c^T runs first.  The root blocks are set to the identity after the fit
// and after every T += alpha P.
static int energy_smooth(int n_brow, int n_bcol, int R, int Cc, int ND, const int *Ap, const int *Aj, const double *Ax, const int *Sp,
                         const int *Sj, const double *Tx, const double *Bc, const double *BtBinv, const double *Dinv,
                         const int *root_row, const double *Bf, int maxiter, double tol, amg_energy **out, int *iterations,
                         double *trace, double *times_ms)
{
    const std::string name = "energy smoothing";
    if (!out || n_brow < 1 || n_bcol < 1 || R < 1 || Cc < 1 || ND < 1 || maxiter < 0) { set_error(name + ": bad arguments"); return AMG_EINVAL; }
    CHK(check_csr_offsets((name + ": A").c_str(), n_brow, Ap, n_brow + 1, 2147483647L, -1, 0));
    CHK(check_csr_offsets((name + ": pattern").c_str(), n_brow, Sp, n_brow + 1, 2147483647L, -1, 0));
    CHK(check_csr_columns((name + ": A").c_str(), n_brow, n_brow, Ap, Aj));
    CHK(check_csr_columns((name + ": pattern").c_str(), n_brow, n_bcol, Sp, Sj));
    if (Sp[n_brow] == 0) { set_error(name + ": empty pattern"); return AMG_EINVAL; }
    if (!rows_sorted_unique(Sp, Sj, n_brow)) { set_error(name + ": the pattern's rows must hold sorted, unique columns"); return AMG_EINVAL; }
    if (!Ax || !Tx || !Bc || !BtBinv || !Dinv) { set_error(name + ": null array"); return AMG_EINVAL; }
    std::vector<int> root_at;
    if (root_row) {
        if (R != Cc) { set_error(name + ": root-node smoothing needs square blocks (R == Cc)"); return AMG_EINVAL; }
        std::vector<char> taken((size_t)n_brow, 0);
        root_at.resize((size_t)n_bcol);
        for (int j = 0; j < n_bcol; ++j) {
            const int i = root_row[j];
            if (i < 0 || i >= n_brow) { set_error(name + ": root row outside the matrix"); return AMG_EINVAL; }
            if (taken[(size_t)i]) { set_error(name + ": two columns share a root row"); return AMG_EINVAL; }
            taken[(size_t)i] = 1;
            if (Sp[i + 1] - Sp[i] != 1 || Sj[Sp[i]] != j) {
                set_error(name + ": the pattern's row at a root must hold exactly one block, the root's own column");
                return AMG_EINVAL;
            }
            root_at[(size_t)j] = Sp[i];
        }
    } else if (Bf) {
        set_error(name + ": an initial fit needs root rows");
        return AMG_EINVAL;
    }
    Smoother s;
    s.n_brow = n_brow; s.n_bcol = n_bcol; s.R = R; s.Cc = Cc; s.ND = ND; s.n_block = Sp[n_brow];
    s.n_scalar = (long)s.n_block * R * Cc;
    if (s.n_scalar >= 2147483647L || (long)Ap[n_brow] * R * R >= 2147483647L) { set_error(name + ": exceeds int32 indices"); return AMG_EINVAL; }
    CHK(require_device());
    LapClock timer;
    std::vector<int> srow((size_t)s.n_block);
    for (int i = 0; i < n_brow; ++i)
        for (int e = Sp[i]; e < Sp[i + 1]; ++e) srow[(size_t)e] = i;
    const size_t np = sizeof(int) * ((size_t)n_brow + 1), vbytes = sizeof(double) * (size_t)s.n_scalar;
    CHK(s.Ap.from_host(Ap, np)); CHK(s.Aj.from_host(Aj, sizeof(int) * (size_t)Ap[n_brow]));
    CHK(s.Ax.from_host(Ax, sizeof(double) * (size_t)Ap[n_brow] * R * R));
    CHK(s.Sp.from_host(Sp, np)); CHK(s.Sj.from_host(Sj, sizeof(int) * (size_t)s.n_block));
    CHK(s.Srow.from_host(srow.data(), sizeof(int) * (size_t)s.n_block));
    CHK(s.Bc.from_host(Bc, sizeof(double) * (size_t)n_bcol * Cc * ND));
    CHK(s.BtBinv.from_host(BtBinv, sizeof(double) * (size_t)n_brow * ND * ND));
    CHK(s.Dinv.from_host(Dinv, sizeof(double) * (size_t)n_brow * R));
    if (root_row) { CHK(s.RootAt.from_host(root_at.data(), sizeof(int) * (size_t)n_bcol)); s.rooted = true; }
    if (Bf) { CHK(s.Bf.from_host(Bf, sizeof(double) * (size_t)n_brow * R * ND)); s.fit = true; }
    std::unique_ptr<amg_energy> h(new amg_energy);
    h->n_scalar = s.n_scalar;
    CHK(h->T.from_host(Tx, vbytes));
    CHK(s.Rx.alloc(vbytes)); CHK(s.Zx.alloc(vbytes)); CHK(s.Px.alloc(vbytes)); CHK(s.APx.alloc(vbytes));
    CHK(s.UB.alloc(sizeof(double) * (size_t)n_brow * R * ND));
    const size_t parts = 2 * sizeof(double) * (((size_t)n_brow + TB - 1) / TB);
    CHK(s.part0.alloc(parts)); CHK(s.part1.alloc(parts));
    if (hipDeviceSynchronize() != hipSuccess) { set_error(name + ": upload failed"); return AMG_ENODEV; }
    const double upload_ms = timer.lap();
    const int rc = s.run(h->T.d(), maxiter, tol, iterations, trace);
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = timer.lap(); }
    CHK(rc);
    *out = h.release();
    return 0;
}

int amg_energy_smooth_device(int n_brow, int n_bcol, int R, int Cc, int ND, const int *Ap, const int *Aj, const double *Ax, const int *Sp,
                             const int *Sj, const double *Tx, const double *Bc, const double *BtBinv, const double *Dinv, int maxiter,
                             double tol, amg_energy **out, int *iterations, double *trace, double *times_ms)
{
    return energy_smooth(n_brow, n_bcol, R, Cc, ND, Ap, Aj, Ax, Sp, Sj, Tx, Bc, BtBinv, Dinv, nullptr, nullptr, maxiter, tol, out,
                         iterations, trace, times_ms);
}

int amg_energy_smooth_rootnode_device(int n_brow, int n_bcol, int R, int Cc, int ND, const int *Ap, const int *Aj, const double *Ax,
                                      const int *Sp, const int *Sj, const double *Tx, const double *Bc, const double *BtBinv,
                                      const double *Dinv, const int *root_row, const double *Bf, int maxiter, double tol,
                                      amg_energy **out, int *iterations, double *trace, double *times_ms)
{
    if (!root_row) { set_error("energy smoothing: null root_row"); return AMG_EINVAL; }
    return energy_smooth(n_brow, n_bcol, R, Cc, ND, Ap, Aj, Ax, Sp, Sj, Tx, Bc, BtBinv, Dinv, root_row, Bf, maxiter, tol, out, iterations,
                         trace, times_ms);
}

// Sx, Sj: the CSR arrays of n_row rows; every row longer than k keeps its k entries of largest magnitude as the
// reference's quicksort leaves them (entries permuted within the row, the others 0.0), in place
int amgcore_truncate_rows_csr_f64(int n_row, int k, const int Sp[], int Sp_size, int Sj[], int Sj_size, double Sx[], int Sx_size)
{
    const std::string name = "truncate_rows_csr";
    CHK(require_device());
    if (n_row < 0 || k < 0) { set_error(name + ": bad sizes"); return AMG_EINVAL; }
    CHK(check_csr_offsets((name + ": S").c_str(), n_row, Sp, Sp_size, std::min(Sj_size, Sx_size), -1, 0));
    if (n_row == 0 || Sp[n_row] == 0) return 0;
    if (!Sj || !Sx) { set_error(name + ": null array"); return AMG_EINVAL; }
    const size_t nnz = (size_t)Sp[n_row];
    DBuf dSp, dSj, dSx;
    CHK(dSp.from_host(Sp, sizeof(int) * ((size_t)n_row + 1)));
    CHK(dSj.from_host(Sj, sizeof(int) * nnz));
    CHK(dSx.from_host(Sx, sizeof(double) * nnz));
    hipLaunchKernelGGL(truncate_rows_kernel, grid_for(n_row), dim3(TB), 0, nullptr, n_row, k, (const int *)dSp.i(), dSj.i(), dSx.d());
    LAUNCH_CHECK("truncate_rows_csr launch");
    AMG_HIP(hipDeviceSynchronize());
    CHK(dSj.to_host(Sj, sizeof(int) * nnz));
    return dSx.to_host(Sx, sizeof(double) * nnz);
}

// the smoothed values on the pattern to the host; releases the result
int amg_energy_fetch(amg_energy *h, double *Tx)
{
    if (!h) return AMG_EINVAL;
    std::unique_ptr<amg_energy> own(h);
    if (!Tx || hipMemcpy(Tx, h->T.p, sizeof(double) * (size_t)h->n_scalar, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("energy smoothing: download failed");
        return AMG_ENODEV;
    }
    return 0;
}

}   // extern "C"
