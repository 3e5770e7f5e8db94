// The flat amg_core table (include/amgcore_hip.h, section 1) for float32, complex64 and complex128 values:
// the reference instantiates its relaxation kernels for float, double, complex<float> and complex<double>
// (pyamg/amg_core/amg_core.i:139-144); the float64 entries live in capi.hip, ne.hip and schwarz.hip,
// specialised for the resident hierarchy.  These kernels are templated on the value type T and
// spell out every expression of relaxation.h with the operand types it has there, through the scalar
// rules of scalar.hpp, so the results are the reference's bit for bit.
//
// Shapes: the SpMV and Jacobi rows run in 256-row workgroups that stage their entries' products in LDS
// (coalesced) and sum every row left to right in stored order; every Gauss-Seidel-type sweep runs by
// dependency levels (one launch per level, one thread per task) built by the index-only builders the
// float64 path uses (build_levels, ne_touch_levels, schwarz_levels), which reproduce the sequential
// loop exactly.
#include "hier.hpp"
#include "flat.hpp"
#include "scalar.hpp"
#include "typed_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace amg;
using namespace amg::sc;
using namespace amg::tk;

namespace {

template <class T> T *tp(const DBuf &b) { return (T *)b.p; }

// ----------------------------------------------------------------------------------------------- kernels

// relaxation.h:529-561, one dependency level: delta = ((b_i - a_i . x) Dinv_i) omega; x += conj(a_i) delta
template <class T, class F>
__global__ void gs_ne_level(const int *Ap, const int *Aj, const T *Ax, T *x, const T *b, const T *Dinv, F omega,
                            const int *rows, int count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = rows[t];
    T delta = from_real<T>(0.0);
    for (int j = Ap[i]; j < Ap[i + 1]; ++j) delta = add(delta, mul(Ax[j], x[Aj[j]]));
    delta = mulr(mul(sub(b[i], delta), Dinv[i]), omega);
    for (int j = Ap[i]; j < Ap[i + 1]; ++j) x[Aj[j]] = add(x[Aj[j]], mul(conj(Ax[j]), delta));
}

// relaxation.h:594-631, one dependency level (A by columns): delta = (conj(a_i) . r) (Dinv_i omega)
template <class T, class F>
__global__ void gs_nr_level(const int *Ap, const int *Aj, const T *Ax, T *x, T *r, const T *Dinv, F omega,
                            const int *cols, int count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = cols[t];
    T delta = from_real<T>(0.0);
    for (int j = Ap[i]; j < Ap[i + 1]; ++j) delta = add(delta, mul(conj(Ax[j]), r[Aj[j]]));
    delta = mul(delta, mulr(Dinv[i], omega));
    x[i] = add(x[i], delta);
    for (int j = Ap[i]; j < Ap[i + 1]; ++j) r[Aj[j]] = sub(r[Aj[j]], mul(delta, Ax[j]));
}

// relaxation.h:465-496 through the transposed pattern: temp[c] gathers (omega conj(a)) delta[row] in the
// reference's (row, position) order, starting from 0 where c is a swept row
template <class T>
__global__ void jacobi_ne_gather(const int *Tp, const int *Trow, const T *Tval, const T *delta, const T *omega,
                                 T *temp, const unsigned char *in_range, int n)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const T w = omega[0];
    T acc = in_range[c] ? from_real<T>(0.0) : temp[c];
    for (int k = Tp[c]; k < Tp[c + 1]; ++k) acc = add(acc, mul(mul(w, conj(Tval[k])), delta[Trow[k]]));
    temp[c] = acc;
}
template <class T>
__global__ void add_rows(T *x, const T *temp, const int *rows, int count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int i = rows[t];
    x[i] = add(x[i], temp[i]);
}

// relaxation.h:935-1007, one dependency level, one thread per subdomain; r lives in scratch[Sp[d] ..)
template <class T>
__global__ void schwarz_level(const int *Ap, const int *Aj, const T *Ax, T *x, const T *b, const T *Tx, const int *Tp,
                              const int *Sj, const int *Sp, T *scratch, const int *doms, int count)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int d = doms[t];
    const int s0 = Sp[d], m = Sp[d + 1] - s0;
    T *r = scratch + s0;
    for (int c = 0; c < m; ++c) {
        const int row = Sj[s0 + c];
        T acc = from_real<T>(0.0);
        for (int jj = Ap[row]; jj < Ap[row + 1]; ++jj) acc = sub(acc, mul(Ax[jj], x[Aj[jj]]));
        r[c] = add(acc, b[row]);
    }
    const T *M = Tx + Tp[d];
    for (int i = 0; i < m; ++i) {
        T acc = from_real<T>(0.0);
        for (int k = 0; k < m; ++k) acc = add(acc, mul(M[(long)i * m + k], r[k]));
        const int row = Sj[s0 + i];
        x[row] = add(x[row], acc);
    }
}

// ----------------------------------------------------------------------------------------------- host side

int blocks_for(long n, int per) { return (int)((n + per - 1) / per); }

// Ap nondecreasing from 0 within Aj/Ax, every index in [0, ncols): nothing a kernel reads can leave its array
int check_pattern(const int *Ap, int nrows, const int *Aj, int ncols)
{
    if (!Ap || Ap[0] < 0) { set_error("bad Ap"); return AMG_EINVAL; }
    for (int i = 0; i < nrows; ++i)
        if (Ap[i + 1] < Ap[i]) { set_error("Ap is not nondecreasing"); return AMG_EINVAL; }
    for (int k = Ap[0]; k < Ap[nrows]; ++k)
        if (Aj[k] < 0 || Aj[k] >= ncols) { set_error("column index out of range"); return AMG_EINVAL; }
    return 0;
}

template <class T>
int put(DBuf &d, const T *src, long count)
{
    return d.from_host(src, sizeof(T) * (size_t)std::max(0L, count));
}
template <class T>
int get(const DBuf &d, T *dst, long count)
{
    return d.to_host(dst, sizeof(T) * (size_t)std::max(0L, count));
}

// the device copies of a matrix's pattern and values (nnz entries of `per` values each)
template <class T>
struct DevMat {
    DBuf Ap, Aj, Ax;
    int load(const int *hAp, int nrows, const int *hAj, const T *hAx, long per)
    {
        const long nnz = hAp[nrows];
        CHK(put(Ap, hAp, nrows + 1L));
        CHK(put(Aj, hAj, nnz));
        return put(Ax, hAx, nnz * per);
    }
};

// Gauss-Seidel-type sweep: tasks run level by level (level_ptr), `order` lists them in level order
template <class Launch>
int run_levels(const std::vector<int> &level_ptr, Launch launch)
{
    for (size_t l = 0; l + 1 < level_ptr.size(); ++l) {
        const int cnt = level_ptr[l + 1] - level_ptr[l];
        if (cnt > 0) CHK(launch(level_ptr[l], cnt));
    }
    return 0;
}

// tasks (rows of the pattern) in dependency-level order
int level_rows(int n, const int *Ap, const int *Aj, const std::vector<int> &tasks, std::vector<int> &level_ptr,
               std::vector<int> &rows)
{
    std::vector<int> order;
    CHK(build_levels(n, Ap, Aj, tasks.data(), (int)tasks.size(), level_ptr, order));
    rows.resize(order.size());
    for (size_t k = 0; k < order.size(); ++k) rows[k] = tasks[(size_t)order[k]];
    return 0;
}

template <class T>
int gs_csr(const int *Ap, int Ap_size, const int *Aj, const T *Ax, T *x, int x_size, const T *b, int b_size,
           const std::vector<int> &tasks)
{
    const int n = Ap_size - 1;
    if (tasks.empty()) return 0;
    CHK(check_pattern(Ap, n, Aj, x_size));
    std::vector<int> lp, rows;
    CHK(level_rows(n, Ap, Aj, tasks, lp, rows));
    DevMat<T> A;
    DBuf dx, db, dr;
    CHK(A.load(Ap, n, Aj, Ax, 1));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dr, rows.data(), (long)rows.size()));
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL(gs_level<T>, dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr, A.Ap.i(),
                           A.Aj.i(), tp<T>(A.Ax), tp<T>(dx), tp<T>(db), dr.i() + off, cnt);
        return launched("gauss_seidel level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    return get(dx, x, x_size);
}

// the rows of a CSR matrix run through rows_stream in workgroups of ROWS_PER_WG
template <class T, int MODE>
int launch_rows(int lo, int hi, int start, int step, const DevMat<T> &A, const T *v, const T *b, const T *omega, T *out)
{
    if (hi <= lo) return 0;
    hipLaunchKernelGGL((rows_stream<T, MODE>), dim3(blocks_for(hi - lo, ROWS_PER_WG)), dim3(ROWS_PER_WG), 0, nullptr,
                       lo, hi, start, step, A.Ap.i(), A.Aj.i(), tp<T>(A.Ax), v, b, omega, out);
    return launched("rows_stream");
}

}  // namespace

// ----------------------------------------------------------------------------------------------- entries
namespace amg {
namespace typed {

template <class T>
int gauss_seidel(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                 int x_size, const T b[], int b_size, int row_start, int row_stop, int row_step)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    std::vector<int> tasks;
    CHK(sweep_rows(row_start, row_stop, row_step, std::min(Ap_size - 1, std::min(x_size, b_size)), tasks));
    return gs_csr(Ap, Ap_size, Aj, Ax, x, x_size, b, b_size, tasks);
}

template <class T>
int gauss_seidel_indexed(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                         int x_size, const T b[], int b_size, const int Id[], int Id_size, int row_start,
                         int row_stop, int row_step)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    std::vector<int> pos, tasks;
    CHK(sweep_rows(row_start, row_stop, row_step, Id_size, pos));
    const int n = std::min(Ap_size - 1, std::min(x_size, b_size));
    tasks.resize(pos.size());
    for (size_t t = 0; t < pos.size(); ++t) {
        tasks[t] = Id[pos[t]];
        if (tasks[t] < 0 || tasks[t] >= n) { set_error("Id entry out of range"); return AMG_EINVAL; }
    }
    return gs_csr(Ap, Ap_size, Aj, Ax, x, x_size, b, b_size, tasks);
}

template <class T>
int bsr_gauss_seidel(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                     int x_size, const T b[], int b_size, int row_start, int row_stop, int row_step, int blocksize)
{
    CHK(require_device());
    if (blocksize < 1) { set_error("blocksize < 1"); return AMG_EINVAL; }
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, blocksize * blocksize));
    const int nb = Ap_size - 1;
    std::vector<int> tasks;
    CHK(sweep_rows(row_start, row_stop, row_step, std::min(nb, std::min(x_size, b_size) / blocksize), tasks));
    if (tasks.empty()) return 0;
    CHK(check_pattern(Ap, nb, Aj, x_size / blocksize));
    std::vector<int> lp, rows;
    CHK(level_rows(nb, Ap, Aj, tasks, lp, rows));
    DevMat<T> A;
    DBuf dx, db, dr;
    CHK(A.load(Ap, nb, Aj, Ax, (long)blocksize * blocksize));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dr, rows.data(), (long)rows.size()));
    const int rev = row_step < 0 ? 1 : 0;
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL((bsr_point_level<T, false>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr,
                           A.Ap.i(), A.Aj.i(), tp<T>(A.Ax), tp<T>(dx), tp<T>(dx), tp<T>(db), (const T *)nullptr,
                           dr.i() + off, cnt, blocksize, rev);
        return launched("bsr_gauss_seidel level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    return get(dx, x, x_size);
}

template <class T>
int jacobi(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[], int x_size,
           const T b[], int b_size, T temp[], int temp_size, int row_start, int row_stop, int row_step,
           const T omega[], int omega_size)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    if (omega_size < 1 || !omega) { set_error("omega must be a length-1 array"); return AMG_EINVAL; }
    const int n = Ap_size - 1;
    std::vector<int> rows;
    CHK(sweep_rows(row_start, row_stop, row_step, std::min(n, std::min(std::min(x_size, b_size), temp_size)), rows));
    if (rows.empty()) return 0;
    CHK(check_pattern(Ap, n, Aj, temp_size));
    const int lo = std::min(rows.front(), rows.back()), hi = std::max(rows.front(), rows.back()) + 1;
    DevMat<T> A;
    DBuf dx, db, dt, dw;
    CHK(A.load(Ap, n, Aj, Ax, 1));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dt, temp, temp_size));
    CHK(put(dw, omega, 1));
    hipLaunchKernelGGL(copy_sweep<T>, dim3(blocks_for(hi - lo, 256)), dim3(256), 0, nullptr, lo, hi, row_start,
                       row_step, (const T *)tp<T>(dx), tp<T>(dt));    // relaxation.h:216-218
    CHK(launched("jacobi copy"));
    CHK((launch_rows<T, ROWS_JACOBI>(lo, hi, row_start, row_step, A, tp<T>(dt), tp<T>(db), tp<T>(dw), tp<T>(dx))));
    AMG_HIP(hipDeviceSynchronize());
    CHK(get(dx, x, x_size));
    return get(dt, temp, temp_size);
}

template <class T>
int bsr_jacobi(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
               int x_size, const T b[], int b_size, T temp[], int temp_size, int row_start, int row_stop,
               int row_step, int blocksize, const T omega[], int omega_size)
{
    CHK(require_device());
    if (blocksize < 1) { set_error("blocksize < 1"); return AMG_EINVAL; }
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, blocksize * blocksize));
    if (omega_size < 1 || !omega) { set_error("omega must be a length-1 array"); return AMG_EINVAL; }
    if (row_step < 0) {
        // relaxation.h:303-305 never terminates for a negative step
        set_error("bsr_jacobi: backward sweeps are not defined by the reference");
        return AMG_EINVAL;
    }
    const int nb = Ap_size - 1;
    std::vector<int> rows;
    CHK(sweep_rows(row_start, row_stop, row_step,
                   std::min(nb, std::min(std::min(x_size, b_size), temp_size) / blocksize), rows));
    if (rows.empty()) return 0;
    CHK(check_pattern(Ap, nb, Aj, temp_size / blocksize));
    const long ncopy = (long)std::abs(row_stop - row_start) * blocksize;     // relaxation.h:303-305
    if (ncopy > std::min(x_size, temp_size)) { set_error("temp/x too short"); return AMG_EINVAL; }
    DevMat<T> A;
    DBuf dx, db, dt, dw, dr;
    CHK(A.load(Ap, nb, Aj, Ax, (long)blocksize * blocksize));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dt, temp, temp_size));
    CHK(put(dw, omega, 1));
    CHK(put(dr, rows.data(), (long)rows.size()));
    if (ncopy) AMG_HIP(hipMemcpy(dt.p, dx.p, sizeof(T) * (size_t)ncopy, hipMemcpyDeviceToDevice));
    const int cnt = (int)rows.size();
    hipLaunchKernelGGL((bsr_point_level<T, true>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr,
                       A.Ap.i(), A.Aj.i(), tp<T>(A.Ax), tp<T>(dt), tp<T>(dx), tp<T>(db), tp<T>(dw), dr.i(), cnt,
                       blocksize, 0);
    CHK(launched("bsr_jacobi"));
    AMG_HIP(hipDeviceSynchronize());
    CHK(get(dx, x, x_size));
    return get(dt, temp, temp_size);
}

template <class T>
int block_jacobi(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                 int x_size, const T b[], int b_size, const T Tx[], int Tx_size, T temp[], int temp_size,
                 int row_start, int row_stop, int row_step, const T omega[], int omega_size, int blocksize)
{
    CHK(require_device());
    if (blocksize < 1) { set_error("blocksize < 1"); return AMG_EINVAL; }
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, blocksize * blocksize));
    if (omega_size < 1 || !omega) { set_error("omega must be a length-1 array"); return AMG_EINVAL; }
    const int nb = Ap_size - 1;
    std::vector<int> rows;
    CHK(sweep_rows(row_start, row_stop, row_step,
                   std::min(nb, std::min(std::min(x_size, b_size), temp_size) / blocksize), rows));
    if (rows.empty()) return 0;
    if ((long)nb * blocksize * blocksize > Tx_size) { set_error("Dinv too short"); return AMG_EINVAL; }
    CHK(check_pattern(Ap, nb, Aj, temp_size / blocksize));
    DevMat<T> A;
    DBuf dx, db, dt, dd, dw, dr, ds;
    CHK(A.load(Ap, nb, Aj, Ax, (long)blocksize * blocksize));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dt, temp, temp_size));
    CHK(put(dd, Tx, (long)nb * blocksize * blocksize));
    CHK(put(dw, omega, 1));
    CHK(put(dr, rows.data(), (long)rows.size()));
    CHK(ds.alloc(sizeof(T) * (size_t)nb * blocksize));
    // relaxation.h:686-688: temp = x on the swept block rows, as point rows of a strided sweep
    const int lo = std::min(rows.front(), rows.back()), hi = std::max(rows.front(), rows.back()) + 1;
    for (int k = 0; k < blocksize; ++k) {
        // point row r*bs + k of block row r: the sweep start*bs + k, step*bs
        hipLaunchKernelGGL(copy_sweep<T>, dim3(blocks_for((long)(hi - lo) * blocksize, 256)), dim3(256), 0, nullptr,
                           lo * blocksize, hi * blocksize, row_start * blocksize + k, row_step * blocksize,
                           (const T *)tp<T>(dx), tp<T>(dt));
        CHK(launched("block_jacobi copy"));
    }
    const int cnt = (int)rows.size();
    hipLaunchKernelGGL((block_level<T, true>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr, A.Ap.i(),
                       A.Aj.i(), tp<T>(A.Ax), tp<T>(dd), tp<T>(dt), tp<T>(dx), tp<T>(db), tp<T>(dw), tp<T>(ds), dr.i(),
                       cnt, blocksize);
    CHK(launched("block_jacobi"));
    AMG_HIP(hipDeviceSynchronize());
    CHK(get(dx, x, x_size));
    return get(dt, temp, temp_size);
}

template <class T>
int block_gauss_seidel(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                       int x_size, const T b[], int b_size, const T Tx[], int Tx_size, int row_start, int row_stop,
                       int row_step, int blocksize)
{
    CHK(require_device());
    if (blocksize < 1) { set_error("blocksize < 1"); return AMG_EINVAL; }
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, blocksize * blocksize));
    const int nb = Ap_size - 1;
    std::vector<int> tasks;
    CHK(sweep_rows(row_start, row_stop, row_step, std::min(nb, std::min(x_size, b_size) / blocksize), tasks));
    if (tasks.empty()) return 0;
    if ((long)nb * blocksize * blocksize > Tx_size) { set_error("Dinv too short"); return AMG_EINVAL; }
    CHK(check_pattern(Ap, nb, Aj, x_size / blocksize));
    std::vector<int> lp, rows;
    CHK(level_rows(nb, Ap, Aj, tasks, lp, rows));
    DevMat<T> A;
    DBuf dx, db, dd, dr, ds;
    CHK(A.load(Ap, nb, Aj, Ax, (long)blocksize * blocksize));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dd, Tx, (long)nb * blocksize * blocksize));
    CHK(put(dr, rows.data(), (long)rows.size()));
    CHK(ds.alloc(sizeof(T) * (size_t)nb * blocksize));
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL((block_level<T, false>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr,
                           A.Ap.i(), A.Aj.i(), tp<T>(A.Ax), tp<T>(dd), tp<T>(dx), tp<T>(dx), tp<T>(db),
                           (const T *)nullptr, tp<T>(ds), dr.i() + off, cnt, blocksize);
        return launched("block_gauss_seidel level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    return get(dx, x, x_size);
}

// a compact pattern of the listed tasks (row t = row tasks[t] of A): the touch levels of ne.hip take tasks 0..n-1
int task_touch_levels(int nvec, const int *Ap, const int *Aj, const std::vector<int> &tasks,
                      std::vector<int> &level_ptr, std::vector<int> &order)
{
    std::vector<int> cp(tasks.size() + 1, 0), cj;
    for (size_t t = 0; t < tasks.size(); ++t) {
        for (int k = Ap[tasks[t]]; k < Ap[tasks[t] + 1]; ++k) cj.push_back(Aj[k]);
        cp[t + 1] = (int)cj.size();
    }
    std::vector<int> pos;
    CHK(ne_touch_levels(nvec, cp.data(), cj.data(), (int)tasks.size(), level_ptr, pos));
    order.resize(pos.size());
    for (size_t k = 0; k < pos.size(); ++k) order[k] = tasks[(size_t)pos[k]];
    return 0;
}

template <class T, class F>
int gauss_seidel_ne(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                    int x_size, const T b[], int b_size, int row_start, int row_stop, int row_step, const T Tx[],
                    int Tx_size, F omega)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    std::vector<int> tasks, lp, order;
    CHK(sweep_rows(row_start, row_stop, row_step, std::min(n, std::min(b_size, Tx_size)), tasks));
    if (tasks.empty()) return 0;
    CHK(check_pattern(Ap, n, Aj, x_size));
    CHK(task_touch_levels(x_size, Ap, Aj, tasks, lp, order));
    DevMat<T> A;
    DBuf dx, db, dT, dord;
    CHK(A.load(Ap, n, Aj, Ax, 1));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dT, Tx, Tx_size));
    CHK(put(dord, order.data(), (long)order.size()));
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL((gs_ne_level<T, F>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr, A.Ap.i(),
                           A.Aj.i(), tp<T>(A.Ax), tp<T>(dx), tp<T>(db), tp<T>(dT), omega, dord.i() + off, cnt);
        return launched("gauss_seidel_ne level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    return get(dx, x, x_size);
}

template <class T, class F>
int gauss_seidel_nr(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[],
                    int x_size, T z[], int z_size, int col_start, int col_stop, int col_step, const T Tx[],
                    int Tx_size, F omega)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    std::vector<int> tasks, lp, order;
    CHK(sweep_rows(col_start, col_stop, col_step, std::min(n, std::min(x_size, Tx_size)), tasks));
    if (tasks.empty()) return 0;
    CHK(check_pattern(Ap, n, Aj, z_size));
    CHK(task_touch_levels(z_size, Ap, Aj, tasks, lp, order));
    DevMat<T> A;
    DBuf dx, dz, dT, dord;
    CHK(A.load(Ap, n, Aj, Ax, 1));
    CHK(put(dx, x, x_size));
    CHK(put(dz, z, z_size));
    CHK(put(dT, Tx, Tx_size));
    CHK(put(dord, order.data(), (long)order.size()));
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL((gs_nr_level<T, F>), dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr, A.Ap.i(),
                           A.Aj.i(), tp<T>(A.Ax), tp<T>(dx), tp<T>(dz), tp<T>(dT), omega, dord.i() + off, cnt);
        return launched("gauss_seidel_nr level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    CHK(get(dx, x, x_size));
    return get(dz, z, z_size);
}

template <class T>
int jacobi_ne(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size, T x[], int x_size,
              const T b[], int b_size, const T Tx[], int Tx_size, T temp[], int temp_size, int row_start,
              int row_stop, int row_step, const T omega[], int omega_size)
{
    (void)b; (void)b_size;
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    if (omega_size < 1 || !omega) { set_error("omega must be a length-1 array"); return AMG_EINVAL; }
    if (row_step <= 0) { set_error("jacobi_ne: row_step must be positive (relaxation.h:481 uses '<')"); return AMG_EINVAL; }
    const int n = Ap_size - 1;
    std::vector<int> rows;
    for (long i = row_start; i < row_stop; i += row_step) {
        if (i < 0 || i >= n || i >= x_size || i >= temp_size || i >= Tx_size) { set_error("sweep leaves the matrix"); return AMG_EINVAL; }
        rows.push_back((int)i);
    }
    if (rows.empty()) return 0;
    CHK(check_pattern(Ap, n, Aj, temp_size));
    // transposed pattern of the swept rows, contributions in (row, position) order
    std::vector<unsigned char> in_range((size_t)temp_size, 0);
    for (int i : rows) in_range[i] = 1;
    std::vector<int> Tp((size_t)temp_size + 1, 0);
    for (int i : rows)
        for (int j = Ap[i]; j < Ap[i + 1]; ++j) Tp[Aj[j] + 1]++;
    for (int c = 0; c < temp_size; ++c) Tp[c + 1] += Tp[c];
    std::vector<int> Trow((size_t)Tp[temp_size]);
    std::vector<T> Tval((size_t)Tp[temp_size]);
    std::vector<int> cur(Tp.begin(), Tp.end() - 1);
    for (int i : rows)
        for (int j = Ap[i]; j < Ap[i + 1]; ++j) {
            const int k = cur[Aj[j]]++;
            Trow[k] = i;
            Tval[k] = Ax[j];
        }
    DBuf dTp, dTr, dTv, dx, dtemp, ddelta, dmask, drows, dw;
    CHK(put(dTp, Tp.data(), (long)Tp.size()));
    CHK(put(dTr, Trow.data(), (long)Trow.size()));
    CHK(put(dTv, Tval.data(), (long)Tval.size()));
    CHK(put(dx, x, x_size));
    CHK(put(dtemp, temp, temp_size));
    CHK(put(ddelta, Tx, Tx_size));
    CHK(put(dmask, in_range.data(), (long)in_range.size()));
    CHK(put(drows, rows.data(), (long)rows.size()));
    CHK(put(dw, omega, 1));
    hipLaunchKernelGGL(jacobi_ne_gather<T>, dim3(blocks_for(temp_size, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr,
                       dTp.i(), dTr.i(), tp<T>(dTv), tp<T>(ddelta), tp<T>(dw), tp<T>(dtemp),
                       (const unsigned char *)dmask.p, temp_size);
    CHK(launched("jacobi_ne gather"));
    const int cnt = (int)rows.size();
    hipLaunchKernelGGL(add_rows<T>, dim3(blocks_for(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, nullptr, tp<T>(dx),
                       tp<T>(dtemp), drows.i(), cnt);
    CHK(launched("jacobi_ne update"));
    AMG_HIP(hipDeviceSynchronize());
    CHK(get(dx, x, x_size));
    return get(dtemp, temp, temp_size);
}

template <class T>
int overlapping_schwarz_csr(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const T Ax[], int Ax_size,
                            T x[], int x_size, const T b[], int b_size, const T Tx[], int Tx_size, const int Tp[],
                            int Tp_size, const int Sj[], int Sj_size, const int Sp[], int Sp_size, int nsdomains,
                            int nrows, int row_start, int row_stop, int row_step)
{
    CHK(require_device());
    CHK(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (nrows != n || x_size < n || b_size < n) { set_error("vector / matrix sizes disagree"); return AMG_EINVAL; }
    if (nsdomains < 0 || Sp_size < nsdomains + 1 || Tp_size < nsdomains + 1) { set_error("bad subdomain pointers"); return AMG_EINVAL; }
    if (nsdomains && (Sp[nsdomains] > Sj_size || Tp[nsdomains] > Tx_size)) { set_error("bad subdomain arrays"); return AMG_EINVAL; }
    std::vector<int> tasks;
    CHK(sweep_rows(row_start, row_stop, row_step, nsdomains, tasks));
    if (tasks.empty()) return 0;
    for (int d = 0; d < nsdomains; ++d)
        if (Sp[d] < 0 || Sp[d + 1] < Sp[d] || Tp[d] < 0 || Tp[d + 1] < Tp[d]) { set_error("bad subdomain pointers"); return AMG_EINVAL; }
    for (int d : tasks)
        if ((long)(Sp[d + 1] - Sp[d]) * (Sp[d + 1] - Sp[d]) != (long)Tp[d + 1] - Tp[d]) { set_error("inverse block size does not match its subdomain"); return AMG_EINVAL; }
    CHK(check_pattern(Ap, n, Aj, n));
    std::vector<int> lp, order;
    CHK(schwarz_levels(n, Ap, Aj, Sj, Sp, tasks, lp, order));
    DevMat<T> A;
    DBuf dx, db, dT, dTp, dSj, dSp, dord, dscr;
    CHK(A.load(Ap, n, Aj, Ax, 1));
    CHK(put(dx, x, x_size));
    CHK(put(db, b, b_size));
    CHK(put(dT, Tx, Tp[nsdomains]));
    CHK(put(dTp, Tp, nsdomains + 1L));
    CHK(put(dSj, Sj, Sp[nsdomains]));
    CHK(put(dSp, Sp, nsdomains + 1L));
    CHK(put(dord, order.data(), (long)order.size()));
    CHK(dscr.alloc(sizeof(T) * (size_t)Sp[nsdomains]));
    CHK(run_levels(lp, [&](int off, int cnt) {
        hipLaunchKernelGGL(schwarz_level<T>, dim3(blocks_for(cnt, 64)), dim3(64), 0, nullptr, A.Ap.i(), A.Aj.i(),
                           tp<T>(A.Ax), tp<T>(dx), tp<T>(db), tp<T>(dT), dTp.i(), dSj.i(), dSp.i(), tp<T>(dscr),
                           dord.i() + off, cnt);
        return launched("schwarz level");
    }));
    AMG_HIP(hipDeviceSynchronize());
    return get(dx, x, x_size);
}

template <class T>
int csr_matvec(int n_row, int n_col, const int Ap[], const int Aj[], const T Ax[], const T x[], T y[])
{
    CHK(require_device());
    if (n_row < 0 || n_col < 0 || !Ap) { set_error("bad csr_matvec arguments"); return AMG_EINVAL; }
    if (n_row == 0) return 0;
    CHK(check_pattern(Ap, n_row, Aj, n_col));
    DevMat<T> A;
    DBuf dx, dy;
    CHK(A.load(Ap, n_row, Aj, Ax, 1));
    CHK(put(dx, x, n_col));
    CHK(put(dy, y, n_row));
    CHK((launch_rows<T, ROWS_MATVEC>(0, n_row, 0, 1, A, tp<T>(dx), (const T *)nullptr, (const T *)nullptr, tp<T>(dy))));
    AMG_HIP(hipDeviceSynchronize());
    return get(dy, y, n_row);
}

// scipy's bsr_matvec adds, for every point row, the blocks of its block row in stored order and each block's
// columns in order: the CSR matvec of the expanded matrix
template <class T>
int bsr_matvec(int n_brow, int n_bcol, int R, int C, const int Ap[], const int Aj[], const T Ax[], const T x[], T y[])
{
    CHK(require_device());
    if (n_brow < 0 || n_bcol < 0 || R < 1 || C < 1 || !Ap) { set_error("bad bsr_matvec arguments"); return AMG_EINVAL; }
    CHK(check_pattern(Ap, n_brow, Aj, n_bcol));
    std::vector<int> cp((size_t)n_brow * R + 1, 0), cj;
    std::vector<T> cx;
    const long nnz = (long)(Ap[n_brow] - Ap[0]) * R * C;
    cj.reserve((size_t)nnz);
    cx.reserve((size_t)nnz);
    for (int i = 0; i < n_brow; ++i)
        for (int r = 0; r < R; ++r) {
            for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj)
                for (int c = 0; c < C; ++c) {
                    cj.push_back(Aj[jj] * C + c);
                    cx.push_back(Ax[((long)jj * R + r) * C + c]);
                }
            cp[(size_t)i * R + r + 1] = (int)cj.size();
        }
    return csr_matvec<T>(n_brow * R, n_bcol * C, cp.data(), cj.data(), cx.data(), x, y);
}

}  // namespace typed
}  // namespace amg

// ----------------------------------------------------------------------------------------------- C ABI
#define AMG_TYPED_DEFINE(SUF, CT, T, F)                                                                          \
    int amgcore_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],      \
                                   int Ax_size, CT x[], int x_size, const CT b[], int b_size, int row_start,     \
                                   int row_stop, int row_step)                                                   \
    {                                                                                                            \
        return amg::typed::gauss_seidel<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size,     \
                                           (const T *)b, b_size, row_start, row_stop, row_step);                 \
    }                                                                                                            \
    int amgcore_bsr_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],  \
                                       int Ax_size, CT x[], int x_size, const CT b[], int b_size, int row_start, \
                                       int row_stop, int row_step, int blocksize)                                \
    {                                                                                                            \
        return amg::typed::bsr_gauss_seidel<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size, \
                                               (const T *)b, b_size, row_start, row_stop, row_step, blocksize);  \
    }                                                                                                            \
    int amgcore_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],            \
                             int Ax_size, CT x[], int x_size, const CT b[], int b_size, CT temp[],               \
                             int temp_size, int row_start, int row_stop, int row_step, const CT omega[],         \
                             int omega_size)                                                                     \
    {                                                                                                            \
        return amg::typed::jacobi<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size,           \
                                     (const T *)b, b_size, (T *)temp, temp_size, row_start, row_stop, row_step,  \
                                     (const T *)omega, omega_size);                                              \
    }                                                                                                            \
    int amgcore_bsr_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],        \
                                 int Ax_size, CT x[], int x_size, const CT b[], int b_size, CT temp[],           \
                                 int temp_size, int row_start, int row_stop, int row_step, int blocksize,        \
                                 const CT omega[], int omega_size)                                               \
    {                                                                                                            \
        return amg::typed::bsr_jacobi<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size,       \
                                         (const T *)b, b_size, (T *)temp, temp_size, row_start, row_stop,        \
                                         row_step, blocksize, (const T *)omega, omega_size);                     \
    }                                                                                                            \
    int amgcore_gauss_seidel_indexed_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size,             \
                                           const CT Ax[], int Ax_size, CT x[], int x_size, const CT b[],         \
                                           int b_size, const int Id[], int Id_size, int row_start,               \
                                           int row_stop, int row_step)                                           \
    {                                                                                                            \
        return amg::typed::gauss_seidel_indexed<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x,     \
                                                   x_size, (const T *)b, b_size, Id, Id_size, row_start,         \
                                                   row_stop, row_step);                                          \
    }                                                                                                            \
    int amgcore_jacobi_ne_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],         \
                                int Ax_size, CT x[], int x_size, const CT b[], int b_size, const CT Tx[],        \
                                int Tx_size, CT temp[], int temp_size, int row_start, int row_stop,              \
                                int row_step, const CT omega[], int omega_size)                                  \
    {                                                                                                            \
        return amg::typed::jacobi_ne<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size,        \
                                        (const T *)b, b_size, (const T *)Tx, Tx_size, (T *)temp, temp_size,      \
                                        row_start, row_stop, row_step, (const T *)omega, omega_size);            \
    }                                                                                                            \
    int amgcore_overlapping_schwarz_csr_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size,          \
                                              const CT Ax[], int Ax_size, CT x[], int x_size, const CT b[],      \
                                              int b_size, const CT Tx[], int Tx_size, const int Tp[],            \
                                              int Tp_size, const int Sj[], int Sj_size, const int Sp[],          \
                                              int Sp_size, int nsdomains, int nrows, int row_start,              \
                                              int row_stop, int row_step)                                        \
    {                                                                                                            \
        return amg::typed::overlapping_schwarz_csr<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x,  \
                                                      x_size, (const T *)b, b_size, (const T *)Tx, Tx_size, Tp,  \
                                                      Tp_size, Sj, Sj_size, Sp, Sp_size, nsdomains, nrows,       \
                                                      row_start, row_stop, row_step);                            \
    }                                                                                                            \
    int amgcore_gauss_seidel_ne_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],   \
                                      int Ax_size, CT x[], int x_size, const CT b[], int b_size, int row_start,  \
                                      int row_stop, int row_step, const CT Tx[], int Tx_size, F omega)           \
    {                                                                                                            \
        return amg::typed::gauss_seidel_ne<T, F>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x,       \
                                                 x_size, (const T *)b, b_size, row_start, row_stop, row_step,    \
                                                 (const T *)Tx, Tx_size, omega);                                 \
    }                                                                                                            \
    int amgcore_gauss_seidel_nr_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],   \
                                      int Ax_size, CT x[], int x_size, CT z[], int z_size, int col_start,        \
                                      int col_stop, int col_step, const CT Tx[], int Tx_size, F omega)           \
    {                                                                                                            \
        return amg::typed::gauss_seidel_nr<T, F>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x,       \
                                                 x_size, (T *)z, z_size, col_start, col_stop, col_step,          \
                                                 (const T *)Tx, Tx_size, omega);                                 \
    }                                                                                                            \
    int amgcore_block_jacobi_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size, const CT Ax[],      \
                                   int Ax_size, CT x[], int x_size, const CT b[], int b_size, const CT Tx[],     \
                                   int Tx_size, CT temp[], int temp_size, int row_start, int row_stop,           \
                                   int row_step, const CT omega[], int omega_size, int blocksize)                \
    {                                                                                                            \
        return amg::typed::block_jacobi<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x, x_size,     \
                                           (const T *)b, b_size, (const T *)Tx, Tx_size, (T *)temp, temp_size,   \
                                           row_start, row_stop, row_step, (const T *)omega, omega_size,          \
                                           blocksize);                                                           \
    }                                                                                                            \
    int amgcore_block_gauss_seidel_##SUF(const int Ap[], int Ap_size, const int Aj[], int Aj_size,               \
                                         const CT Ax[], int Ax_size, CT x[], int x_size, const CT b[],           \
                                         int b_size, const CT Tx[], int Tx_size, int row_start, int row_stop,    \
                                         int row_step, int blocksize)                                            \
    {                                                                                                            \
        return amg::typed::block_gauss_seidel<T>(Ap, Ap_size, Aj, Aj_size, (const T *)Ax, Ax_size, (T *)x,       \
                                                 x_size, (const T *)b, b_size, (const T *)Tx, Tx_size,           \
                                                 row_start, row_stop, row_step, blocksize);                      \
    }                                                                                                            \
    int amgcore_csr_matvec_##SUF(int n_row, int n_col, const int Ap[], const int Aj[], const CT Ax[],            \
                                 const CT x[], CT y[])                                                           \
    {                                                                                                            \
        return amg::typed::csr_matvec<T>(n_row, n_col, Ap, Aj, (const T *)Ax, (const T *)x, (T *)y);            \
    }                                                                                                            \
    int amgcore_bsr_matvec_##SUF(int n_brow, int n_bcol, int R, int C, const int Ap[], const int Aj[],           \
                                 const CT Ax[], const CT x[], CT y[])                                            \
    {                                                                                                            \
        return amg::typed::bsr_matvec<T>(n_brow, n_bcol, R, C, Ap, Aj, (const T *)Ax, (const T *)x, (T *)y);     \
    }

static_assert(sizeof(amg_c64) == sizeof(c64) && sizeof(amg_c128) == sizeof(c128), "complex layout");

extern "C" {
AMG_TYPED_DEFINE(f32, float, float, float)
AMG_TYPED_DEFINE(c64, amg_c64, c64, float)
AMG_TYPED_DEFINE(c128, amg_c128, c128, double)
}  // extern "C"
