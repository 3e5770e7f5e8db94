// Resident hierarchies of other value types (include/amgcore_hip.h, section 5): multilevel_solver.solve() and
// __solve() (multilevel.py:316-556) for a hierarchy whose operators hold complex128 values.  The engine is a
// template on the value type T; only complex128 is instantiated.
//
// Arithmetic: every step but the residual norm gives the reference's bits.
//   A x, R r, P e      scipy's csr_matvec / bsr_matvec: each row summed from zero in stored order, products
//                      through scalar.hpp (no contraction: the library builds with -ffp-contract=off)
//   r = b - (A x)      the product formed from zero, then subtracted; coarse_b = R r; x += (P e)
//   smoothers          the amg_core kernels of typed_kernels.hpp (one launch per dependency level for the
//                      Gauss-Seidel family, levels from build_levels)
//   numpy steps        polynomial (relaxation.py:653-668) and sor (relaxation.py:158-170) scale by a real
//                      scalar the way numpy does: promoted to c + 0i, full complex product (npmul below)
//   residual norm      sqrt(sum(re^2 + im^2)) by a two-stage reduction in double (the reference's is BLAS)
//   dense coarse solve sequential row sums, left to right from zero
//
// Shapes: CSR rows run in 256-row workgroups that stage their entries' products in LDS (coalesced 16-byte loads)
// and sum each row in stored order; BSR rows run one thread per point row.  Launches are eager on one stream.
#include "hier.hpp"
#include "flat.hpp"
#include "scalar.hpp"
#include "typed_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace amg;
using namespace amg::sc;
using namespace amg::tk;

namespace {

constexpr int NORM_BLOCKS = 512;    // partial sums of the residual norm
constexpr int NORM_WG = 256;
constexpr int VEC_WG = 256;

enum { SM_NONE = 0, SM_JACOBI = 1, SM_GS = 2, SM_SOR = 3, SM_POLY = 4, SM_BJACOBI = 5, SM_BGS = 6 };
enum { COARSE_NONE = 0, COARSE_DENSE = 1, COARSE_SMOOTHER = 2, COARSE_CALLBACK = 3 };

// numpy's product of a complex array with a real scalar c: c is promoted to c + 0i and the full complex product
// formed, (a.re c - a.im 0, a.re 0 + a.im c); it differs from component-wise scaling in the sign of zeros
AMG_HD c128 npmul(c128 a, double c) { return c128{a.re * c - a.im * 0.0, a.re * 0.0 + a.im * c}; }

// ----------------------------------------------------------------------------------------------- row epilogues
template <class T> struct EpiStore {           // y = A v (from zero)
    T *y;
    __device__ void operator()(int i, T acc) const { y[i] = acc; }
};
template <class T> struct EpiResid {           // r = b - (A v)
    const T *b;
    T *r;
    __device__ void operator()(int i, T acc) const { r[i] = sub(b[i], acc); }
};
template <class T> struct EpiAdd {             // x += (A v)
    T *x;
    __device__ void operator()(int i, T acc) const { x[i] = add(x[i], acc); }
};
// polynomial smoother, first step: residual = b - A x; h = c0 * residual.  (x is this kernel's operand: with one
// coefficient x += h runs as a kernel of its own, add_to)
template <class T> struct EpiPoly0 {
    const T *b;
    T *r, *h;
    double c;
    __device__ void operator()(int i, T acc) const
    {
        const T ri = sub(b[i], acc);
        r[i] = ri;
        h[i] = npmul(ri, c);
    }
};
// later steps: h = c * residual + A h (acc = A h); the last one adds h to x instead of storing it
template <class T> struct EpiPolyStep {
    const T *r;
    T *hout, *x;
    double c;
    int last;
    __device__ void operator()(int i, T acc) const
    {
        const T hi = add(npmul(r[i], c), acc);
        if (last) x[i] = add(x[i], hi);
        else hout[i] = hi;
    }
};

// ----------------------------------------------------------------------------------------------- kernels
// CSR rows: products staged in LDS a chunk of the workgroup's entries at a time, each row summed from zero in
// stored order by its own thread (the order of scipy's csr_matvec)
template <class T, class Epi>
__global__ void __launch_bounds__(ROWS_PER_WG)
csr_rows(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
         const T *__restrict__ v, Epi epi)
{
    __shared__ T prod[CHUNK];
    const int r0 = blockIdx.x * ROWS_PER_WG;
    const int r1 = min(n, r0 + ROWS_PER_WG);
    const int i = r0 + (int)threadIdx.x;
    const bool mine = i < r1;
    const int e0 = Ap[r0], e1 = Ap[r1];
    const int rs = mine ? Ap[i] : 0, re = mine ? Ap[i + 1] : 0;
    T acc = from_real<T>(0.0);
    for (int c0 = e0; c0 < e1; c0 += CHUNK) {
        const int cn = min(CHUNK, e1 - c0);
        for (int k = threadIdx.x; k < cn; k += ROWS_PER_WG) prod[k] = mul(Ax[c0 + k], v[Aj[c0 + k]]);
        __syncthreads();
        const int a = max(rs, c0), z = min(re, c0 + cn);
        for (int k = a; k < z; ++k) acc = add(acc, prod[k - c0]);
        __syncthreads();
    }
    if (mine) epi(i, acc);
}

// BSR rows (R x C blocks): point row p = i R + r summed over its blocks in stored order, columns within a
// block left to right, from zero (scipy's bsr_matvec: gemv accumulating into a zeroed y)
template <class T, class Epi>
__global__ void bsr_rows(int npoint, int R, int C, const int *__restrict__ Ap, const int *__restrict__ Aj,
                         const T *__restrict__ Ax, const T *__restrict__ v, Epi epi)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npoint) return;
    const int i = p / R, r = p - i * R;
    const long RC = (long)R * C;
    T acc = from_real<T>(0.0);
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
        const T *A = Ax + jj * RC + (long)r * C;
        const T *xv = v + (long)Aj[jj] * C;
        for (int c = 0; c < C; ++c) acc = add(acc, mul(A[c], xv[c]));
    }
    epi(p, acc);
}

// x += h
template <class T>
__global__ void add_to(int n, T *__restrict__ x, const T *__restrict__ h)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = add(x[i], h[i]);
}

// sor (relaxation.py:166-168): x *= omega; x_old *= (1 - omega); x += x_old, with numpy's products
template <class T>
__global__ void sor_blend(int n, T *__restrict__ x, const T *__restrict__ xold, double w, double w1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = add(npmul(x[i], w), npmul(xold[i], w1));
}

// dense coarse operator (row-major): x_i = sum_j M_ij b_j from zero, left to right.  One workgroup per row: its
// threads form the row's products a chunk at a time (coalesced loads of M) into LDS, one thread adds them in order.
constexpr int DENSE_WG = 256;
template <class T>
__global__ void __launch_bounds__(DENSE_WG)
dense_apply(int n, const T *__restrict__ M, const T *__restrict__ b, T *__restrict__ x)
{
    __shared__ T prod[CHUNK];
    const int i = blockIdx.x;
    const T *row = M + (long)i * n;
    T acc = from_real<T>(0.0);
    for (int c0 = 0; c0 < n; c0 += CHUNK) {
        const int cn = min(CHUNK, n - c0);
        for (int k = threadIdx.x; k < cn; k += DENSE_WG) prod[k] = mul(row[c0 + k], b[c0 + k]);
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < cn; ++k) acc = add(acc, prod[k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) x[i] = acc;
}

AMG_HD double sq(c128 v) { return v.re * v.re + v.im * v.im; }

// ||v||^2 in two stages: fixed partial sums per workgroup, then one workgroup adds them and takes the root
template <class T>
__global__ void __launch_bounds__(NORM_WG) norm_partial(const T *__restrict__ v, long n, double *__restrict__ part)
{
    __shared__ double s[NORM_WG];
    double acc = 0.0;
    for (long k = (long)blockIdx.x * NORM_WG + threadIdx.x; k < n; k += (long)gridDim.x * NORM_WG) acc += sq(v[k]);
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NORM_WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(NORM_WG) norm_final(const double *__restrict__ part, int np, double *__restrict__ out)
{
    __shared__ double s[NORM_WG];
    double acc = 0.0;
    for (int k = threadIdx.x; k < np; k += NORM_WG) acc += part[k];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NORM_WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sqrt(s[0]);
}

// ----------------------------------------------------------------------------------------------- host side
int blocks_of(long n, int per) { return (int)((n + per - 1) / per); }

int launched(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
    return 0;
}

// Ap nondecreasing from 0, every column index in [0, ncols): no kernel can read outside its arrays
int check_pattern(const int *Ap, int nrows, const int *Aj, int ncols)
{
    if (!Ap || Ap[0] != 0) { set_error("bad Ap"); return AMG_EINVAL; }
    for (int i = 0; i < nrows; ++i)
        if (Ap[i + 1] < Ap[i]) { set_error("Ap is not nondecreasing"); return AMG_EINVAL; }
    for (long k = 0; k < Ap[nrows]; ++k)
        if (Aj[k] < 0 || Aj[k] >= ncols) { set_error("column index out of range"); return AMG_EINVAL; }
    return 0;
}

struct Pool {            // device buffers of one hierarchy, counted for device_bytes
    long bytes = 0;
    int alloc(DBuf &d, size_t n)
    {
        CHK(d.alloc(n));
        bytes += (long)n;
        return 0;
    }
    int upload(DBuf &d, const void *src, size_t n)
    {
        CHK(alloc(d, n));
        if (n) AMG_HIP(hipMemcpy(d.p, src, n, hipMemcpyHostToDevice));
        return 0;
    }
};

// one operator: CSR (R = C = 1) or BSR with R x C blocks; nb block rows, nrows = nb R point rows
template <class T>
struct XMat {
    bool set = false;
    int bsr = 0, nrows = 0, ncols = 0, R = 1, C = 1, nb = 0;
    long nnzb = 0;
    DBuf Ap, Aj, Ax;
    std::vector<int> hAp, hAj;      // the pattern on the host until the schedules are built
    int load(Pool &pool, int fmt, int nr, int nc, int r, int c, const int *ap, const int *aj, const void *ax)
    {
        if (fmt != 0 && fmt != 1) { set_error("fmt must be 0 (CSR) or 1 (BSR)"); return AMG_EINVAL; }
        if (nr < 0 || nc < 0 || r < 1 || c < 1 || nr % r || nc % c) { set_error("bad shape / blocksize"); return AMG_EINVAL; }
        if (!ap || (!aj && ap[0] != ap[nr / r]) || (!ax && ap[0] != ap[nr / r])) { set_error("null array"); return AMG_EINVAL; }
        bsr = fmt;
        nrows = nr, ncols = nc, R = r, C = c, nb = nr / r;
        CHK(check_pattern(ap, nb, aj, nc / c));
        nnzb = ap[nb];
        CHK(pool.upload(Ap, ap, sizeof(int) * (size_t)(nb + 1)));
        CHK(pool.upload(Aj, aj, sizeof(int) * (size_t)nnzb));
        CHK(pool.upload(Ax, ax, sizeof(T) * (size_t)(nnzb * R * C)));
        hAp.assign(ap, ap + nb + 1);
        hAj.assign(aj, aj + nnzb);
        set = true;
        return 0;
    }
    const int *ap() const { return Ap.i(); }
    const int *aj() const { return Aj.i(); }
    const T *ax() const { return (const T *)Ax.p; }
};

// rows of v through A, each row's sum handed to epi (CSR: LDS-staged workgroups; BSR: a thread per point row)
template <class T, class Epi>
int apply_rows(const XMat<T> &A, const T *v, Epi epi, hipStream_t st)
{
    if (A.nrows == 0) return 0;
    if (!A.bsr || (A.R == 1 && A.C == 1)) {
        hipLaunchKernelGGL((csr_rows<T, Epi>), dim3(blocks_of(A.nrows, ROWS_PER_WG)), dim3(ROWS_PER_WG), 0, st,
                           A.nrows, A.ap(), A.aj(), A.ax(), v, epi);
    } else {
        hipLaunchKernelGGL((bsr_rows<T, Epi>), dim3(blocks_of(A.nrows, VEC_WG)), dim3(VEC_WG), 0, st, A.nrows, A.R,
                           A.C, A.ap(), A.aj(), A.ax(), v, epi);
    }
    return launched("row kernel");
}

// dependency levels of a sweep over the block rows of a pattern (rows in level order on the device)
struct Sweep {
    std::vector<int> lp;
    DBuf rows;
    int build(Pool &pool, int nb, const std::vector<int> &Ap, const std::vector<int> &Aj, bool backward)
    {
        std::vector<int> tasks(nb), order, rws(nb);
        for (int t = 0; t < nb; ++t) tasks[t] = backward ? nb - 1 - t : t;
        CHK(build_levels(nb, Ap.data(), Aj.data(), tasks.data(), nb, lp, order));
        for (int k = 0; k < nb; ++k) rws[k] = tasks[order[k]];
        return pool.upload(rows, rws.data(), sizeof(int) * (size_t)nb);
    }
};

template <class T>
struct XSmoother {
    bool set = false;
    int kind = SM_NONE, iterations = 1, sweep = 0, bs = 1;
    T omega = from_real<T>(1.0);
    std::vector<double> coef;
    DBuf Dinv, omega_dev, iota;
    XMat<T> Ab;                 // A re-blocked to bs x bs (block smoothers), when the level's A is not already
    Sweep fwd, bwd;
};

template <class T>
struct XLevel {
    XMat<T> A, P, R;
    XSmoother<T> sm[2];
    DBuf x, b, r, h1, h2, t;     // iterate, right-hand side, residual, polynomial ping-pong, jacobi/sor copy
};

template <class T>
struct Engine {
    int device = 0, nlev = 0;
    bool finalized = false;
    bool sealed = false;                  // finalize has run: the operators, smoothers and coarse solver are fixed
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<XLevel<T>> lv;
    int coarse = COARSE_NONE;
    XSmoother<T> csm;                     // relaxation-named coarse solver
    DBuf M;
    int nM = 0;
    amg_coarse_callback_x cb = nullptr;
    void *cb_user = nullptr;
    std::vector<T> hb, hx;
    DBuf part, res;
    int nres_cap = 0;
    double last_ms = 0.0;
    Pool pool;
    ~Engine()
    {
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (st) hipStreamDestroy(st);
    }
};

// ----------------------------------------------------------------------------------------------- smoothers
template <class T>
const XMat<T> &block_op(const XLevel<T> &L, const XSmoother<T> &s) { return s.Ab.set ? s.Ab : L.A; }

template <class T>
int gs_sweep(const XMat<T> &A, T *x, const T *b, const Sweep &S, bool reverse, hipStream_t st)
{
    for (size_t l = 0; l + 1 < S.lp.size(); ++l) {
        const int off = S.lp[l], cnt = S.lp[l + 1] - S.lp[l];
        if (cnt <= 0) continue;
        if (!A.bsr) {       // a BSR operator, 1 x 1 blocks included, relaxes through bsr_gauss_seidel
            hipLaunchKernelGGL(gs_level<T>, dim3(blocks_of(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, st, A.ap(), A.aj(),
                               A.ax(), x, b, S.rows.i() + off, cnt);
        } else {
            hipLaunchKernelGGL((bsr_point_level<T, false>), dim3(blocks_of(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, st,
                               A.ap(), A.aj(), A.ax(), (const T *)x, x, b, (const T *)nullptr, S.rows.i() + off, cnt,
                               A.R, reverse ? 1 : 0);
        }
        CHK(launched("gauss_seidel level"));
    }
    return 0;
}

template <class T>
int bgs_sweep(const XMat<T> &A, const XSmoother<T> &s, T *x, const T *b, T *scratch, const Sweep &S, hipStream_t st)
{
    for (size_t l = 0; l + 1 < S.lp.size(); ++l) {
        const int off = S.lp[l], cnt = S.lp[l + 1] - S.lp[l];
        if (cnt <= 0) continue;
        hipLaunchKernelGGL((block_level<T, false>), dim3(blocks_of(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, st, A.ap(),
                           A.aj(), A.ax(), (const T *)s.Dinv.p, (const T *)x, x, b, (const T *)nullptr, scratch,
                           S.rows.i() + off, cnt, s.bs);
        CHK(launched("block_gauss_seidel level"));
    }
    return 0;
}

// one application of smoother s on level L: x relaxed in place for right-hand side b
template <class T>
int relax(Engine<T> &E, XLevel<T> &L, const XSmoother<T> &s, T *x, const T *b)
{
    hipStream_t st = E.st;
    const XMat<T> &A = L.A;
    const int n = A.nrows;
    T *t = (T *)L.t.p;
    const size_t vbytes = sizeof(T) * (size_t)n;
    auto sweeps = [&](int sweep) -> int {          // one gauss_seidel(iterations=1, sweep) call
        if (sweep != 1) CHK(gs_sweep(A, x, b, s.fwd, false, st));
        if (sweep != 0) CHK(gs_sweep(A, x, b, s.bwd, true, st));
        return 0;
    };
    switch (s.kind) {
    case SM_NONE:
        return 0;
    case SM_GS:
        for (int it = 0; it < s.iterations; ++it) CHK(sweeps(s.sweep));
        return 0;
    case SM_SOR: {
        const double w = s.omega.re, w1 = 1.0 - w;
        for (int it = 0; it < s.iterations; ++it) {
            AMG_HIP(hipMemcpyAsync(t, x, vbytes, hipMemcpyDeviceToDevice, st));
            CHK(sweeps(s.sweep));
            hipLaunchKernelGGL(sor_blend<T>, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, st, n, x, (const T *)t, w, w1);
            CHK(launched("sor blend"));
        }
        return 0;
    }
    case SM_JACOBI:
        for (int it = 0; it < s.iterations; ++it) {
            AMG_HIP(hipMemcpyAsync(t, x, vbytes, hipMemcpyDeviceToDevice, st));     // relaxation.h:216-218
            if (!A.bsr) {   // BSR, 1 x 1 blocks included: bsr_jacobi
                if (n > 0)
                    hipLaunchKernelGGL((rows_stream<T, ROWS_JACOBI>), dim3(blocks_of(n, ROWS_PER_WG)), dim3(ROWS_PER_WG),
                                       0, st, 0, n, 0, 1, A.ap(), A.aj(), A.ax(), (const T *)t, b,
                                       (const T *)s.omega_dev.p, x);
            } else if (A.nb > 0) {
                hipLaunchKernelGGL((bsr_point_level<T, true>), dim3(blocks_of(A.nb, LEVEL_WG)), dim3(LEVEL_WG), 0, st,
                                   A.ap(), A.aj(), A.ax(), (const T *)t, x, b, (const T *)s.omega_dev.p, s.iota.i(),
                                   A.nb, A.R, 0);
            }
            CHK(launched("jacobi"));
        }
        return 0;
    case SM_BJACOBI: {
        const XMat<T> &B = block_op(L, s);
        for (int it = 0; it < s.iterations; ++it) {
            AMG_HIP(hipMemcpyAsync(t, x, vbytes, hipMemcpyDeviceToDevice, st));     // relaxation.h:686-688
            if (B.nb > 0)
                hipLaunchKernelGGL((block_level<T, true>), dim3(blocks_of(B.nb, LEVEL_WG)), dim3(LEVEL_WG), 0, st,
                                   B.ap(), B.aj(), B.ax(), (const T *)s.Dinv.p, (const T *)t, x, b,
                                   (const T *)s.omega_dev.p, (T *)L.h2.p, s.iota.i(), B.nb, s.bs);
            CHK(launched("block_jacobi"));
        }
        return 0;
    }
    case SM_BGS: {
        const XMat<T> &B = block_op(L, s);
        for (int it = 0; it < s.iterations; ++it) {
            if (s.sweep != 1) CHK(bgs_sweep(B, s, x, b, (T *)L.h2.p, s.fwd, st));
            if (s.sweep != 0) CHK(bgs_sweep(B, s, x, b, (T *)L.h2.p, s.bwd, st));
        }
        return 0;
    }
    case SM_POLY: {
        // relaxation.py:655-668.  norm(x) == 0 selects residual = b; for finite A, b - A 0 is b bit for bit (every
        // product is a zero and a sum from +0 of zeros is +0), so the residual is always formed as b - A x.
        const int nc = (int)s.coef.size();
        T *r = (T *)L.r.p, *h = (T *)L.h1.p, *h2 = (T *)L.h2.p;
        for (int it = 0; it < s.iterations; ++it) {
            CHK(apply_rows(A, (const T *)x, EpiPoly0<T>{b, r, h, s.coef[0]}, st));
            if (nc == 1 && n > 0) {
                hipLaunchKernelGGL(add_to<T>, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, st, n, x, (const T *)h);
                CHK(launched("polynomial update"));
            }
            for (int k = 1; k < nc; ++k) {
                const bool last = k == nc - 1;
                CHK(apply_rows(A, (const T *)h, EpiPolyStep<T>{r, h2, x, s.coef[k], last ? 1 : 0}, st));
                std::swap(h, h2);
            }
        }
        return 0;
    }
    }
    set_error("unknown smoother kind");
    return AMG_EINVAL;
}

// coarse solve of the last level: x = coarse_solver(A, b) (x zeroed first)
template <class T>
int coarse_solve(Engine<T> &E, T *x, const T *b)
{
    XLevel<T> &L = E.lv[E.nlev - 1];
    const int n = L.A.nrows;
    const size_t vbytes = sizeof(T) * (size_t)n;
    switch (E.coarse) {
    case COARSE_NONE:
        if (n) AMG_HIP(hipMemsetAsync(x, 0, vbytes, E.st));
        return 0;
    case COARSE_DENSE:
        if (n) {
            hipLaunchKernelGGL(dense_apply<T>, dim3(n), dim3(DENSE_WG), 0, E.st, n, (const T *)E.M.p, b, x);
            CHK(launched("dense coarse apply"));
        }
        return 0;
    case COARSE_SMOOTHER:
        if (n) AMG_HIP(hipMemsetAsync(x, 0, vbytes, E.st));
        return relax(E, L, E.csm, x, b);
    case COARSE_CALLBACK: {
        E.hb.resize(n);
        E.hx.assign(n, from_real<T>(0.0));
        if (n) AMG_HIP(hipMemcpyAsync(E.hb.data(), b, vbytes, hipMemcpyDeviceToHost, E.st));
        AMG_HIP(hipStreamSynchronize(E.st));
        if (E.cb(E.cb_user, n, E.hb.data(), E.hx.data()) != 0) { set_error("coarse solver callback failed"); return AMG_EINVAL; }
        if (n) AMG_HIP(hipMemcpyAsync(x, E.hx.data(), vbytes, hipMemcpyHostToDevice, E.st));
        AMG_HIP(hipStreamSynchronize(E.st));
        return 0;
    }
    }
    set_error("no coarse solver");
    return AMG_ESTATE;
}

// multilevel.py:473-548 on level l (V, W, F); x_l and b_l live in the level's vectors
template <class T>
int cycle_level(Engine<T> &E, int l, int cyc)
{
    XLevel<T> &L = E.lv[l], &Lc = E.lv[l + 1];
    T *x = (T *)L.x.p, *b = (T *)L.b.p, *r = (T *)L.r.p;
    T *xc = (T *)Lc.x.p, *bc = (T *)Lc.b.p;
    CHK(relax(E, L, L.sm[0], x, b));
    CHK(apply_rows(L.A, (const T *)x, EpiResid<T>{b, r}, E.st));                       // residual = b - A x
    CHK(apply_rows(L.R, (const T *)r, EpiStore<T>{bc}, E.st));                         // coarse_b = R residual
    if (Lc.A.nrows) AMG_HIP(hipMemsetAsync(xc, 0, sizeof(T) * (size_t)Lc.A.nrows, E.st));
    if (l == E.nlev - 2) {
        CHK(coarse_solve(E, xc, bc));
    } else if (cyc == 0) {
        CHK(cycle_level(E, l + 1, 0));
    } else if (cyc == 1) {
        CHK(cycle_level(E, l + 1, 1));
        CHK(cycle_level(E, l + 1, 1));
    } else {
        CHK(cycle_level(E, l + 1, 2));
        CHK(cycle_level(E, l + 1, 0));
    }
    CHK(apply_rows(L.P, (const T *)xc, EpiAdd<T>{x}, E.st));                           // x += P coarse_x
    return relax(E, L, L.sm[1], x, b);
}

template <class T>
int one_cycle(Engine<T> &E, int cyc)
{
    if (E.nlev == 1) {                      // multilevel.py:456-458: x = coarse_solver(A, b)
        XLevel<T> &L = E.lv[0];
        return coarse_solve(E, (T *)L.x.p, (const T *)L.b.p);
    }
    return cycle_level(E, 0, cyc);
}

template <class T>
int device_norm(Engine<T> &E, const T *v, long n, double *out)
{
    hipLaunchKernelGGL(norm_partial<T>, dim3(NORM_BLOCKS), dim3(NORM_WG), 0, E.st, v, n, E.part.d());
    CHK(launched("norm partial"));
    hipLaunchKernelGGL(norm_final, dim3(1), dim3(NORM_WG), 0, E.st, (const double *)E.part.d(), NORM_BLOCKS, out);
    return launched("norm final");
}

// res_slot = ||b - A x|| on level 0
template <class T>
int residual_norm(Engine<T> &E, double *slot)
{
    XLevel<T> &L = E.lv[0];
    CHK(apply_rows(L.A, (const T *)L.x.p, EpiResid<T>{(const T *)L.b.p, (T *)L.r.p}, E.st));
    return device_norm(E, (const T *)L.r.p, L.A.nrows, slot);
}

template <class T>
int load_vectors(Engine<T> &E, const void *b, const void *x, int flags)
{
    XLevel<T> &L = E.lv[0];
    const size_t vbytes = sizeof(T) * (size_t)L.A.nrows;
    if (!vbytes) return 0;
    AMG_HIP(hipMemcpyAsync(L.b.p, b, vbytes, hipMemcpyHostToDevice, E.st));
    if (flags & AMG_SOLVE_X0_ZERO) AMG_HIP(hipMemsetAsync(L.x.p, 0, vbytes, E.st));
    else AMG_HIP(hipMemcpyAsync(L.x.p, x, vbytes, hipMemcpyHostToDevice, E.st));
    return 0;
}

template <class T>
int store_x(Engine<T> &E, void *x)
{
    XLevel<T> &L = E.lv[0];
    const size_t vbytes = sizeof(T) * (size_t)L.A.nrows;
    if (vbytes) AMG_HIP(hipMemcpyAsync(x, L.x.p, vbytes, hipMemcpyDeviceToHost, E.st));
    AMG_HIP(hipStreamSynchronize(E.st));
    return 0;
}

// ----------------------------------------------------------------------------------------------- setup
template <class T>
int build_smoother(Engine<T> &E, XLevel<T> &L, XSmoother<T> &s)
{
    if (s.kind == SM_NONE) return 0;
    const XMat<T> &A = L.A;
    if ((s.kind == SM_BJACOBI || s.kind == SM_BGS) && !s.Ab.set) {
        if (!(A.bsr && A.R == s.bs && A.C == s.bs) && !(s.bs == 1 && (!A.bsr || A.R == 1))) {
            set_error("block smoother: pass A re-blocked to its blocksize (amg_hierx_set_block_matrix)");
            return AMG_ESTATE;
        }
    }
    const XMat<T> &B = (s.kind == SM_BJACOBI || s.kind == SM_BGS) ? block_op(L, s) : A;
    if ((s.kind == SM_BJACOBI || s.kind == SM_BGS) && (long)B.nb * s.bs != A.nrows) {
        set_error("block matrix does not match the level's operator");
        return AMG_EINVAL;
    }
    if (s.kind == SM_GS || s.kind == SM_SOR || s.kind == SM_BGS) {
        if (s.sweep != 1) CHK(s.fwd.build(E.pool, B.nb, B.hAp, B.hAj, false));
        if (s.sweep != 0) CHK(s.bwd.build(E.pool, B.nb, B.hAp, B.hAj, true));
    }
    if (s.kind == SM_JACOBI || s.kind == SM_BJACOBI) {
        std::vector<int> iota(B.nb);
        for (int k = 0; k < B.nb; ++k) iota[k] = k;
        CHK(E.pool.upload(s.iota, iota.data(), sizeof(int) * iota.size()));
        CHK(E.pool.upload(s.omega_dev, &s.omega, sizeof(T)));
    }
    return 0;
}

template <class T>
int set_smoother(Engine<T> &E, int lvl, int which, const amg_smoother_desc_x *d)
{
    if (lvl < 0 || lvl >= E.nlev || which < 0 || which > 2 || !d) { set_error("bad smoother slot"); return AMG_EINVAL; }
    if (which == 2 && lvl != E.nlev - 1) { set_error("the coarse smoother belongs to the last level"); return AMG_EINVAL; }
    if (which < 2 && lvl == E.nlev - 1) { set_error("the last level has no pre/post smoother"); return AMG_EINVAL; }
    if (d->kind < SM_NONE || d->kind > SM_BGS) {
        set_error("smoother kind " + std::to_string(d->kind) + " has no implementation for this value type");
        return AMG_ENOTIMPL;
    }
    XSmoother<T> &s = which == 2 ? E.csm : E.lv[lvl].sm[which];
    if (s.set) { set_error("smoother already set"); return AMG_ESTATE; }
    if (which == 2 && E.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    s.set = true;
    s.kind = d->kind;
    if (s.kind == SM_NONE) return 0;
    if (d->iterations < 0 || d->sweep < 0 || d->sweep > 2) { set_error("bad iterations / sweep"); return AMG_EINVAL; }
    s.iterations = d->iterations;
    s.sweep = d->sweep;
    if (s.kind == SM_JACOBI || s.kind == SM_SOR || s.kind == SM_BJACOBI) {
        if (!d->omega) { set_error("omega missing"); return AMG_EINVAL; }
        std::memcpy(&s.omega, d->omega, sizeof(T));
        if (s.kind == SM_SOR && s.omega.im != 0.0) { set_error("sor: omega must be real"); return AMG_ENOTIMPL; }
    }
    if (s.kind == SM_POLY) {
        if (d->ncoef < 1 || !d->coef) { set_error("polynomial: no coefficients"); return AMG_EINVAL; }
        s.coef.assign(d->coef, d->coef + d->ncoef);
    }
    if (s.kind == SM_BJACOBI || s.kind == SM_BGS) {
        const XMat<T> &A = E.lv[lvl].A;
        if (!A.set) { set_error("set the level's A before its smoothers"); return AMG_ESTATE; }
        if (d->blocksize < 1 || A.nrows % d->blocksize || !d->Dinv) { set_error("bad blocksize / Dinv"); return AMG_EINVAL; }
        s.bs = d->blocksize;
        CHK(E.pool.upload(s.Dinv, d->Dinv, sizeof(T) * (size_t)A.nrows * s.bs));
    }
    return 0;
}

template <class T>
int finalize(Engine<T> &E)
{
    if (E.sealed) {
        if (E.finalized) return 0;
        set_error("an earlier amg_hierx_finalize failed; build a new hierarchy");
        return AMG_ESTATE;
    }
    E.sealed = true;                      // the schedules below consume the host patterns: no setter may follow
    for (int l = 0; l < E.nlev; ++l) {
        XLevel<T> &L = E.lv[l];
        if (!L.A.set) { set_error("level " + std::to_string(l) + ": A missing"); return AMG_ESTATE; }
        if (L.A.nrows != L.A.ncols || L.A.R != L.A.C) { set_error("A must be square with square blocks"); return AMG_EINVAL; }
        const int n = L.A.nrows;
        if (l < E.nlev - 1) {
            const XMat<T> &An = E.lv[l + 1].A;
            if (!L.P.set || !L.R.set) { set_error("level " + std::to_string(l) + ": P or R missing"); return AMG_ESTATE; }
            if (L.P.nrows != n || L.P.ncols != An.nrows || L.R.nrows != An.nrows || L.R.ncols != n) {
                set_error("level " + std::to_string(l) + ": P / R shapes do not match A");
                return AMG_EINVAL;
            }
            for (int w = 0; w < 2; ++w) CHK(build_smoother(E, L, L.sm[w]));
        }
        const size_t vb = sizeof(T) * (size_t)n;
        for (DBuf *v : {&L.x, &L.b, &L.r, &L.h1, &L.h2, &L.t})
            if (!v->p) CHK(E.pool.alloc(*v, vb));
    }
    XLevel<T> &Lc = E.lv[E.nlev - 1];
    if (E.coarse == COARSE_SMOOTHER) CHK(build_smoother(E, Lc, E.csm));
    if (E.coarse == COARSE_DENSE && E.nM != Lc.A.nrows) { set_error("dense coarse operator has the wrong size"); return AMG_EINVAL; }
    if (!E.part.p) CHK(E.pool.alloc(E.part, sizeof(double) * NORM_BLOCKS));
    for (int l = 0; l < E.nlev; ++l) {             // the patterns served the schedules
        for (XMat<T> *M : {&E.lv[l].A, &E.lv[l].P, &E.lv[l].R, &E.lv[l].sm[0].Ab, &E.lv[l].sm[1].Ab}) {
            std::vector<int>().swap(M->hAp);
            std::vector<int>().swap(M->hAj);
        }
    }
    E.finalized = true;
    return 0;
}

template <class T>
int solve(Engine<T> &E, const void *b, void *x, double tol, int maxiter, int cyc, double *residuals, int *nres,
          int flags)
{
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (!b || !x || !residuals || !nres || maxiter < 0 || cyc < 0 || cyc > 2) {
        set_error(cyc == 3 ? "AMLI cycles are not implemented for this value type" : "bad solve arguments");
        return cyc == 3 ? AMG_ENOTIMPL : AMG_EINVAL;
    }
    if (E.nres_cap < maxiter + 2) {
        E.pool.bytes -= (long)sizeof(double) * E.nres_cap;
        if (E.res.p) AMG_HIP(hipFree(E.res.p));
        E.res.p = nullptr;
        CHK(E.pool.alloc(E.res, sizeof(double) * (size_t)(maxiter + 2)));
        E.nres_cap = maxiter + 2;
    }
    double *rd = E.res.d();
    CHK(load_vectors(E, b, x, flags));
    XLevel<T> &L0 = E.lv[0];
    double normb = 0.0;
    CHK(device_norm(E, (const T *)L0.b.p, L0.A.nrows, rd + maxiter + 1));            // multilevel.py:427-429
    AMG_HIP(hipMemcpyAsync(&normb, rd + maxiter + 1, sizeof(double), hipMemcpyDeviceToHost, E.st));
    CHK(residual_norm(E, rd));                                                        // :450
    AMG_HIP(hipMemcpyAsync(&residuals[0], rd, sizeof(double), hipMemcpyDeviceToHost, E.st));
    AMG_HIP(hipStreamSynchronize(E.st));
    if (normb != 0.0) tol = tol * normb;
    const bool fixed = (flags & AMG_SOLVE_NO_EARLY_STOP) != 0;
    int k = 1;
    AMG_HIP(hipEventRecord(E.ev0, E.st));
    while (k <= maxiter && (fixed || residuals[k - 1] > tol)) {                       // :454
        CHK(one_cycle(E, cyc));
        CHK(residual_norm(E, rd + k));
        if (!fixed) {
            AMG_HIP(hipMemcpyAsync(&residuals[k], rd + k, sizeof(double), hipMemcpyDeviceToHost, E.st));
            AMG_HIP(hipStreamSynchronize(E.st));
        }
        ++k;
    }
    AMG_HIP(hipEventRecord(E.ev1, E.st));
    if (fixed && k > 1)
        AMG_HIP(hipMemcpyAsync(residuals + 1, rd + 1, sizeof(double) * (size_t)(k - 1), hipMemcpyDeviceToHost, E.st));
    *nres = k;
    CHK(store_x(E, x));
    float ms = 0.f;
    AMG_HIP(hipEventElapsedTime(&ms, E.ev0, E.ev1));
    E.last_ms = ms;
    return 0;
}

template <class T>
int cycle(Engine<T> &E, const void *b, void *x, int cyc, int flags)
{
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (!b || !x || cyc < 0 || cyc > 2) {
        set_error(cyc == 3 ? "AMLI cycles are not implemented for this value type" : "bad cycle arguments");
        return cyc == 3 ? AMG_ENOTIMPL : AMG_EINVAL;
    }
    CHK(load_vectors(E, b, x, flags));
    AMG_HIP(hipEventRecord(E.ev0, E.st));
    CHK(one_cycle(E, cyc));
    AMG_HIP(hipEventRecord(E.ev1, E.st));
    CHK(store_x(E, x));
    float ms = 0.f;
    AMG_HIP(hipEventElapsedTime(&ms, E.ev0, E.ev1));
    E.last_ms = ms;
    return 0;
}

using C128 = Engine<c128>;

}  // namespace

// the handle: one engine per value type (complex128 only)
struct amg_hierx {
    int value_type = AMG_VALUE_C128;
    C128 e;
};

#define ENTERX(h)                                                       \
    if (!(h)) { amg::set_error("null hierarchy"); return AMG_EINVAL; }  \
    AMG_HIP(hipSetDevice((h)->e.device))
// setters: only before amg_hierx_finalize
#define UNSEALED(h)                                                                                       \
    if ((h)->e.sealed) {                                                                                  \
        amg::set_error("hierarchy already finalised: operators and solvers are set before amg_hierx_finalize"); \
        return AMG_ESTATE;                                                                                \
    }

extern "C" {

int amg_hierx_create(int value_type, int nlevels, int device, amg_hierx **out)
{
    if (!out) { set_error("null out"); return AMG_EINVAL; }
    *out = nullptr;
    if (value_type != AMG_VALUE_C128) {
        set_error("resident hierarchies of this value type are not implemented (complex128 only)");
        return AMG_ENOTIMPL;
    }
    if (nlevels < 1) { set_error("nlevels < 1"); return AMG_EINVAL; }
    CHK(require_device());
    AMG_HIP(hipSetDevice(device));
    amg_hierx *h = new amg_hierx();
    C128 &E = h->e;
    E.device = device;
    E.nlev = nlevels;
    E.lv.resize(nlevels);
    if (hipStreamCreateWithFlags(&E.st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&E.ev0) != hipSuccess || hipEventCreate(&E.ev1) != hipSuccess) {
        delete h;
        set_error("hipStreamCreate / hipEventCreate failed");
        return AMG_ENODEV;
    }
    *out = h;
    return 0;
}

void amg_hierx_destroy(amg_hierx *h)
{
    if (!h) return;
    hipSetDevice(h->e.device);
    hipDeviceSynchronize();
    delete h;
}

int amg_hierx_set_matrix(amg_hierx *h, int lvl, int which, int fmt, int nrows, int ncols, int R, int C,
                         const int *Ap, const int *Aj, const void *Ax)
{
    ENTERX(h);
    UNSEALED(h);
    C128 &E = h->e;
    if (lvl < 0 || lvl >= E.nlev || which < 0 || which > 2 || (which > 0 && lvl == E.nlev - 1)) {
        set_error("bad level / operator slot");
        return AMG_EINVAL;
    }
    XLevel<c128> &L = E.lv[lvl];
    XMat<c128> &M = which == 0 ? L.A : which == 1 ? L.P : L.R;
    if (M.set) { set_error("operator already set"); return AMG_ESTATE; }
    return M.load(E.pool, fmt, nrows, ncols, fmt ? R : 1, fmt ? C : 1, Ap, Aj, Ax);
}

int amg_hierx_set_smoother(amg_hierx *h, int lvl, int which, const amg_smoother_desc_x *d)
{
    ENTERX(h);
    UNSEALED(h);
    CHK(set_smoother(h->e, lvl, which, d));
    if (which == 2) h->e.coarse = COARSE_SMOOTHER;
    return 0;
}

int amg_hierx_set_block_matrix(amg_hierx *h, int lvl, int which, int nbrows, int bs, const int *Ap, const int *Aj,
                               const void *Ax)
{
    ENTERX(h);
    UNSEALED(h);
    C128 &E = h->e;
    if (lvl < 0 || lvl >= E.nlev || which < 0 || which > 2 || bs < 1 || nbrows < 0) { set_error("bad slot"); return AMG_EINVAL; }
    XSmoother<c128> &s = which == 2 ? E.csm : E.lv[lvl].sm[which];
    if ((s.kind != SM_BJACOBI && s.kind != SM_BGS) || s.bs != bs) {
        set_error("set the block smoother first, with the same blocksize");
        return AMG_ESTATE;
    }
    if (s.Ab.set) { set_error("block matrix already set"); return AMG_ESTATE; }
    return s.Ab.load(E.pool, 1, nbrows * bs, nbrows * bs, bs, bs, Ap, Aj, Ax);
}

int amg_hierx_set_coarse_dense(amg_hierx *h, const void *M, int n)
{
    ENTERX(h);
    UNSEALED(h);
    C128 &E = h->e;
    if (n < 0 || (!M && n)) { set_error("bad dense operator"); return AMG_EINVAL; }
    if (E.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    CHK(E.pool.upload(E.M, M, sizeof(c128) * (size_t)n * n));
    E.nM = n;
    E.coarse = COARSE_DENSE;
    return 0;
}

int amg_hierx_set_coarse_callback(amg_hierx *h, amg_coarse_callback_x fn, void *user)
{
    ENTERX(h);
    UNSEALED(h);
    if (!fn) { set_error("null callback"); return AMG_EINVAL; }
    if (h->e.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    h->e.cb = fn;
    h->e.cb_user = user;
    h->e.coarse = COARSE_CALLBACK;
    return 0;
}

int amg_hierx_finalize(amg_hierx *h)
{
    ENTERX(h);
    return finalize(h->e);
}

int amg_hierx_solve(amg_hierx *h, const void *b, void *x, double tol, int maxiter, int cyc, double *residuals,
                    int *nres, int flags)
{
    ENTERX(h);
    return solve(h->e, b, x, tol, maxiter, cyc, residuals, nres, flags);
}

int amg_hierx_cycle(amg_hierx *h, const void *b, void *x, int cyc, int flags)
{
    ENTERX(h);
    return cycle(h->e, b, x, cyc, flags);
}

long amg_hierx_device_bytes(amg_hierx *h) { return h ? h->e.pool.bytes : 0; }

double amg_hierx_last_solve_ms(amg_hierx *h) { return h ? h->e.last_ms : 0.0; }

}  // extern "C"
