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
#include "resident.hpp"
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
constexpr char FINALIZE[] = "amg_hierx_finalize";

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
struct Engine : Core {
    std::vector<XLevel<T>> lv;
    XSmoother<T> csm;                     // relaxation-named coarse solver
    amg_coarse_callback_x cb = nullptr;
    void *cb_user = nullptr;
    std::vector<T> hb, hx;
    DBuf kscr;                            // scratch of the amg_devx_* reductions, then one double for a norm
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

// the steps of a cycle (cycle_level, resident.hpp) on the levels' vectors
template <class T>
struct XCycle {
    Engine<T> &E;
    T *x(int l) const { return (T *)E.lv[l].x.p; }
    T *b(int l) const { return (T *)E.lv[l].b.p; }
    T *r(int l) const { return (T *)E.lv[l].r.p; }
    int relax(int l, int w) { return ::relax(E, E.lv[l], E.lv[l].sm[w], x(l), (const T *)b(l)); }
    int residual(int l) { return apply_rows(E.lv[l].A, (const T *)x(l), EpiResid<T>{b(l), r(l)}, E.st); }
    int restrict_residual(int l) { return apply_rows(E.lv[l].R, (const T *)r(l), EpiStore<T>{b(l + 1)}, E.st); }
    int zero_x(int l)
    {
        if (E.lv[l].A.nrows) AMG_HIP(hipMemsetAsync(x(l), 0, sizeof(T) * (size_t)E.lv[l].A.nrows, E.st));
        return 0;
    }
    int coarse_solve() { return ::coarse_solve(E, x(E.nlev - 1), (const T *)b(E.nlev - 1)); }
    int prolong_add(int l) { return apply_rows(E.lv[l].P, (const T *)x(l + 1), EpiAdd<T>{x(l)}, E.st); }
};

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
    CHK(XCycle<T>{E}.residual(0));
    return device_norm(E, (const T *)E.lv[0].r.p, E.lv[0].A.nrows, slot);
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
    XSmoother<T> *slot = nullptr;
    CHK(smoother_slot(E, lvl, which, d, SM_BGS, "for this value type", slot));
    XSmoother<T> &s = *slot;
    s.set = true;
    s.kind = d->kind;
    if (s.kind == SM_NONE) return 0;
    CHK(check_sweeps(d));
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

// what finalize (resident.hpp) leaves to this engine
template <class T>
struct XSetup {
    Engine<T> &E;
    int square(const XMat<T> &A)
    {
        if (A.nrows != A.ncols || A.R != A.C) { set_error("A must be square with square blocks"); return AMG_EINVAL; }
        return 0;
    }
    int build_smoother(XLevel<T> &L, XSmoother<T> &s) { return ::build_smoother(E, L, s); }
    int level_vectors(int l)
    {
        XLevel<T> &L = E.lv[l];
        for (DBuf *v : {&L.x, &L.b, &L.r, &L.h1, &L.h2, &L.t}) CHK(E.pool.alloc(*v, sizeof(T) * (size_t)L.A.nrows));
        return 0;
    }
    int finish()
    {
        CHK(E.pool.alloc(E.part, sizeof(double) * NORM_BLOCKS));
        for (XLevel<T> &L : E.lv)
            for (XSmoother<T> &s : L.sm) drop_pattern(s.Ab);
        return 0;
    }
};

template <class T>
int solve(Engine<T> &E, const void *b, void *x, double tol, int maxiter, int cyc, double *residuals, int *nres,
          int flags)
{
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (!b || !x || !residuals || !nres || maxiter < 0 || cyc < 0 || cyc > 2) {
        set_error(cyc == 3 ? "AMLI cycles are not implemented for this value type" : "bad solve arguments");
        return cyc == 3 ? AMG_ENOTIMPL : AMG_EINVAL;
    }
    CHK(E.reserve_history(maxiter, 1));
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
    return E.timed(
        [&]() -> int {
            while (k <= maxiter && (fixed || residuals[k - 1] > tol)) {               // :454
                CHK(one_cycle(XCycle<T>{E}, E.nlev, cyc));
                CHK(residual_norm(E, rd + k));
                if (!fixed) {
                    AMG_HIP(hipMemcpyAsync(&residuals[k], rd + k, sizeof(double), hipMemcpyDeviceToHost, E.st));
                    AMG_HIP(hipStreamSynchronize(E.st));
                }
                ++k;
            }
            return 0;
        },
        [&]() -> int {
            if (fixed && k > 1)
                AMG_HIP(hipMemcpyAsync(residuals + 1, rd + 1, sizeof(double) * (size_t)(k - 1), hipMemcpyDeviceToHost, E.st));
            *nres = k;
            return store_x(E, x);
        });
}

template <class T>
int cycle(Engine<T> &E, const void *b, void *x, int cyc, int flags)
{
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (!b || !x || cyc < 0 || cyc > 2) {
        set_error(cyc == 3 ? "AMLI cycles are not implemented for this value type" : "bad cycle arguments");
        return cyc == 3 ? AMG_ENOTIMPL : AMG_EINVAL;
    }
    if (flags & AMG_SOLVE_DEVICE_VECTORS) {         // b, x in HBM: copies on the stream, nothing waits for them
        XLevel<T> &L = E.lv[0];
        const size_t vbytes = sizeof(T) * (size_t)L.A.nrows;
        if (!vbytes) return 0;
        AMG_HIP(hipMemcpyAsync(L.b.p, b, vbytes, hipMemcpyDeviceToDevice, E.st));
        if (flags & AMG_SOLVE_X0_ZERO) AMG_HIP(hipMemsetAsync(L.x.p, 0, vbytes, E.st));
        else AMG_HIP(hipMemcpyAsync(L.x.p, x, vbytes, hipMemcpyDeviceToDevice, E.st));
        CHK(one_cycle(XCycle<T>{E}, E.nlev, cyc));
        AMG_HIP(hipMemcpyAsync(x, L.x.p, vbytes, hipMemcpyDeviceToDevice, E.st));
        return 0;
    }
    CHK(load_vectors(E, b, x, flags));
    return E.timed([&] { return one_cycle(XCycle<T>{E}, E.nlev, cyc); }, [&] { return store_x(E, x); });
}

// the scratch of the device Krylov methods: partial sums and result slots of zdotc, then the slot of a norm
constexpr size_t KSCR_VALUES = AMG_DEVX_PARTIALS + AMG_DEVX_SLOTS + 1;
template <class T>
int krylov_scratch(Engine<T> &E)
{
    if (E.kscr.p) return 0;
    CHK(E.pool.alloc(E.kscr, sizeof(T) * KSCR_VALUES));
    AMG_HIP(hipMemset(E.kscr.p, 0, sizeof(T) * KSCR_VALUES));
    return 0;
}

using C128 = Engine<c128>;

}  // namespace

// the handle: one engine per value type (complex128 only)
struct amg_hierx {
    int value_type = AMG_VALUE_C128;
    C128 e;
};

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
    return open_handle(nlevels, device, out);
}

void amg_hierx_destroy(amg_hierx *h) { close_handle(h); }

int amg_hierx_set_matrix(amg_hierx *h, int lvl, int which, int fmt, int nrows, int ncols, int R, int C,
                         const int *Ap, const int *Aj, const void *Ax)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    C128 &E = h->e;
    XMat<c128> *M = operator_slot(E, lvl, which);
    if (!M) return AMG_EINVAL;
    if (M->set) { set_error("operator already set"); return AMG_ESTATE; }
    return M->load(E.pool, fmt, nrows, ncols, fmt ? R : 1, fmt ? C : 1, Ap, Aj, Ax);
}

int amg_hierx_set_smoother(amg_hierx *h, int lvl, int which, const amg_smoother_desc_x *d)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    CHK(set_smoother(h->e, lvl, which, d));
    if (which == 2) h->e.coarse = COARSE_SMOOTHER;
    return 0;
}

int amg_hierx_set_block_matrix(amg_hierx *h, int lvl, int which, int nbrows, int bs, const int *Ap, const int *Aj,
                               const void *Ax)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
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
    ENTER(h);
    UNSEALED(h, FINALIZE);
    return set_coarse_dense(h->e, M, n, sizeof(c128));
}

int amg_hierx_set_coarse_callback(amg_hierx *h, amg_coarse_callback_x fn, void *user)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    if (!fn) { set_error("null callback"); return AMG_EINVAL; }
    if (h->e.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    h->e.cb = fn;
    h->e.cb_user = user;
    h->e.coarse = COARSE_CALLBACK;
    return 0;
}

int amg_hierx_finalize(amg_hierx *h)
{
    ENTER(h);
    return finalize(h->e, FINALIZE, XSetup<c128>{h->e});
}

int amg_hierx_solve(amg_hierx *h, const void *b, void *x, double tol, int maxiter, int cyc, double *residuals,
                    int *nres, int flags)
{
    ENTER(h);
    return solve(h->e, b, x, tol, maxiter, cyc, residuals, nres, flags);
}

int amg_hierx_cycle(amg_hierx *h, const void *b, void *x, int cyc, int flags)
{
    ENTER(h);
    return cycle(h->e, b, x, cyc, flags);
}

void *amg_hierx_stream(amg_hierx *h) { return h ? (void *)h->e.st : nullptr; }

int amg_hierx_level_size(amg_hierx *h, int lvl)
{
    if (!h || lvl < 0 || lvl >= h->e.nlev || !h->e.lv[lvl].A.set) return -1;
    return h->e.lv[lvl].A.nrows;
}

int amg_hierx_apply(amg_hierx *h, int lvl, const void *x_dev, void *y_dev)
{
    ENTER(h);
    C128 &E = h->e;
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (lvl < 0 || lvl >= E.nlev || !x_dev || !y_dev || x_dev == y_dev) { set_error("bad apply arguments"); return AMG_EINVAL; }
    return apply_rows(E.lv[lvl].A, (const c128 *)x_dev, EpiStore<c128>{(c128 *)y_dev}, E.st);
}

void *amg_hierx_vec_alloc(amg_hierx *h, long n)
{
    if (!h || n < 0 || hipSetDevice(h->e.device) != hipSuccess) { set_error("bad vector allocation"); return nullptr; }
    void *p = nullptr;
    const size_t bytes = sizeof(c128) * (size_t)n;
    if (hipMalloc(&p, bytes + 128) != hipSuccess) { set_error("device allocation failed"); return nullptr; }
    if (hipMemset(p, 0, bytes + 128) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        hipFree(p);
        set_error("device allocation failed");
        return nullptr;
    }
    h->e.pool.bytes += (long)bytes;
    return p;
}

void amg_hierx_vec_free(amg_hierx *h, void *p, long n)
{
    if (!h || !p) return;
    hipSetDevice(h->e.device);
    hipStreamSynchronize(h->e.st);
    hipFree(p);
    h->e.pool.bytes -= (long)(sizeof(c128) * (size_t)n);
}

void *amg_hierx_scratch(amg_hierx *h)
{
    if (!h || hipSetDevice(h->e.device) != hipSuccess || krylov_scratch(h->e) != 0) return nullptr;
    return h->e.kscr.p;
}

int amg_hierx_norm(amg_hierx *h, const void *v_dev, long n, double *host)
{
    ENTER(h);
    C128 &E = h->e;
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (!v_dev || !host || n < 0) { set_error("bad norm arguments"); return AMG_EINVAL; }
    CHK(krylov_scratch(E));
    double *slot = (double *)((c128 *)E.kscr.p + AMG_DEVX_PARTIALS + AMG_DEVX_SLOTS);
    CHK(device_norm(E, (const c128 *)v_dev, n, slot));
    AMG_HIP(hipMemcpyAsync(host, slot, sizeof(double), hipMemcpyDeviceToHost, E.st));
    AMG_HIP(hipStreamSynchronize(E.st));
    return 0;
}

long amg_hierx_device_bytes(amg_hierx *h) { return h ? h->e.pool.bytes : 0; }

double amg_hierx_last_solve_ms(amg_hierx *h) { return h ? h->e.last_ms : 0.0; }

}  // extern "C"
