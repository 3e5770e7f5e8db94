// Resident float64 hierarchies for SEVERAL right-hand sides (include/amgcore_hip.h, section 6): the cycle of
// multilevel.py:316-548 applied to k vectors at once.  Every operator entry is read once per application and applied
// to all columns; every Gauss-Seidel dependency level is one launch for all columns.
//
// Layout: every work vector of a level is double v[n][KP], column fastest, KP in {1, 2, 4, 8} (template parameter);
// k columns run at the next width, the padding columns are zero, never reported and never waited for.  A gathered
// operand row v[j][0..KP) is 8 KP contiguous bytes: KP / 2 lanes share a row and load 16 bytes each.
//
// Arithmetic: per column every iterate has the bits of the one-vector engine and of the
// reference -- each row sum runs left to right over the row's stored entries, multiply and add rounded separately
// (the library builds with -ffp-contract=off), epilogues parenthesised as in relaxation.h / relaxation.py.  No
// kernel mixes columns, so a column's bits do not depend on k, on its position or on its neighbours.  The residual
// norm of a column is a two-stage reduction over a fixed grid: its tree depends on n only.
#include "resident.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace amg;

namespace {

constexpr int KMAX = 8;             // widest layout
constexpr int ROWS_WG = 256;        // lanes of one operator workgroup
constexpr int CHUNK = 2048;         // entries (column, value) staged in LDS at a time
constexpr int LEVEL_WG = 64;        // threads of a Gauss-Seidel level launch
constexpr int NORM_BLOCKS = 2048;   // partial sums of a norm: fixed, so the tree depends on n only
constexpr int NORM_WG = 256;
constexpr int VEC_WG = 256;

constexpr char FINALIZE[] = "amg_hierm_finalize";
// how a row is summed: from zero over all entries (products), from zero without the diagonal (jacobi, gauss_seidel),
// or bsr_jacobi / bsr_gauss_seidel with 1 x 1 blocks: from b[i], every off-diagonal block's product (0 + a x)
// subtracted in stored order
enum { ROW_SUM = 0, ROW_OFFDIAG = 1, ROW_BSR1 = 2 };

// one row of a vector: KP doubles
template <int KP> struct Row { double v[KP]; };

template <int KP> __device__ __forceinline__ Row<KP> ldrow(const double *p)
{
    Row<KP> r;
    if constexpr (KP == 1) {
        r.v[0] = p[0];
    } else {
        const double2 *q = reinterpret_cast<const double2 *>(p);      // rows of KP >= 2 doubles are 16-byte aligned
#pragma unroll
        for (int c = 0; c < KP / 2; ++c) {
            const double2 d = q[c];
            r.v[2 * c] = d.x;
            r.v[2 * c + 1] = d.y;
        }
    }
    return r;
}

template <int KP> __device__ __forceinline__ void strow(double *p, const Row<KP> &r)
{
    if constexpr (KP == 1) {
        p[0] = r.v[0];
    } else {
        double2 *q = reinterpret_cast<double2 *>(p);
#pragma unroll
        for (int c = 0; c < KP / 2; ++c) q[c] = make_double2(r.v[2 * c], r.v[2 * c + 1]);
    }
}

// ----------------------------------------------------------------------------------------------- row epilogues
// called with the offset off = i KP + c of a lane's CW columns of row i, their sums and the row's diagonal entry (0 when the row stores none or the mode keeps it in the sum)
template <int CW> struct EpiStore {            // y = A v (from zero)
    double *y;
    __device__ void operator()(long off, const Row<CW> &acc, double) const { strow<CW>(y + off, acc); }
};
template <int CW> struct EpiResid {            // r = b - (A v)
    const double *b;
    double *r;
    __device__ void operator()(long off, const Row<CW> &acc, double) const
    {
        const Row<CW> bi = ldrow<CW>(b + off);
        Row<CW> o;
#pragma unroll
        for (int c = 0; c < CW; ++c) o.v[c] = bi.v[c] - acc.v[c];
        strow<CW>(r + off, o);
    }
};
template <int CW> struct EpiAdd {              // x += (A v)
    double *x;
    __device__ void operator()(long off, const Row<CW> &acc, double) const
    {
        Row<CW> o = ldrow<CW>(x + off);
#pragma unroll
        for (int c = 0; c < CW; ++c) o.v[c] = o.v[c] + acc.v[c];
        strow<CW>(x + off, o);
    }
};
// polynomial, first step (relaxation.py:655-663): residual = b - A x; h = c0 * residual
template <int CW> struct EpiPoly0 {
    const double *b;
    double *r, *h;
    double c0;
    __device__ void operator()(long off, const Row<CW> &acc, double) const
    {
        const Row<CW> bi = ldrow<CW>(b + off);
        Row<CW> ri, hi;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            ri.v[c] = bi.v[c] - acc.v[c];
            hi.v[c] = c0 * ri.v[c];
        }
        strow<CW>(r + off, ri);
        strow<CW>(h + off, hi);
    }
};
// later steps (relaxation.py:666): h = c * residual + A h; the last one adds h to x (:668) instead of storing it
template <int CW> struct EpiPolyStep {
    const double *r;
    double *hout, *x;
    double cf;
    int last;
    __device__ void operator()(long off, const Row<CW> &acc, double) const
    {
        const Row<CW> ri = ldrow<CW>(r + off);
        Row<CW> hi;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const double cr = cf * ri.v[c];
            hi.v[c] = cr + acc.v[c];
        }
        if (last) {
            Row<CW> xi = ldrow<CW>(x + off);
#pragma unroll
            for (int c = 0; c < CW; ++c) xi.v[c] = xi.v[c] + hi.v[c];
            strow<CW>(x + off, xi);
        } else {
            strow<CW>(hout + off, hi);
        }
    }
};
// jacobi (relaxation.h:202-239), ROW_OFFDIAG sums: x = (1 - w) temp + w ((b - rsum) / diag).  x holds a copy of
// temp on entry, so a row without a usable diagonal is left alone.
template <int CW> struct EpiJacobi {
    const double *temp, *b;
    double *x;
    double w;
    __device__ void operator()(long off, const Row<CW> &acc, double diag) const
    {
        if (diag == 0.0) return;
        const Row<CW> ti = ldrow<CW>(temp + off), bi = ldrow<CW>(b + off);
        Row<CW> o;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const double q = (bi.v[c] - acc.v[c]) / diag;
            const double t1 = (1.0 - w) * ti.v[c];
            const double t2 = w * q;
            o.v[c] = t1 + t2;
        }
        strow<CW>(x + off, o);
    }
};
// bsr_jacobi with 1 x 1 blocks (relaxation.h:268-360), ROW_BSR1 sums (acc = b - off-diagonal products):
// x = (1 - w) temp + (w acc) / diag
template <int CW> struct EpiJacobiBsr1 {
    const double *temp;
    double *x;
    double w;
    __device__ void operator()(long off, const Row<CW> &acc, double diag) const
    {
        if (diag == 0.0) return;
        const Row<CW> ti = ldrow<CW>(temp + off);
        Row<CW> o;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const double t1 = (1.0 - w) * ti.v[c];
            const double t2 = (w * acc.v[c]) / diag;
            o.v[c] = t1 + t2;
        }
        strow<CW>(x + off, o);
    }
};

// ----------------------------------------------------------------------------------------------- kernels
// Operator rows for KP columns: the (column, value) pairs of a workgroup's rows are one contiguous slice, staged in
// LDS a chunk at a time with coalesced loads -- every entry leaves HBM once.  A row is shared by KP / 2 lanes, each
// holding the running sums of two columns in registers and gathering its 16 bytes of every operand row (one lane
// per row for KP = 1, 2): the lanes of a row load 8 KP contiguous bytes, and a workgroup of 256 lanes covers
// 512 / KP rows, so that at 8 columns the ~2000 entries of 64 rows of a Galerkin operator (about 31 per row) are ONE
// chunk and every lane works between the two barriers.  Each column's sum runs in stored order in one lane.
template <int KP> struct Shape {
    static constexpr int CW = KP >= 2 ? 2 : 1;          // columns per lane
    static constexpr int LPR = KP / CW;                 // lanes per row
    static constexpr int ROWS = ROWS_WG / LPR;          // rows per workgroup
};

template <int KP, int MODE, class Epi>
__global__ void __launch_bounds__(ROWS_WG)
csr_rows_multi(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
               const double *__restrict__ v, const double *__restrict__ b0, Epi epi)
{
    constexpr int CW = Shape<KP>::CW, LPR = Shape<KP>::LPR, ROWS = Shape<KP>::ROWS;
    __shared__ int sj[CHUNK];
    __shared__ double sa[CHUNK];
    const int r0 = blockIdx.x * ROWS;
    const int r1 = min(n, r0 + ROWS);
    const int i = r0 + (int)threadIdx.x / LPR;
    const int cb = ((int)threadIdx.x % LPR) * CW;       // this lane's first column
    const bool mine = i < r1;
    const int e0 = Ap[r0], e1 = Ap[r1];
    const int rs = mine ? Ap[i] : 0, re = mine ? Ap[i + 1] : 0;
    const long o = (long)i * KP + cb;
    Row<CW> acc;
#pragma unroll
    for (int c = 0; c < CW; ++c) acc.v[c] = 0.0;
    if (MODE == ROW_BSR1 && mine) acc = ldrow<CW>(b0 + o);
    double diag = 0.0;
    for (int c0 = e0; c0 < e1; c0 += CHUNK) {
        const int cn = min(CHUNK, e1 - c0);
        for (int k = threadIdx.x; k < cn; k += ROWS_WG) {
            sj[k] = Aj[c0 + k];
            sa[k] = Ax[c0 + k];
        }
        __syncthreads();
        const int a = max(rs, c0), z = min(re, c0 + cn);
        for (int k = a; k < z; ++k) {
            const int j = sj[k - c0];
            const double aij = sa[k - c0];
            if (MODE != ROW_SUM && j == i) {
                diag = aij;
                continue;
            }
            const Row<CW> xv = ldrow<CW>(v + (long)j * KP + cb);
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (MODE == ROW_BSR1) {
                    const double loc = 0.0 + aij * xv.v[c];
                    acc.v[c] = acc.v[c] - loc;
                } else {
                    const double p = aij * xv.v[c];
                    acc.v[c] = acc.v[c] + p;
                }
            }
        }
        __syncthreads();
    }
    if (mine) epi(o, acc, diag);
}

// The same rows without the LDS stage, for operators with short rows (stencils: 7 entries per row): the KP / 2 lanes of
// a row read the row's entries themselves (the same address in all of them: one request; consecutive rows'
// entries are adjacent, so a wave's loads walk the same few cache lines) -- no staging stores, no barrier, and the
// loads of several entries can be in flight at once.  Same sums in the same order as csr_rows_multi.
template <int KP, int MODE, class Epi>
__global__ void __launch_bounds__(ROWS_WG)
csr_rows_direct(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                const double *__restrict__ v, const double *__restrict__ b0, Epi epi)
{
    constexpr int CW = Shape<KP>::CW, LPR = Shape<KP>::LPR, ROWS = Shape<KP>::ROWS;
    const int i = blockIdx.x * ROWS + (int)threadIdx.x / LPR;
    if (i >= n) return;
    const int cb = ((int)threadIdx.x % LPR) * CW;
    const long o = (long)i * KP + cb;
    Row<CW> acc;
#pragma unroll
    for (int c = 0; c < CW; ++c) acc.v[c] = 0.0;
    if (MODE == ROW_BSR1) acc = ldrow<CW>(b0 + o);
    double diag = 0.0;
    const int rs = Ap[i], re = Ap[i + 1];
#pragma unroll 4
    for (int k = rs; k < re; ++k) {
        const int j = Aj[k];
        const double aij = Ax[k];
        if (MODE != ROW_SUM && j == i) {
            diag = aij;
            continue;
        }
        const Row<CW> xv = ldrow<CW>(v + (long)j * KP + cb);
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (MODE == ROW_BSR1) {
                const double loc = 0.0 + aij * xv.v[c];
                acc.v[c] = acc.v[c] - loc;
            } else {
                const double p = aij * xv.v[c];
                acc.v[c] = acc.v[c] + p;
            }
        }
    }
    epi(o, acc, diag);
}

// One dependency level of a Gauss-Seidel sweep for KP columns: a lane per row of the level, the row's entries read
// once.  CSR (relaxation.h:34-62): x = (b - rsum) / diag; BSR 1 x 1 (relaxation.h:90-173): x = (b - p1 - p2 ..) / diag.
template <int KP, bool BSR1>
__global__ void __launch_bounds__(LEVEL_WG)
gs_level_multi(const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax, double *x,
               const double *__restrict__ b, const int *__restrict__ rows, int count)
{
    const int t = blockIdx.x * LEVEL_WG + threadIdx.x;
    if (t >= count) return;
    const int i = rows[t];
    const Row<KP> bi = ldrow<KP>(b + (long)i * KP);
    Row<KP> acc;
#pragma unroll
    for (int c = 0; c < KP; ++c) acc.v[c] = BSR1 ? bi.v[c] : 0.0;
    double diag = 0.0;
    const int rs = Ap[i], re = Ap[i + 1];
    for (int jj = rs; jj < re; ++jj) {
        const int j = Aj[jj];
        const double aij = Ax[jj];
        if (j == i) {
            diag = aij;
            continue;
        }
        const Row<KP> xv = ldrow<KP>(x + (long)j * KP);
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (BSR1) {
                const double loc = 0.0 + aij * xv.v[c];
                acc.v[c] = acc.v[c] - loc;
            } else {
                const double p = aij * xv.v[c];
                acc.v[c] = acc.v[c] + p;
            }
        }
    }
    if (diag == 0.0) return;
    Row<KP> o;
#pragma unroll
    for (int c = 0; c < KP; ++c) o.v[c] = BSR1 ? acc.v[c] / diag : (bi.v[c] - acc.v[c]) / diag;
    strow<KP>(x + (long)i * KP, o);
}

// x += h over all n KP entries
__global__ void add_to_multi(long m, double *__restrict__ x, const double *__restrict__ h)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) x[i] = x[i] + h[i];
}

// sor (relaxation.py:166-168): x *= omega; x_old *= (1 - omega); x += x_old
__global__ void sor_blend_multi(long m, double *__restrict__ x, const double *__restrict__ xold, double omega)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) {
        const double a = x[i] * omega;
        const double b = xold[i] * (1.0 - omega);
        x[i] = a + b;
    }
}

// dense coarse operator M (row-major n x n) for KP columns: x[i][c] = sum_k M[i][k] b[k][c], from zero, left to right
// (the row sums of amg_dev_dense_apply).  The KP lanes of a row read the same M entry: one request.
template <int KP>
__global__ void dense_apply_multi(int n, const double *__restrict__ M, const double *__restrict__ b, double *__restrict__ x)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = t / KP;
    const int c = (int)(t - i * KP);
    if (i >= n) return;
    const double *row = M + i * n;
    double s = 0.0;
    for (int k = 0; k < n; ++k) s = s + row[k] * b[(long)k * KP + c];
    x[i * KP + c] = s;
}

// column j of src into column j of dst (the iterate of a column at the moment it stopped)
template <int KP>
__global__ void snapshot_column(long n, int j, const double *__restrict__ src, double *__restrict__ dst)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i * KP + j] = src[i * KP + j];
}

// per-column ||v||^2 in two stages over a FIXED grid: lane t of workgroup w adds rows w 256 + t, + 2048 256, ... in
// order, a binary tree joins the lanes, then one workgroup joins the 2048 partial sums the same way and takes the
// roots.  Columns never meet: the tree of a column depends on n only.
template <int KP>
__global__ void __launch_bounds__(NORM_WG) norm_partial_multi(const double *__restrict__ v, long n, double *__restrict__ part)
{
    __shared__ double s[KP][NORM_WG];
    Row<KP> acc;
#pragma unroll
    for (int c = 0; c < KP; ++c) acc.v[c] = 0.0;
    for (long k = (long)blockIdx.x * NORM_WG + threadIdx.x; k < n; k += (long)NORM_BLOCKS * NORM_WG) {
        const Row<KP> r = ldrow<KP>(v + k * KP);
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const double q = r.v[c] * r.v[c];
            acc.v[c] = acc.v[c] + q;
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c][threadIdx.x] = acc.v[c];
    __syncthreads();
    for (int w = NORM_WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int c = 0; c < KP; ++c) s[c][threadIdx.x] = s[c][threadIdx.x] + s[c][threadIdx.x + w];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < KP) part[(long)blockIdx.x * KMAX + threadIdx.x] = s[threadIdx.x][0];
}

__global__ void __launch_bounds__(NORM_WG) norm_final_multi(const double *__restrict__ part, int kp, double *__restrict__ out)
{
    __shared__ double s[NORM_WG];
    for (int c = 0; c < kp; ++c) {
        double acc = 0.0;
        for (int k = threadIdx.x; k < NORM_BLOCKS; k += NORM_WG) acc = acc + part[(long)k * KMAX + c];
        s[threadIdx.x] = acc;
        __syncthreads();
        for (int w = NORM_WG / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[c] = sqrt(s[0]);
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------- host side
int width_of(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

// one operator: CSR, or BSR with 1 x 1 blocks (the same arrays; the flag selects the bsr_* rounding of the relaxations)
struct MMat {
    bool set = false;
    int bsr = 0, nrows = 0, ncols = 0;
    long nnz = 0;
    DBuf Ap, Aj, Ax;
    std::vector<int> hAp, hAj;      // the pattern on the host until the schedules are built
    int load(Pool &pool, int fmt, int nr, int nc, const int *ap, const int *aj, const double *ax)
    {
        if (nr < 0 || nc < 0) { set_error("bad shape"); return AMG_EINVAL; }
        if (!ap || ((!aj || !ax) && ap[0] != ap[nr])) { set_error("null array"); return AMG_EINVAL; }
        bsr = fmt;
        nrows = nr, ncols = nc;
        CHK(check_pattern(ap, nr, aj, nc));
        nnz = ap[nr];
        CHK(pool.upload(Ap, ap, sizeof(int) * (size_t)(nr + 1)));
        CHK(pool.upload(Aj, aj, sizeof(int) * (size_t)nnz));
        CHK(pool.upload(Ax, ax, sizeof(double) * (size_t)nnz));
        hAp.assign(ap, ap + nr + 1);
        hAj.assign(aj, aj + nnz);
        set = true;
        return 0;
    }
};

struct MSmoother {
    bool set = false;
    int kind = AMG_SM_NONE, iterations = 1, sweep = 0;
    double omega = 1.0;
    std::vector<double> coef;
    Sweep fwd, bwd;
};

struct MLevel {
    MMat A, P, R;
    MSmoother sm[2];
    DBuf x, b, r, h1, h2, t;     // iterate, right-hand side, residual, polynomial ping-pong, jacobi / sor copy
};

struct Engine : Core {
    int kmax = 1, kpmax = 1;
    std::vector<MLevel> lv;
    MSmoother csm;                        // relaxation-named coarse solver
    DBuf xs;                              // the iterates of the columns that stopped
    std::vector<double> hb, hx;           // packing of k != KP columns
};

// operators of up to DIRECT_MAX_ROW entries per row on average skip the LDS stage (AMG_MULTI_DIRECT=0: never; A/B runs)
constexpr int DIRECT_MAX_ROW = 12;
bool direct_rows()
{
    static const bool on = !(std::getenv("AMG_MULTI_DIRECT") && std::atoi(std::getenv("AMG_MULTI_DIRECT")) == 0);
    return on;
}

// rows of v through A for KP columns, each row's sums handed to epi
template <int KP, int MODE, class Epi>
int apply_rows(const MMat &A, const double *v, const double *b0, Epi epi, hipStream_t st)
{
    if (A.nrows == 0) return 0;
    const dim3 grid(blocks_of(A.nrows, Shape<KP>::ROWS));
    if (A.nnz <= (long)DIRECT_MAX_ROW * A.nrows && direct_rows())
        hipLaunchKernelGGL((csr_rows_direct<KP, MODE, Epi>), grid, dim3(ROWS_WG), 0, st, A.nrows, A.Ap.i(), A.Aj.i(),
                           A.Ax.d(), v, b0, epi);
    else
        hipLaunchKernelGGL((csr_rows_multi<KP, MODE, Epi>), grid, dim3(ROWS_WG), 0, st, A.nrows, A.Ap.i(), A.Aj.i(),
                           A.Ax.d(), v, b0, epi);
    return launched("operator rows");
}

// ----------------------------------------------------------------------------------------------- smoothers
template <int KP>
int gs_sweep(const MMat &A, double *x, const double *b, const Sweep &S, hipStream_t st)
{
    for (size_t l = 0; l + 1 < S.lp.size(); ++l) {
        const int off = S.lp[l], cnt = S.lp[l + 1] - S.lp[l];
        if (cnt <= 0) continue;
        if (A.bsr)
            hipLaunchKernelGGL((gs_level_multi<KP, true>), dim3(blocks_of(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, st,
                               A.Ap.i(), A.Aj.i(), A.Ax.d(), x, b, S.rows.i() + off, cnt);
        else
            hipLaunchKernelGGL((gs_level_multi<KP, false>), dim3(blocks_of(cnt, LEVEL_WG)), dim3(LEVEL_WG), 0, st,
                               A.Ap.i(), A.Aj.i(), A.Ax.d(), x, b, S.rows.i() + off, cnt);
        CHK(launched("gs_level_multi"));
    }
    return 0;
}

// one application of smoother s on level L: x relaxed in place for right-hand side b
template <int KP>
int relax(Engine &E, MLevel &L, const MSmoother &s, double *x, const double *b)
{
    hipStream_t st = E.st;
    const MMat &A = L.A;
    const int n = A.nrows;
    const long m = (long)n * KP;
    double *t = L.t.d();
    const size_t vbytes = sizeof(double) * (size_t)m;
    if (n == 0) return 0;
    auto sweeps = [&]() -> int {                    // one gauss_seidel(iterations=1, sweep) call
        if (s.sweep != AMG_SWEEP_BACKWARD) CHK(gs_sweep<KP>(A, x, b, s.fwd, st));
        if (s.sweep != AMG_SWEEP_FORWARD) CHK(gs_sweep<KP>(A, x, b, s.bwd, st));
        return 0;
    };
    switch (s.kind) {
    case AMG_SM_NONE:
        return 0;
    case AMG_SM_GAUSS_SEIDEL:
        for (int it = 0; it < s.iterations; ++it) CHK(sweeps());
        return 0;
    case AMG_SM_SOR:
        for (int it = 0; it < s.iterations; ++it) {
            AMG_HIP(hipMemcpyAsync(t, x, vbytes, hipMemcpyDeviceToDevice, st));
            CHK(sweeps());
            hipLaunchKernelGGL(sor_blend_multi, dim3(blocks_of(m, VEC_WG)), dim3(VEC_WG), 0, st, m, x, (const double *)t, s.omega);
            CHK(launched("sor blend"));
        }
        return 0;
    case AMG_SM_JACOBI:
        for (int it = 0; it < s.iterations; ++it) {
            AMG_HIP(hipMemcpyAsync(t, x, vbytes, hipMemcpyDeviceToDevice, st));     // relaxation.h:216-218
            if (A.bsr)
                CHK((apply_rows<KP, ROW_BSR1>(A, (const double *)t, b, EpiJacobiBsr1<Shape<KP>::CW>{t, x, s.omega}, st)));
            else
                CHK((apply_rows<KP, ROW_OFFDIAG>(A, (const double *)t, b, EpiJacobi<Shape<KP>::CW>{t, b, x, s.omega}, st)));
        }
        return 0;
    case AMG_SM_POLYNOMIAL: {
        // relaxation.py:655-668.  norm(x) == 0 selects residual = b; for finite A, b - A 0 is b bit for bit, so the
        // residual is always formed as b - A x.
        const int nc = (int)s.coef.size();
        double *r = L.r.d(), *h = L.h1.d(), *h2 = L.h2.d();
        for (int it = 0; it < s.iterations; ++it) {
            CHK((apply_rows<KP, ROW_SUM>(A, (const double *)x, nullptr, EpiPoly0<Shape<KP>::CW>{b, r, h, s.coef[0]}, st)));
            if (nc == 1) {
                hipLaunchKernelGGL(add_to_multi, dim3(blocks_of(m, VEC_WG)), dim3(VEC_WG), 0, st, m, x, (const double *)h);
                CHK(launched("polynomial update"));
            }
            for (int k = 1; k < nc; ++k) {
                const bool last = k == nc - 1;
                CHK((apply_rows<KP, ROW_SUM>(A, (const double *)h, nullptr, EpiPolyStep<Shape<KP>::CW>{r, h2, x, s.coef[k], last ? 1 : 0}, st)));
                std::swap(h, h2);
            }
        }
        return 0;
    }
    }
    set_error("unknown smoother kind");
    return AMG_EINVAL;
}

// coarse solve of the last level: x = coarse_solver(A, b)
template <int KP>
int coarse_solve(Engine &E, double *x, const double *b)
{
    MLevel &L = E.lv[E.nlev - 1];
    const int n = L.A.nrows;
    const size_t vbytes = sizeof(double) * (size_t)n * KP;
    if (n == 0) return 0;
    switch (E.coarse) {
    case COARSE_NONE:
        AMG_HIP(hipMemsetAsync(x, 0, vbytes, E.st));
        return 0;
    case COARSE_DENSE:
        hipLaunchKernelGGL(dense_apply_multi<KP>, dim3(blocks_of((long)n * KP, VEC_WG)), dim3(VEC_WG), 0, E.st, n,
                           (const double *)E.M.d(), b, x);
        return launched("dense coarse apply");
    case COARSE_SMOOTHER:
        AMG_HIP(hipMemsetAsync(x, 0, vbytes, E.st));
        return relax<KP>(E, L, E.csm, x, b);
    }
    set_error("no coarse solver");
    return AMG_ESTATE;
}

// the steps of a cycle (cycle_level, resident.hpp) on the levels' vectors, KP columns wide
template <int KP>
struct MCycle {
    static constexpr int CW = Shape<KP>::CW;
    Engine &E;
    double *x(int l) const { return E.lv[l].x.d(); }
    double *b(int l) const { return E.lv[l].b.d(); }
    double *r(int l) const { return E.lv[l].r.d(); }
    template <class Epi> int rows(const MMat &A, const double *v, Epi epi) { return apply_rows<KP, ROW_SUM>(A, v, nullptr, epi, E.st); }
    int relax(int l, int w) { return ::relax<KP>(E, E.lv[l], E.lv[l].sm[w], x(l), b(l)); }
    int residual(int l) { return rows(E.lv[l].A, x(l), EpiResid<CW>{b(l), r(l)}); }
    int restrict_residual(int l) { return rows(E.lv[l].R, r(l), EpiStore<CW>{b(l + 1)}); }
    int zero_x(int l)
    {
        if (E.lv[l].A.nrows) AMG_HIP(hipMemsetAsync(x(l), 0, sizeof(double) * (size_t)E.lv[l].A.nrows * KP, E.st));
        return 0;
    }
    int coarse_solve() { return ::coarse_solve<KP>(E, x(E.nlev - 1), b(E.nlev - 1)); }
    int prolong_add(int l) { return rows(E.lv[l].P, x(l + 1), EpiAdd<CW>{x(l)}); }
};

// out[0..KP) = the columns' norms
template <int KP>
int device_norm(Engine &E, const double *v, long n, double *out)
{
    hipLaunchKernelGGL(norm_partial_multi<KP>, dim3(NORM_BLOCKS), dim3(NORM_WG), 0, E.st, v, n, E.part.d());
    CHK(launched("norm partial"));
    hipLaunchKernelGGL(norm_final_multi, dim3(1), dim3(NORM_WG), 0, E.st, (const double *)E.part.d(), KP, out);
    return launched("norm final");
}

// slot[0..KP) = ||b - A x|| of every column on level 0
template <int KP>
int residual_norm(Engine &E, double *slot)
{
    CHK(MCycle<KP>{E}.residual(0));
    return device_norm<KP>(E, E.lv[0].r.d(), E.lv[0].A.nrows, slot);
}

// host (n, k) row-major -> device [n][KP], padding columns zero
template <int KP>
int upload_columns(Engine &E, std::vector<double> &stage, const double *src, int k, double *dst)
{
    const long n = E.lv[0].A.nrows;
    if (!n) return 0;
    if (k == KP) {
        AMG_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n * KP, hipMemcpyHostToDevice, E.st));
        return 0;
    }
    stage.assign((size_t)n * KP, 0.0);
    for (long i = 0; i < n; ++i)
        for (int c = 0; c < k; ++c) stage[(size_t)i * KP + c] = src[(size_t)i * k + c];
    AMG_HIP(hipMemcpyAsync(dst, stage.data(), sizeof(double) * (size_t)n * KP, hipMemcpyHostToDevice, E.st));
    return 0;
}

template <int KP>
int load_vectors(Engine &E, int k, const double *B, const double *X, int flags)
{
    MLevel &L = E.lv[0];
    CHK(upload_columns<KP>(E, E.hb, B, k, L.b.d()));
    if (flags & AMG_SOLVE_X0_ZERO) {
        if (L.A.nrows) AMG_HIP(hipMemsetAsync(L.x.d(), 0, sizeof(double) * (size_t)L.A.nrows * KP, E.st));
    } else {
        CHK(upload_columns<KP>(E, E.hx, X, k, L.x.d()));
    }
    return 0;
}

// device [n][KP] -> host (n, k); synchronises the stream
template <int KP>
int store_columns(Engine &E, const double *src, int k, double *X)
{
    const long n = E.lv[0].A.nrows;
    if (n && k == KP) {
        AMG_HIP(hipMemcpyAsync(X, src, sizeof(double) * (size_t)n * KP, hipMemcpyDeviceToHost, E.st));
    } else if (n) {
        E.hx.resize((size_t)n * KP);
        AMG_HIP(hipMemcpyAsync(E.hx.data(), src, sizeof(double) * (size_t)n * KP, hipMemcpyDeviceToHost, E.st));
    }
    AMG_HIP(hipStreamSynchronize(E.st));
    if (n && k != KP)
        for (long i = 0; i < n; ++i)
            for (int c = 0; c < k; ++c) X[(size_t)i * k + c] = E.hx[(size_t)i * KP + c];
    return 0;
}

template <int KP>
int snapshot(Engine &E, int j)
{
    const long n = E.lv[0].A.nrows;
    if (!n) return 0;
    hipLaunchKernelGGL(snapshot_column<KP>, dim3(blocks_of(n, VEC_WG)), dim3(VEC_WG), 0, E.st, n, j,
                       (const double *)E.lv[0].x.d(), E.xs.d());
    return launched("snapshot");
}

template <int KP>
int solve_kp(Engine &E, int k, const double *B, double *X, double tol, int maxiter, int cyc, double *residuals,
             int *nres, int flags)
{
    const int stride = maxiter + 1;                   // of a column's history in residuals
    double *rd = E.res.d();                           // (maxiter + 2) slots of KMAX doubles; the last: ||b_j||
    CHK(load_vectors<KP>(E, k, B, X, flags));
    MLevel &L0 = E.lv[0];
    double normb[KMAX], cur[KMAX], tolj[KMAX];
    CHK(device_norm<KP>(E, L0.b.d(), L0.A.nrows, rd + (long)(maxiter + 1) * KMAX));       // multilevel.py:427-429
    AMG_HIP(hipMemcpyAsync(normb, rd + (long)(maxiter + 1) * KMAX, sizeof(double) * KP, hipMemcpyDeviceToHost, E.st));
    CHK(residual_norm<KP>(E, rd));                                                      // :450
    AMG_HIP(hipMemcpyAsync(cur, rd, sizeof(double) * KP, hipMemcpyDeviceToHost, E.st));
    AMG_HIP(hipStreamSynchronize(E.st));
    const bool fixed = (flags & AMG_SOLVE_NO_EARLY_STOP) != 0;
    bool active[KMAX], snapped = false;
    int nactive = 0;
    for (int j = 0; j < k; ++j) {
        tolj[j] = normb[j] != 0.0 ? tol * normb[j] : tol;
        residuals[(size_t)j * stride] = cur[j];
        nres[j] = 1;
        active[j] = fixed || cur[j] > tolj[j];                                          // :454, per column
        if (active[j]) ++nactive;
    }
    if (nactive && maxiter > 0)
        for (int j = 0; j < k; ++j)
            if (!active[j]) { CHK(snapshot<KP>(E, j)); snapped = true; }
    int it = 1;
    auto run = [&]() -> int {
        while (it <= maxiter && nactive > 0) {
            CHK(one_cycle(MCycle<KP>{E}, E.nlev, cyc));
            CHK(residual_norm<KP>(E, rd + (long)it * KMAX));
            if (!fixed) {
                AMG_HIP(hipMemcpyAsync(cur, rd + (long)it * KMAX, sizeof(double) * KP, hipMemcpyDeviceToHost, E.st));
                AMG_HIP(hipStreamSynchronize(E.st));
                for (int j = 0; j < k; ++j) {
                    if (!active[j]) continue;
                    residuals[(size_t)j * stride + it] = cur[j];
                    nres[j] = it + 1;
                    if (!(cur[j] > tolj[j])) {
                        active[j] = false;
                        --nactive;
                        // the other columns go on: keep this one's iterate (nothing follows when it was the last)
                        if (nactive > 0 && it < maxiter) { CHK(snapshot<KP>(E, j)); snapped = true; }
                    }
                }
            }
            ++it;
        }
        return 0;
    };
    auto store = [&]() -> int {
        if (fixed && it > 1) {
            std::vector<double> all((size_t)it * KMAX);
            AMG_HIP(hipMemcpyAsync(all.data(), rd, sizeof(double) * all.size(), hipMemcpyDeviceToHost, E.st));
            AMG_HIP(hipStreamSynchronize(E.st));
            for (int j = 0; j < k; ++j) {
                for (int q = 1; q < it; ++q) residuals[(size_t)j * stride + q] = all[(size_t)q * KMAX + j];
                nres[j] = it;
            }
        }
        if (!snapped) return store_columns<KP>(E, L0.x.d(), k, X);
        // columns that ran to the end (or stopped in the last cycle run) hold their result in x
        for (int j = 0; j < k; ++j)
            if (nres[j] == it) CHK(snapshot<KP>(E, j));
        return store_columns<KP>(E, E.xs.d(), k, X);
    };
    return E.timed(run, store);
}

template <int KP>
int cycle_kp(Engine &E, int k, const double *B, double *X, int cyc, int flags)
{
    CHK(load_vectors<KP>(E, k, B, X, flags));
    return E.timed([&] { return one_cycle(MCycle<KP>{E}, E.nlev, cyc); },
                   [&] { return store_columns<KP>(E, E.lv[0].x.d(), k, X); });
}

int check_call(Engine &E, int k, const void *B, const void *X, int cyc)
{
    if (!E.finalized) { set_error("hierarchy not finalised"); return AMG_ESTATE; }
    if (k < 1 || k > E.kmax) { set_error("k must be in 1 .. kmax of amg_hierm_create"); return AMG_EINVAL; }
    if (cyc == AMG_CYCLE_AMLI) { set_error("AMLI cycles are not implemented for several right-hand sides"); return AMG_ENOTIMPL; }
    if (!B || !X || cyc < 0 || cyc > 2) { set_error("bad arguments"); return AMG_EINVAL; }
    return 0;
}

// ----------------------------------------------------------------------------------------------- setup
int build_smoother(Engine &E, MLevel &L, MSmoother &s)
{
    if (s.kind == AMG_SM_GAUSS_SEIDEL || s.kind == AMG_SM_SOR) {
        const MMat &A = L.A;
        if (s.sweep != AMG_SWEEP_BACKWARD) CHK(s.fwd.build(E.pool, A.nrows, A.hAp, A.hAj, false));
        if (s.sweep != AMG_SWEEP_FORWARD) CHK(s.bwd.build(E.pool, A.nrows, A.hAp, A.hAj, true));
    }
    return 0;
}

int set_smoother(Engine &E, int lvl, int which, const amg_smoother_desc *d)
{
    MSmoother *slot = nullptr;
    CHK(smoother_slot(E, lvl, which, d, AMG_SM_POLYNOMIAL, "for several right-hand sides", slot));
    MSmoother &s = *slot;
    if (d->kind != AMG_SM_NONE) {
        CHK(check_sweeps(d));
        if (d->kind == AMG_SM_POLYNOMIAL && (d->ncoef < 1 || !d->coef)) { set_error("polynomial: no coefficients"); return AMG_EINVAL; }
    }
    s.set = true;
    s.kind = d->kind;
    if (s.kind == AMG_SM_NONE) return 0;
    s.iterations = d->iterations;
    s.sweep = d->sweep;
    s.omega = d->omega;
    if (s.kind == AMG_SM_POLYNOMIAL) s.coef.assign(d->coef, d->coef + d->ncoef);
    return 0;
}

// what finalize (resident.hpp) leaves to this engine
struct MSetup {
    Engine &E;
    int square(const MMat &A)
    {
        if (A.nrows != A.ncols) { set_error("A must be square"); return AMG_EINVAL; }
        return 0;
    }
    int build_smoother(MLevel &L, MSmoother &s) { return ::build_smoother(E, L, s); }
    // work vectors by what the level's smoothers use: the polynomial ping-pong, the copy jacobi and sor keep
    int level_vectors(int l)
    {
        MLevel &L = E.lv[l];
        const size_t vb = sizeof(double) * (size_t)L.A.nrows * E.kpmax;
        bool poly = false, copy = false;
        auto uses = [&](const MSmoother &s) {
            poly = poly || s.kind == AMG_SM_POLYNOMIAL;
            copy = copy || s.kind == AMG_SM_JACOBI || s.kind == AMG_SM_SOR;
        };
        uses(L.sm[0]);
        uses(L.sm[1]);
        if (l == E.nlev - 1) uses(E.csm);
        for (DBuf *v : {&L.x, &L.b, &L.r}) CHK(E.pool.alloc(*v, vb));
        if (poly) for (DBuf *v : {&L.h1, &L.h2}) CHK(E.pool.alloc(*v, vb));
        if (copy) CHK(E.pool.alloc(L.t, vb));
        return 0;
    }
    int finish()
    {
        CHK(E.pool.alloc(E.xs, sizeof(double) * (size_t)E.lv[0].A.nrows * E.kpmax));
        return E.pool.alloc(E.part, sizeof(double) * NORM_BLOCKS * KMAX);
    }
};

}  // namespace

struct amg_hierm {
    Engine e;
};

#define BY_WIDTH(kp, fn, ...)                 \
    switch (kp) {                             \
    case 1: return fn<1>(__VA_ARGS__);        \
    case 2: return fn<2>(__VA_ARGS__);        \
    case 4: return fn<4>(__VA_ARGS__);        \
    default: return fn<8>(__VA_ARGS__);       \
    }

extern "C" {

int amg_hierm_create(int nlevels, int device, int kmax, amg_hierm **out)
{
    if (!out) { set_error("null out"); return AMG_EINVAL; }
    *out = nullptr;
    if (nlevels < 1) { set_error("nlevels < 1"); return AMG_EINVAL; }
    if (kmax < 1 || kmax > KMAX) { set_error("kmax must be in 1 .. 8 (more columns run in groups)"); return AMG_EINVAL; }
    CHK(open_handle(nlevels, device, out));
    (*out)->e.kmax = kmax;
    (*out)->e.kpmax = width_of(kmax);
    return 0;
}

void amg_hierm_destroy(amg_hierm *h) { close_handle(h); }

int amg_hierm_set_matrix(amg_hierm *h, int lvl, int which, int fmt, int nrows, int ncols, int R, int C,
                         const int *Ap, const int *Aj, const double *Ax)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    Engine &E = h->e;
    MMat *M = operator_slot(E, lvl, which);
    if (!M) return AMG_EINVAL;
    if (fmt != AMG_FMT_CSR && fmt != AMG_FMT_BSR) { set_error("fmt must be 0 (CSR) or 1 (BSR)"); return AMG_EINVAL; }
    if (fmt == AMG_FMT_BSR && (R != 1 || C != 1)) {
        set_error("several right-hand sides: BSR operators with 1 x 1 blocks only");
        return AMG_ENOTIMPL;
    }
    if (M->set) { set_error("operator already set"); return AMG_ESTATE; }
    return M->load(E.pool, fmt, nrows, ncols, Ap, Aj, Ax);
}

int amg_hierm_set_smoother(amg_hierm *h, int lvl, int which, const amg_smoother_desc *d)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    if (which != AMG_PRE && which != AMG_POST) { set_error("which must be AMG_PRE or AMG_POST"); return AMG_EINVAL; }
    return set_smoother(h->e, lvl, which, d);
}

int amg_hierm_set_coarse_dense(amg_hierm *h, const double *M, int n)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    return set_coarse_dense(h->e, M, n, sizeof(double));
}

int amg_hierm_set_coarse_smoother(amg_hierm *h, const amg_smoother_desc *d)
{
    ENTER(h);
    UNSEALED(h, FINALIZE);
    CHK(set_smoother(h->e, h->e.nlev - 1, 2, d));
    h->e.coarse = COARSE_SMOOTHER;
    return 0;
}

int amg_hierm_finalize(amg_hierm *h)
{
    ENTER(h);
    return finalize(h->e, FINALIZE, MSetup{h->e});
}

int amg_hierm_solve(amg_hierm *h, int k, const double *B, double *X, double tol, int maxiter, int cyc,
                    double *residuals, int *nres, int flags)
{
    ENTER(h);
    Engine &E = h->e;
    CHK(check_call(E, k, B, X, cyc));
    if (!residuals || !nres || maxiter < 0) { set_error("bad solve arguments"); return AMG_EINVAL; }
    CHK(E.reserve_history(maxiter, KMAX));
    BY_WIDTH(width_of(k), solve_kp, E, k, B, X, tol, maxiter, cyc, residuals, nres, flags)
}

int amg_hierm_cycle(amg_hierm *h, int k, const double *B, double *X, int cyc, int flags)
{
    ENTER(h);
    Engine &E = h->e;
    CHK(check_call(E, k, B, X, cyc));
    BY_WIDTH(width_of(k), cycle_kp, E, k, B, X, cyc, flags)
}

long amg_hierm_device_bytes(amg_hierm *h) { return h ? h->e.pool.bytes : 0; }

double amg_hierm_last_solve_ms(amg_hierm *h) { return h ? h->e.last_ms : 0.0; }

}  // extern "C"
