// Galerkin products of the setup on the device: C = A * B for CSR operands with scipy's csr_matmat arithmetic and
// output order (scipy/sparse/sparsetools/csr.h csr_matmat, called by pyamg/aggregation/aggregation.py:425-426 as
// R * A * P) -- per output row the products are accumulated in the order (entry of A's row, entry of B's row), the
// output columns come out in REVERSE first-touch order, exact-zero results are dropped.
//
// Main kernel (spgemm_group_kernel): G lanes per output row, every row with a table of its own in LDS; left-hand
// entries strictly in order, the lanes over the right-hand row each entry selects.  The routes of matmat(), in order:
//   1. G = 8, 16, 32 or 64 lanes per row from the right-hand operand's mean row length (complex128 one step wider);
//   2. a row outgrew its table and G < 64: the whole product again with the whole wave per row (64 lanes, LDS);
//   3. a row outgrew that too and the longest row has more than 1024 and at most 2^22 products: the whole wave per row
//      with the row's table in HBM, sized so that no row outgrows it;
//   4. no row has more than 1024 products (complex128 only: its wave table takes fewer distinct columns than that, the
//      float64 one takes them all): one thread per row with private tables in HBM (spgemm_rows_kernel, two tiers);
//   5. longer rows than 2^22 products: AMG_EINVAL, the caller's host path -- the per-thread tables would not fit, which
//      the memory guard decides on the host.
// A product without rows is the empty product without a launch.  What a product did is kept per thread for
// amg_spgemm_last_route.  Every path runs a count pass (non-zero results per row) and a fill pass (results written at
// their final places); both do the full arithmetic, neither allocates per row.  Bit-identical to the host restatement
// (setup_host.cpp amgsetup_csr_matmat_*) and to scipy: same products, same order, separate multiply and add.
// Right-hand operands hold each column once per row (amgcore_hip.h); left-hand rows may repeat columns.
#include "hier.hpp"
#include "scalar.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <type_traits>
#include <vector>

using namespace amg;

namespace {

struct Lap {                 // AMG_SETUP_VERBOSE=1: stage times on stderr
    bool on = std::getenv("AMG_SETUP_VERBOSE") && std::getenv("AMG_SETUP_VERBOSE")[0] != '0';
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what)
    {
        if (!on) return;
        hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[setup]     device Galerkin: %-28s %6.2fs\n", what, std::chrono::duration<double>(now - t).count());
        t = now;
    }
};

using sc::c128;

// The value type V of a product is double or c128 (interleaved complex128).  The complex product is scalar.hpp's
// (ar br - ai bi, ar bi + ai br) without contraction, sums add part by part, and a result is dropped only when both of
// its parts are zero (scipy's complex `!= 0`).  The double overloads are the plain operators the float64 kernels
// always used.
template <class V> __device__ __forceinline__ V vzero();
template <> __device__ __forceinline__ double vzero<double>() { return 0.0; }
template <> __device__ __forceinline__ c128 vzero<c128>() { return c128{0.0, 0.0}; }
__device__ __forceinline__ double vmul(double a, double b) { return a * b; }
__device__ __forceinline__ c128 vmul(c128 a, c128 b) { return sc::mul(a, b); }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ c128 vadd(c128 a, c128 b) { return sc::add(a, b); }
__device__ __forceinline__ bool vnz(double a) { return a != 0.0; }
__device__ __forceinline__ bool vnz(c128 a) { return sc::nonzero(a); }

template <class V>
struct DCsrView {          // a CSR operand in HBM that somebody else owns (row pointer as 64-bit offsets)
    int n_row = 0, n_col = 0;
    long nnz = 0;
    const long *Ap = nullptr;
    const int *Aj = nullptr;
    const V *Ax = nullptr;
};
template <class V>
struct DCsrT {             // the same, owning its arrays
    int n_row = 0, n_col = 0;
    long nnz = 0;
    DevArr<long> Ap;
    DevArr<int> Aj;
    DevArr<V> Ax;
    using View = DCsrView<V>;
    operator View() const { return View{n_row, n_col, nnz, Ap, Aj, Ax}; }
};
using DCsr = DCsrT<double>;

// largest number of products of any output row (sizes the tables)
__global__ void spgemm_upper_kernel(int n_row, const long *Ap, const int *Aj, const long *Bp, int *row_upper)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_row) return;
    long u = 0;
    for (long jj = Ap[i]; jj < Ap[i + 1]; ++jj) { const int j = Aj[jj]; u += Bp[j + 1] - Bp[j]; }
    row_upper[i] = (int)min(u, 2147483647L);
}

// FILL = false: count[i] = number of non-zero results of row i (-1: the row has more than `limit` distinct columns and
// is left to a launch with larger tables).  FILL = true: write them at Cp[i] .. in reverse first-touch order (rows
// marked -1 are skipped).  Rows: all (`rows` null) or the listed ones.  Thread t owns table t (cap entries): keys stay
// -1 between rows (cleared through the order list).
// Reached by complex128 products only, and only when no row has more than 1024 products: rows of 961 to 1024 distinct
// columns, which the 2048-entry wave table does not take.  (A float64 row that outgrows its 4096-entry wave table has
// more than 1024 products and goes to the HBM wave tables; past their gate of 2^22 products the memory guard of
// matmat() refuses every product, because the second tier here would hold 256 tables of 2^24 entries at the least.)
// The tables of the second tier are sized by the PRODUCTS of the longest row (2048 entries at most, then); the rows'
// DISTINCT columns are mostly far fewer, so the first launch runs with 256-entry tables (6 KB per thread: Infinity
// Cache / L2) and only rows of more than 128 distinct columns are redone with the large ones.
template <class V, bool FILL>
__global__ __launch_bounds__(256) void spgemm_rows_kernel(int n_work, const int *rows, const long *Ap, const int *Aj, const V *Ax,
                                                         const long *Bp, const int *Bj, const V *Bx, int cap, int limit,
                                                         int *keys, V *sums, int *order, int *count, const long *Cp,
                                                         int *Cj, V *Cx)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nthreads = (long)gridDim.x * blockDim.x;
    int *key = keys + tid * cap;
    V *sum = sums + tid * cap;
    int *ord = order + tid * cap;
    const unsigned mask = (unsigned)cap - 1u;
    for (long w = tid; w < n_work; w += nthreads) {
        const long i = rows ? rows[w] : w;
        if (FILL && !rows && count[i] < 0) continue;                // done by the large-table launch
        int n_ins = 0;
        bool over = false;
        for (long jj = Ap[i]; jj < Ap[i + 1] && !over; ++jj) {
            const int j = Aj[jj];
            const V v = Ax[jj];
            for (long kk = Bp[j]; kk < Bp[j + 1]; ++kk) {
                const int c = Bj[kk];
                unsigned h = ((unsigned)c * 2654435761u) & mask;
                for (;;) {
                    const int k = key[h];
                    if (k == c) break;
                    if (k == -1) {
                        if (n_ins >= limit) { over = true; break; }
                        key[h] = c; sum[h] = vzero<V>(); ord[n_ins++] = (int)h;
                        break;
                    }
                    h = (h + 1u) & mask;
                }
                if (over) break;
                const V p = vmul(v, Bx[kk]);
                sum[h] = vadd(sum[h], p);
            }
        }
        if (over) {
            for (int q = 0; q < n_ins; ++q) key[ord[q]] = -1;
            if (!FILL) count[i] = -1;
            continue;
        }
        if (FILL) {
            long at = Cp[i];
            for (int q = n_ins - 1; q >= 0; --q) {
                const int h = ord[q];
                const V sv = sum[h];
                if (vnz(sv)) { Cj[at] = key[h]; Cx[at] = sv; ++at; }
                key[h] = -1;
            }
        } else {
            int nz = 0;
            for (int q = 0; q < n_ins; ++q) {
                const int h = ord[q];
                nz += vnz(sum[h]) ? 1 : 0;
                key[h] = -1;
            }
            count[i] = nz;
        }
    }
}

// The main kernel: G lanes per output row (64 / G rows per wave), every row with a table of its own in LDS.  The
// entries of the left-hand row are taken strictly one after the other; the G lanes take the entries of the right-hand
// row that entry selects (contiguous in memory: coalesced) -- distinct columns, so no two lanes ever add to the same
// sum in one step and every sum still receives its products in the sequential order.  New columns of a step are
// numbered in lane (= entry) order by a ballot, which is the sequential first-touch order.  G is chosen from the
// right-hand operand's average row length (7-point operator: 8 lanes, eight rows per wave with 512-entry tables;
// long rows: the whole wave on one row with 4096 entries).  A row whose distinct columns do not fit its table raises
// `overflow`: the caller retries with the whole wave per row, then with the row's table in HBM (HBM = true below) or,
// where no row has more than 1024 products, with the one-thread-per-row kernel; see the routes at the head of the file.
// Table entries per wave.  float64: 4096 (16 B per entry, 64 KB of LDS, two waves per compute unit).  complex128: an
// entry costs 24 B, so 2048 (48 KB) keep two waves per compute unit; the host picks lane groups one step wider for
// complex operands, which gives every row the table it has in float64 at all widths below the whole wave.
template <class V> struct wave_cap { static constexpr int value = 4096; };
template <> struct wave_cap<c128> { static constexpr int value = 2048; };
// HBM = true (G = 64 only): the table of the wave's row lives in HBM instead (gcap entries per workgroup, keys preset
// to -1 by the host) -- rows of tens of thousands of products on small coarse levels, where a few hundred waves with
// 2 MB tables each are plenty.
template <class V, bool FILL, int G, bool HBM>
__global__ __launch_bounds__(64) void spgemm_group_kernel(int n_row, const long *Ap, const int *Aj, const V *Ax,
                                                         const long *Bp, const int *Bj, const V *Bx, int *count,
                                                         const long *Cp, int *Cj, V *Cx, int *overflow,
                                                         int *gkey, V *gsum, int *gord, int gcap)
{
    constexpr int WCAP = wave_cap<V>::value;
    static_assert(!HBM || G == 64, "tables in HBM: one row per wave");
    constexpr int NG = 64 / G;             // rows per wave
    constexpr int LB = 64;                 // left-hand entries staged per batch and row
    __shared__ int key_s[HBM ? 1 : WCAP];
    __shared__ V sum_s[HBM ? 1 : WCAP];
    __shared__ int ord_s[HBM ? 1 : WCAP];
    __shared__ V stv_s[NG * LB];
    __shared__ long stb_s[NG * LB];
    __shared__ int stl_s[NG * LB];
    const int lane = threadIdx.x;
    const int g = lane / G, gl = lane % G;                          // group (row slot) and lane within the group
    const int CAP = HBM ? gcap : WCAP / NG;                         // table entries per row
    int *key = HBM ? gkey + (long)blockIdx.x * gcap : key_s + g * CAP;
    V *sum = HBM ? gsum + (long)blockIdx.x * gcap : sum_s + g * CAP;
    int *ord = HBM ? gord + (long)blockIdx.x * gcap : ord_s + g * CAP;
    V *st_v = stv_s + g * LB;
    long *st_b0 = stb_s + g * LB;
    int *st_len = stl_s + g * LB;
    const unsigned mask = (unsigned)CAP - 1u;
    const unsigned long long gmask = (G == 64) ? ~0ULL : (((1ULL << G) - 1ULL) << (g * G));
    const unsigned long long below = (G == 64 ? ((1ULL << lane) - 1ULL) : (((1ULL << gl) - 1ULL) << (g * G)));
    if (!HBM) for (int q = lane; q < WCAP; q += 64) key_s[q] = -1;
    __syncthreads();
    const long stride = (long)gridDim.x * NG;
    const long first = (long)blockIdx.x * NG + g;
    const long rounds = (n_row + stride - 1) / stride;              // the same for every lane: ballots below are wave-wide
    for (long r = 0; r < rounds; ++r) {
        const long i = first + r * stride;
        const bool have = i < n_row;
        int n_ins = 0;
        bool bad = false;
        const long jbeg = have ? Ap[i] : 0, jend = have ? Ap[i + 1] : 0;
        // The left-hand row is staged LB entries at a time: the group's lanes fetch (value, start and length of the
        // right-hand row it selects) for a whole batch at once -- two dependent round trips per batch instead of per
        // entry -- and the first chunks of the next entries' right-hand rows are requested four entries ahead of
        // use.  What remains per entry is LDS work.
        for (long j0 = jbeg;; j0 += LB) {
            if (__ballot(!bad && j0 < jend) == 0ULL) break;
            __syncthreads();
            for (int e = gl; e < LB; e += G) {
                const long jj = j0 + e;
                int len = -1;                                           // -1: past the end of the row
                if (!bad && jj < jend) {
                    const int j = Aj[jj];
                    const long b0 = Bp[j];
                    len = (int)(Bp[j + 1] - b0);
                    st_v[e] = Ax[jj]; st_b0[e] = b0;
                }
                st_len[e] = len;
            }
            __syncthreads();
            // the first chunks of the next PD entries' right-hand rows are requested ahead of use (a ring of PD
            // register slots, the loop unrolled by PD so that the slot index is a constant)
            constexpr int PD = 4;
            int pc[PD]; V px[PD];
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                pc[u] = 0; px[u] = vzero<V>();
                const int l = st_len[u];
                if (gl < l) { const long b = st_b0[u]; pc[u] = Bj[b + gl]; px[u] = Bx[b + gl]; }
            }
            bool batch_done = false;
            for (int e0 = 0; e0 < LB && !batch_done; e0 += PD) {
#pragma unroll
                for (int u = 0; u < PD; ++u) {
                    const int e = e0 + u;
                    const int len = st_len[e];
                    if (__ballot(len >= 0) == 0ULL) { batch_done = true; break; }   // every row of the wave is through its batch
                    const long b0 = len >= 0 ? st_b0[e] : 0;
                    const int c0 = pc[u]; const V x0 = px[u];
                    const V v = len >= 0 ? st_v[e] : vzero<V>();
                    // refill this slot with entry e + PD before touching the table
                    pc[u] = 0; px[u] = vzero<V>();
                    if (e + PD < LB) {
                        const int l = st_len[e + PD];
                        if (gl < l) { const long b = st_b0[e + PD]; pc[u] = Bj[b + gl]; px[u] = Bx[b + gl]; }
                    }
                    // this entry: its right-hand row in chunks of G (the first one is already here)
                    for (int kb = 0;; kb += G) {
                        const bool active = !bad && kb < len;
                        if (__ballot(active) == 0ULL) break;
                        bool inserted = false;
                        int h = 0;
                        if (active) {
                            if (n_ins + G > CAP / 2) bad = true;        // keep the table at most half full
                            else if (kb + gl < len) {
                                int c; V x;
                                if (kb == 0) { c = c0; x = x0; } else { c = Bj[b0 + kb + gl]; x = Bx[b0 + kb + gl]; }
                                h = (int)(((unsigned)c * 2654435761u) & mask);
                                for (;;) {
                                    const int k = atomicCAS(&key[h], -1, c);
                                    if (k == -1) { inserted = true; sum[h] = vzero<V>(); break; }
                                    if (k == c) break;
                                    h = (h + 1) & (int)mask;
                                }
                                const V p = vmul(v, x);
                                sum[h] = vadd(sum[h], p);
                            }
                        }
                        const unsigned long long m = __ballot(inserted);
                        if (inserted) ord[n_ins + __popcll(m & below)] = h;
                        n_ins += __popcll(m & gmask);
                        __syncthreads();                                // (one wave: orders the LDS accesses of the step)
                    }
                }
            }
        }
        if (bad && gl == 0) *overflow = 1;
        if (FILL) {
            long at = have ? Cp[i] : 0;
            int q0 = n_ins - 1;
            for (;;) {                                              // reverse first-touch order, zeros dropped
                if (__ballot(q0 >= 0) == 0ULL) break;
                const int q = q0 - gl;
                V sv = vzero<V>(); int kv = 0;
                if (q >= 0) { const int hh = ord[q]; sv = sum[hh]; kv = key[hh]; }
                const bool keep = (q >= 0) && vnz(sv) && !bad;
                const unsigned long long m = __ballot(keep);
                if (keep) { const long w = at + __popcll(m & below); Cj[w] = kv; Cx[w] = sv; }
                at += __popcll(m & gmask);
                q0 -= G;
            }
        } else {
            int nz = 0, q0 = 0;
            for (;;) {
                if (__ballot(q0 < n_ins) == 0ULL) break;
                const int q = q0 + gl;
                const bool keep = (q < n_ins) && vnz(sum[ord[q]]);
                nz += __popcll(__ballot(keep) & gmask);
                q0 += G;
            }
            if (have && gl == 0) count[i] = nz;
        }
        __syncthreads();
        for (int q = gl; q < n_ins; q += G) key[ord[q]] = -1;
        __syncthreads();
    }
}

template <class V>
int upload_dcsr(DCsrT<V> &M, int n_row, int n_col, const long *Ap, const int *Aj, const V *Ax)
{
    M.n_row = n_row; M.n_col = n_col; M.nnz = Ap[n_row];
    AMG_HIP(M.Ap.malloc_bytes(sizeof(long) * ((size_t)n_row + 1)));
    AMG_HIP(M.Aj.malloc_bytes(sizeof(int) * (size_t)std::max(M.nnz, 1L)));
    AMG_HIP(M.Ax.malloc_bytes(sizeof(V) * (size_t)std::max(M.nnz, 1L)));
    AMG_HIP(hipMemcpy(M.Ap, Ap, sizeof(long) * ((size_t)n_row + 1), hipMemcpyHostToDevice));
    AMG_HIP(hipMemcpy(M.Aj, Aj, sizeof(int) * (size_t)M.nnz, hipMemcpyHostToDevice));
    AMG_HIP(hipMemcpy(M.Ax, Ax, sizeof(V) * (size_t)M.nnz, hipMemcpyHostToDevice));
    return 0;
}

// What matmat() did for the calling thread's most recent product (amg_spgemm_last_route, amgcore_hip.h): the tests pin
// every route below to operands built for it.
enum { ROUTE_NONE = 0, ROUTE_LDS = 1, ROUTE_HBM_WAVE = 2, ROUTE_HBM_THREAD = 3, ROUTE_REFUSED = 4 };
struct Route { int cplx = 0, g_first = 0, g_final = 0, where = ROUTE_NONE, cap = 0, blocks = 0, big_rows = 0; };
thread_local Route last_route;

// threads (= tables) of a per-thread launch that wants `want` of them: whole workgroups of 256, at least one
inline long table_threads(long want) { return (std::max<long>(256, want) + 255) / 256 * 256; }

// C = A * B, both in HBM; C allocated here
template <class V>
int matmat(const typename DCsrT<V>::View &A, const typename DCsrT<V>::View &B, DCsrT<V> &C)
{
    constexpr bool CPLX = !std::is_same<V, double>::value;
    Route &route = last_route;
    route = Route{};
    route.cplx = CPLX ? 1 : 0;
    route.where = ROUTE_REFUSED;                                // until a path below has run to its end
    if (A.n_col != B.n_row) { set_error("spgemm: inner dimensions differ"); return AMG_EINVAL; }
    C.n_row = A.n_row; C.n_col = B.n_col;
    const int n = A.n_row;
    constexpr long ENTRY = 8 + (long)sizeof(V);                 // bytes of a table entry: key, place in the order list, sum
    if (n == 0) {                                               // no rows: the empty product, without a launch
        route.where = ROUTE_NONE;
        C.nnz = 0; C.Aj.reset(); C.Ax.reset();
        AMG_HIP(C.Ap.malloc_bytes(sizeof(long)));
        AMG_HIP(hipMemset(C.Ap, 0, sizeof(long)));
        return 0;
    }
    DevArr<int> upper;
    AMG_HIP(upper.malloc_bytes(sizeof(int) * (size_t)std::max(n, 1)));
    hipLaunchKernelGGL(spgemm_upper_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, A.Ap, A.Aj, B.Ap, upper);
    std::vector<int> hu((size_t)n);
    AMG_HIP(hipMemcpy(hu.data(), upper, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    upper.reset();
    const int max_upper = n ? *std::max_element(hu.begin(), hu.end()) : 0;
    int cap = 64;
    while (cap < 2 * max_upper && cap < (1 << 30)) cap <<= 1;
    // G lanes per row with the tables in LDS; a row whose distinct columns outgrow its table sends the whole product on:
    // to the whole wave per row, then to the paths with tables in HBM below
    const double avgB = B.n_row > 0 ? (double)B.nnz / (double)B.n_row : 1.0;
    const int G0r = avgB <= 10.0 ? 8 : (avgB <= 20.0 ? 16 : (avgB <= 40.0 ? 32 : 64));
    const int G0 = CPLX ? std::min(64, 2 * G0r) : G0r;             // complex: one step wider (wave_cap)
    route.g_first = G0;
    for (int G = G0; G <= 64; G = (G == 64 ? 128 : 64)) {          // the preferred width, then the whole wave per row
        DevArr<int> count, overflow;
        AMG_HIP(count.malloc_bytes(sizeof(int) * (size_t)std::max(n, 1)));
        AMG_HIP(overflow.malloc_bytes(sizeof(int)));
        AMG_HIP(hipMemset(overflow, 0, sizeof(int)));
        const int rows_per_wave = 64 / G;
        const int blocks = (int)std::min<long>(((long)n + rows_per_wave - 1) / rows_per_wave, 256L * 2 * 8);
#define GROUP_LAUNCH(FILL, GG) hipLaunchKernelGGL((spgemm_group_kernel<V, FILL, GG, false>), dim3(blocks), dim3(64), 0, nullptr, n, A.Ap, A.Aj, A.Ax, \
                                                  B.Ap, B.Aj, B.Ax, count, (const long *)C.Ap, C.Aj, C.Ax, overflow, (int *)nullptr, \
                                                  (V *)nullptr, (int *)nullptr, 0)
#define GROUP_DISPATCH(FILL) do { if (G == 8) { if constexpr (!CPLX) GROUP_LAUNCH(FILL, 8); } else if (G == 16) GROUP_LAUNCH(FILL, 16); \
                                  else if (G == 32) GROUP_LAUNCH(FILL, 32); else GROUP_LAUNCH(FILL, 64); } while (0)
        C.Ap.reset(); C.Aj.reset(); C.Ax.reset();
        GROUP_DISPATCH(false);
        LAUNCH_CHECK("spgemm group count launch");
        int ovf = 0;
        AMG_HIP(hipMemcpy(&ovf, overflow, sizeof(int), hipMemcpyDeviceToHost));
        if (std::getenv("AMG_SETUP_VERBOSE") && std::getenv("AMG_SETUP_VERBOSE")[0] != '0')
            std::fprintf(stderr, "[setup]     device product %d x %d%s: %d lanes per row (right-hand rows avg %.1f, longest row %d products)%s\n",
                         A.n_row, B.n_col, CPLX ? " (complex128)" : "", G, avgB, max_upper, ovf ? " -- a row outgrew its LDS table" : "");
        if (!ovf) {
            std::vector<int> hc((size_t)n);
            AMG_HIP(hipMemcpy(hc.data(), count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
            std::vector<long> cp((size_t)n + 1);
            cp[0] = 0;
            for (int i = 0; i < n; ++i) cp[(size_t)i + 1] = cp[(size_t)i] + hc[(size_t)i];
            C.nnz = cp[(size_t)n];
            AMG_HIP(C.Ap.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
            AMG_HIP(C.Aj.malloc_bytes(sizeof(int) * (size_t)std::max(C.nnz, 1L)));
            AMG_HIP(C.Ax.malloc_bytes(sizeof(V) * (size_t)std::max(C.nnz, 1L)));
            AMG_HIP(hipMemcpy(C.Ap, cp.data(), sizeof(long) * ((size_t)n + 1), hipMemcpyHostToDevice));
            GROUP_DISPATCH(true);
            LAUNCH_CHECK("spgemm group fill launch");
            AMG_HIP(hipDeviceSynchronize());
            route.g_final = G; route.where = ROUTE_LDS; route.cap = wave_cap<V>::value / rows_per_wave; route.blocks = blocks;
            return 0;
        }
#undef GROUP_DISPATCH
#undef GROUP_LAUNCH
    }
    // whole wave per row with the row's table in HBM: long rows on a small level (a few thousand rows of tens of
    // thousands of products -- the coarse Galerkin products)
    if (max_upper > 1024 && max_upper <= (1 << 22)) {
        long distinct_bound = std::min<long>(max_upper, (long)B.n_col);
        int gcap = 1024;
        while (gcap < 2 * distinct_bound + 256) gcap <<= 1;
        const int blocks = (int)std::max<long>(1, std::min<long>(std::min<long>(n, 1024), (4L << 30) / ((long)gcap * ENTRY)));
        DevArr<int> count, overflow, gkey, gord;
        DevArr<V> gsum;
        AMG_HIP(count.malloc_bytes(sizeof(int) * (size_t)std::max(n, 1)));
        AMG_HIP(overflow.malloc_bytes(sizeof(int)));
        AMG_HIP(hipMemset(overflow, 0, sizeof(int)));
        AMG_HIP(gkey.malloc_bytes(sizeof(int) * (size_t)blocks * gcap));
        AMG_HIP(gord.malloc_bytes(sizeof(int) * (size_t)blocks * gcap));
        AMG_HIP(gsum.malloc_bytes(sizeof(V) * (size_t)blocks * gcap));
        AMG_HIP(hipMemset(gkey, 0xFF, sizeof(int) * (size_t)blocks * gcap));
        C.Ap.reset(); C.Aj.reset(); C.Ax.reset();
        hipLaunchKernelGGL((spgemm_group_kernel<V, false, 64, true>), dim3(blocks), dim3(64), 0, nullptr, n, A.Ap, A.Aj, A.Ax, B.Ap, B.Aj, B.Ax,
                           count, (const long *)nullptr, (int *)nullptr, (V *)nullptr, overflow, gkey, gsum, gord, gcap);
        LAUNCH_CHECK("spgemm HBM-table count launch");
        int ovf = 0;
        AMG_HIP(hipMemcpy(&ovf, overflow, sizeof(int), hipMemcpyDeviceToHost));
        if (std::getenv("AMG_SETUP_VERBOSE") && std::getenv("AMG_SETUP_VERBOSE")[0] != '0')
            std::fprintf(stderr, "[setup]     device product %d x %d: one wave per row, %d-entry tables in HBM%s\n", A.n_row, B.n_col, gcap,
                         ovf ? " -- overflow" : "");
        int rc = 0;
        if (!ovf) {
            std::vector<int> hc((size_t)n);
            AMG_HIP(hipMemcpy(hc.data(), count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
            std::vector<long> cp((size_t)n + 1);
            cp[0] = 0;
            for (int i = 0; i < n; ++i) cp[(size_t)i + 1] = cp[(size_t)i] + hc[(size_t)i];
            C.nnz = cp[(size_t)n];
            AMG_HIP(C.Ap.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
            AMG_HIP(C.Aj.malloc_bytes(sizeof(int) * (size_t)std::max(C.nnz, 1L)));
            AMG_HIP(C.Ax.malloc_bytes(sizeof(V) * (size_t)std::max(C.nnz, 1L)));
            AMG_HIP(hipMemcpy(C.Ap, cp.data(), sizeof(long) * ((size_t)n + 1), hipMemcpyHostToDevice));
            hipLaunchKernelGGL((spgemm_group_kernel<V, true, 64, true>), dim3(blocks), dim3(64), 0, nullptr, n, A.Ap, A.Aj, A.Ax, B.Ap, B.Aj, B.Ax,
                               count, (const long *)C.Ap, C.Aj, C.Ax, overflow, gkey, gsum, gord, gcap);
            rc = launched("spgemm HBM-table fill launch");
            if (hipDeviceSynchronize() != hipSuccess && rc == 0) rc = AMG_ENODEV;
            if (rc == 0) { route.g_final = 64; route.where = ROUTE_HBM_WAVE; route.cap = gcap; route.blocks = blocks; }
        }
        if (!ovf) return rc;
    }
    // One thread per row.  The guard counts what Tables::make below would allocate if every row went on to the second
    // tier -- whole workgroups of 256 tables in either tier, however few rows there are -- against the 4 GB the HBM wave
    // tables may take.  Rows of at most 1024 products always pass (at most 65536 tables of 256 and of 2048 entries,
    // 3.6 GB).  Longer rows arrive here only past the gate of the HBM wave tables, 2^22 products: the second tier would
    // then hold 256 tables of 2^24 entries or more (69 GB in float64), so every such product goes back to the caller's
    // host path, decided here and not by a failed allocation.
    const int small_cap = std::min(cap, 256);
    const long t2_threads = std::min<long>(256L * 512L, (3L << 30) / ((long)cap * ENTRY));
    const double table_bytes = ((double)table_threads(std::min<long>(65536, n)) * (double)small_cap +
                                (double)table_threads(std::min<long>(t2_threads, n)) * (double)cap) * (double)ENTRY;
    if (table_bytes > (double)(4L << 30)) {
        route.cap = cap;
        set_error("spgemm: rows with more distinct columns than the LDS tables hold on a level too large for per-thread tables (host path)");
        return AMG_EINVAL;
    }
    // first tier: 256-entry tables (up to 128 distinct columns per row), 65536 threads
    struct Tables {
        DevArr<int> keys, order; DevArr<V> sums; int cap = 0; long threads = 0; int blocks = 0;
        int make(int cap_, long want_threads)
        {
            cap = cap_;
            threads = table_threads(want_threads);
            blocks = (int)(threads / 256);
            AMG_HIP(keys.malloc_bytes(sizeof(int) * (size_t)(threads * cap)));
            AMG_HIP(order.malloc_bytes(sizeof(int) * (size_t)(threads * cap)));
            AMG_HIP(sums.malloc_bytes(sizeof(V) * (size_t)(threads * cap)));
            AMG_HIP(hipMemset(keys, 0xFF, sizeof(int) * (size_t)(threads * cap)));
            return 0;
        }
    };
    if (std::getenv("AMG_SETUP_VERBOSE") && std::getenv("AMG_SETUP_VERBOSE")[0] != '0')
        std::fprintf(stderr, "[setup]     device product %d x %d%s: one thread per row, %d-entry tables in HBM (%d-entry ones for rows that outgrow them)\n",
                     A.n_row, B.n_col, CPLX ? " (complex128)" : "", small_cap, cap);
    Tables T1, T2;
    CHK(T1.make(small_cap, std::min<long>(65536, n)));
    DevArr<int> count, big_rows;
    AMG_HIP(count.malloc_bytes(sizeof(int) * (size_t)std::max(n, 1)));
    hipLaunchKernelGGL((spgemm_rows_kernel<V, false>), dim3(T1.blocks), dim3(256), 0, nullptr, n, (const int *)nullptr, A.Ap, A.Aj, A.Ax,
                       B.Ap, B.Aj, B.Ax, T1.cap, T1.cap / 2, T1.keys, T1.sums, T1.order, count, (const long *)nullptr,
                       (int *)nullptr, (V *)nullptr);
    LAUNCH_CHECK("spgemm count launch");
    std::vector<int> hc((size_t)n);
    AMG_HIP(hipMemcpy(hc.data(), count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    std::vector<int> big;
    for (int i = 0; i < n; ++i) if (hc[(size_t)i] < 0) big.push_back(i);
    if (!big.empty()) {
        // second tier: the rows that outgrew the small tables, with tables sized by the longest row's products
        CHK(T2.make(cap, std::min<long>(t2_threads, (long)big.size())));
        AMG_HIP(big_rows.malloc_bytes(sizeof(int) * big.size()));
        AMG_HIP(hipMemcpy(big_rows, big.data(), sizeof(int) * big.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((spgemm_rows_kernel<V, false>), dim3(T2.blocks), dim3(256), 0, nullptr, (int)big.size(), big_rows, A.Ap, A.Aj, A.Ax,
                           B.Ap, B.Aj, B.Ax, T2.cap, T2.cap / 2, T2.keys, T2.sums, T2.order, count, (const long *)nullptr,
                           (int *)nullptr, (V *)nullptr);
        LAUNCH_CHECK("spgemm count launch (large tables)");
        AMG_HIP(hipMemcpy(hc.data(), count, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        for (int i : big) if (hc[(size_t)i] < 0) { set_error("spgemm: row overflowed the large table"); return AMG_ESTATE; }
    }
    std::vector<long> cp((size_t)n + 1);
    cp[0] = 0;
    for (int i = 0; i < n; ++i) cp[(size_t)i + 1] = cp[(size_t)i] + hc[(size_t)i];
    C.nnz = cp[(size_t)n];
    AMG_HIP(C.Ap.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
    AMG_HIP(C.Aj.malloc_bytes(sizeof(int) * (size_t)std::max(C.nnz, 1L)));
    AMG_HIP(C.Ax.malloc_bytes(sizeof(V) * (size_t)std::max(C.nnz, 1L)));
    AMG_HIP(hipMemcpy(C.Ap, cp.data(), sizeof(long) * ((size_t)n + 1), hipMemcpyHostToDevice));
    if (!big.empty()) {
        // mark the large rows in `count` again (the first-tier fill skips rows with count < 0)
        std::vector<int> mark(hc);
        for (int i : big) mark[(size_t)i] = -1;
        AMG_HIP(hipMemcpy(count, mark.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL((spgemm_rows_kernel<V, true>), dim3(T1.blocks), dim3(256), 0, nullptr, n, (const int *)nullptr, A.Ap, A.Aj, A.Ax,
                       B.Ap, B.Aj, B.Ax, T1.cap, T1.cap / 2, T1.keys, T1.sums, T1.order, count, C.Ap, C.Aj, C.Ax);
    LAUNCH_CHECK("spgemm fill launch");
    if (!big.empty()) {
        hipLaunchKernelGGL((spgemm_rows_kernel<V, true>), dim3(T2.blocks), dim3(256), 0, nullptr, (int)big.size(), big_rows, A.Ap, A.Aj, A.Ax,
                           B.Ap, B.Aj, B.Ax, T2.cap, T2.cap / 2, T2.keys, T2.sums, T2.order, count, C.Ap, C.Aj, C.Ax);
        LAUNCH_CHECK("spgemm fill launch (large tables)");
    }
    AMG_HIP(hipDeviceSynchronize());
    route.g_final = 1; route.where = ROUTE_HBM_THREAD; route.cap = T1.cap; route.blocks = T1.blocks; route.big_rows = (int)big.size();
    return 0;
}

__global__ void widen_rowptr_kernel(int n, const int *Ap32, long *Ap64)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) Ap64[i] = Ap32[i];
}

__global__ void narrow_rowptr_kernel(int n, const long *Ap64, int *Ap32)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) Ap32[i] = (int)Ap64[i];
}

}   // namespace

namespace amg {
// C = A * A for a square operand already in HBM (the squarings of the evolution strength measure, strength.hip); the
// arrays of C are allocated here and move into the caller's owners
int spgemm_square_device(int n, long nnz, const long *Ap, const int *Aj, const double *Ax, long *Cnnz, DevArr<long> &Cp, DevArr<int> &Cj,
                         DevArr<double> &Cx)
{
    const DCsr::View A{n, n, nnz, Ap, Aj, Ax};
    DCsr C;
    CHK(matmat(A, A, C));
    *Cnnz = C.nnz; Cp = std::move(C.Ap); Cj = std::move(C.Aj); Cx = std::move(C.Ax);
    return 0;
}

// C = A * B for operands already in HBM (the Galerkin products of the classical chain, classical.hip): A is n_row x n_inner,
// B n_inner x n_col, both with 64-bit row pointers.  Same ownership rule as above.  AMG_EINVAL, with nothing moved, where
// matmat() refuses the product or C would hold 2^31 entries or more (C's columns and the callers' offsets are ints).
int spgemm_device(int n_row, int n_inner, int n_col, long a_nnz, const long *Ap, const int *Aj, const double *Ax, long b_nnz,
                  const long *Bp, const int *Bj, const double *Bx, long *Cnnz, DevArr<long> &Cp, DevArr<int> &Cj, DevArr<double> &Cx)
{
    const DCsr::View A{n_row, n_inner, a_nnz, Ap, Aj, Ax}, B{n_inner, n_col, b_nnz, Bp, Bj, Bx};
    DCsr C;
    CHK(matmat(A, B, C));
    if (C.nnz >= (1L << 31)) { set_error("spgemm: the product holds 2^31 entries or more"); return AMG_EINVAL; }
    *Cnnz = C.nnz; Cp = std::move(C.Ap); Cj = std::move(C.Aj); Cx = std::move(C.Ax);
    return 0;
}

// the n + 1 offsets of a 32-bit row pointer as 64-bit ones (allocated here) and back; both arrays in HBM
int widen_rowptr_device(int n, const int *p32, DevArr<long> &p64)
{
    AMG_HIP(p64.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
    hipLaunchKernelGGL(widen_rowptr_kernel, dim3((n + 256) / 256), dim3(256), 0, nullptr, n, p32, (long *)p64);
    LAUNCH_RETURN("spgemm: row pointer widening launch");
}

// nnz: the last offset, which the caller knows; 2^31 or more does not fit and is AMG_EINVAL
int narrow_rowptr_device(int n, long nnz, const long *p64, int *p32)
{
    if (nnz < 0 || nnz >= (1L << 31)) { set_error("spgemm: offsets of 2^31 or more do not fit 32-bit row pointers"); return AMG_EINVAL; }
    hipLaunchKernelGGL(narrow_rowptr_kernel, dim3((n + 256) / 256), dim3(256), 0, nullptr, n, p64, p32);
    LAUNCH_RETURN("spgemm: row pointer narrowing launch");
}
}   // namespace amg

struct __attribute__((visibility("hidden"))) amg_galerkin {
    DCsr C;
    DCsrT<c128> Cz;             // the product of the complex128 entries (is_c128)
    bool is_c128 = false;
    std::vector<long> cp;
};

extern "C" {

// Ac = (R * A) * P with A taken from level `level` of a hierarchy handle that already holds it in HBM (the handle of
// the setup-time spectral-radius estimate), R and P handed in as host CSR arrays (64-bit row pointers).  On return
// Cp (n_coarse + 1 entries) is filled and *out holds the product; amg_galerkin_fetch copies its columns and values
// (Cp[n_coarse] entries each) to the host and releases it.  AMG_EINVAL when the operator is not held as plain CSR or a
// row is too long for the device tables: the caller then uses its host path.
int amg_hier_galerkin(amg_hier *h, int level, int n_coarse, const int64_t *Rp, const int *Rj, const double *Rx,
                      const int64_t *Pp, const int *Pj, const double *Px, int64_t *Cp, amg_galerkin **out)
{
    if (!h || !out || level < 0 || level >= (int)h->lv.size()) { set_error("galerkin: bad arguments"); return AMG_EINVAL; }
    const DevCsr &M = h->lv[(size_t)level].A;
    if (!M.Ap || !M.Aj || !M.Ax) { set_error("galerkin: the operator is not held as CSR"); return AMG_EINVAL; }
    AMG_HIP(hipSetDevice(h->device));
    const int n = M.nrows;
    Lap lap;
    DCsr R, P, RA;
    DevArr<long> Ap64;                     // the level's operator as a borrowed operand: its row pointer widened
    AMG_HIP(Ap64.malloc_bytes(sizeof(long) * ((size_t)n + 1)));
    hipLaunchKernelGGL(widen_rowptr_kernel, dim3((n + 256) / 256), dim3(256), 0, nullptr, n, M.Ap, Ap64);
    const DCsr::View A{n, M.ncols, M.nnz, Ap64, M.Aj, M.Ax};
    int rc = upload_dcsr(R, n_coarse, n, (const long *)Rp, Rj, Rx);
    lap("R to HBM");
    if (rc == 0) rc = matmat(R, A, RA);
    lap("R*A");
    R = {};
    Ap64.reset();
    if (rc != 0) return rc;
    rc = upload_dcsr(P, n, n_coarse, (const long *)Pp, Pj, Px);
    lap("P to HBM");
    std::unique_ptr<amg_galerkin> g(new amg_galerkin);
    if (rc == 0) rc = matmat(RA, P, g->C);
    lap("(R*A)*P");
    P = {};
    RA = {};
    CHK(rc);
    if (hipMemcpy(Cp, g->C.Ap, sizeof(long) * ((size_t)n_coarse + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("galerkin: row pointer download failed");
        return AMG_ENODEV;
    }
    *out = g.release();
    return 0;
}

int amg_galerkin_fetch(amg_galerkin *g, int *Cj, double *Cx)
{
    if (!g) return AMG_EINVAL;
    if (g->is_c128) { set_error("galerkin: a complex128 product is fetched with amg_galerkin_fetch_c128"); return AMG_EINVAL; }
    std::unique_ptr<amg_galerkin> own(g);
    if (g->C.nnz > 0) {
        if (!Cj || !Cx) { set_error("galerkin fetch: null array"); return AMG_EINVAL; }
        if (hipMemcpy(Cj, g->C.Aj, sizeof(int) * (size_t)g->C.nnz, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(Cx, g->C.Ax, sizeof(double) * (size_t)g->C.nnz, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("galerkin: download failed");
            return AMG_ENODEV;
        }
    }
    return 0;
}

// C = A * B for host CSR operands through the device kernels (tests; same arithmetic as amg_hier_galerkin's products)
int amg_csr_matmat_device(int n_row, int n_inner, int n_col, const int64_t *Ap, const int *Aj, const double *Ax,
                          const int64_t *Bp, const int *Bj, const double *Bx, int64_t *Cp, amg_galerkin **out)
{
    if (!out) return AMG_EINVAL;
    DCsr A, B;
    CHK(upload_dcsr(A, n_row, n_inner, (const long *)Ap, Aj, Ax));
    CHK(upload_dcsr(B, n_inner, n_col, (const long *)Bp, Bj, Bx));
    std::unique_ptr<amg_galerkin> g(new amg_galerkin);
    CHK(matmat(A, B, g->C));
    A = {}; B = {};
    if (hipMemcpy(Cp, g->C.Ap, sizeof(long) * ((size_t)n_row + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("matmat: row pointer download failed");
        return AMG_ENODEV;
    }
    *out = g.release();
    return 0;
}

// ---- complex128 operands (values as interleaved (re, im) pairs of doubles); the products run through the same
// kernels instantiated for c128: every output entry accumulates (ar br - ai bi, ar bi + ai br) from zero in traversal
// order, part by part, comes out in reverse first-touch order and is dropped only when both parts are zero.

// C = A * B for host CSR operands: the complex twin of amg_csr_matmat_device
int amg_csr_matmat_device_c128(int n_row, int n_inner, int n_col, const int64_t *Ap, const int *Aj, const void *Ax,
                               const int64_t *Bp, const int *Bj, const void *Bx, int64_t *Cp, amg_galerkin **out)
{
    if (!out || !Ap || !Bp || !Cp || n_row < 0 || n_inner < 0 || n_col < 0) { set_error("matmat: bad arguments"); return AMG_EINVAL; }
    DCsrT<c128> A, B;
    CHK(upload_dcsr(A, n_row, n_inner, (const long *)Ap, Aj, (const c128 *)Ax));
    CHK(upload_dcsr(B, n_inner, n_col, (const long *)Bp, Bj, (const c128 *)Bx));
    std::unique_ptr<amg_galerkin> g(new amg_galerkin);
    g->is_c128 = true;
    CHK(matmat(A, B, g->Cz));
    A = {}; B = {};
    if (hipMemcpy(Cp, g->Cz.Ap, sizeof(long) * ((size_t)n_row + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("matmat: row pointer download failed");
        return AMG_ENODEV;
    }
    *out = g.release();
    return 0;
}

// Ac = (R * A) * P from three host CSR operands (64-bit row pointers): R is n_coarse x n_fine, A n_fine x n_fine,
// P n_fine x n_coarse.  R * A is formed in HBM and stays there.  On return Cp (n_coarse + 1 entries) is filled and
// *out holds the product for amg_galerkin_fetch_c128.  AMG_EINVAL when a row is too long for the device tables: the
// caller then uses its host path.
int amg_galerkin_device_c128(int n_fine, int n_coarse, const int64_t *Rp, const int *Rj, const void *Rx,
                             const int64_t *Ap, const int *Aj, const void *Ax,
                             const int64_t *Pp, const int *Pj, const void *Px, int64_t *Cp, amg_galerkin **out)
{
    if (!out || !Rp || !Ap || !Pp || !Cp || n_fine < 0 || n_coarse < 0) { set_error("galerkin: bad arguments"); return AMG_EINVAL; }
    Lap lap;
    DCsrT<c128> A, R, P, RA;
    int rc = upload_dcsr(R, n_coarse, n_fine, (const long *)Rp, Rj, (const c128 *)Rx);
    if (rc == 0) rc = upload_dcsr(A, n_fine, n_fine, (const long *)Ap, Aj, (const c128 *)Ax);
    lap("R, A to HBM");
    if (rc == 0) rc = matmat(R, A, RA);
    lap("R*A");
    R = {}; A = {};
    if (rc != 0) return rc;
    rc = upload_dcsr(P, n_fine, n_coarse, (const long *)Pp, Pj, (const c128 *)Px);
    lap("P to HBM");
    std::unique_ptr<amg_galerkin> g(new amg_galerkin);
    g->is_c128 = true;
    if (rc == 0) rc = matmat(RA, P, g->Cz);
    lap("(R*A)*P");
    P = {}; RA = {};
    CHK(rc);
    if (hipMemcpy(Cp, g->Cz.Ap, sizeof(long) * ((size_t)n_coarse + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("galerkin: row pointer download failed");
        return AMG_ENODEV;
    }
    *out = g.release();
    return 0;
}

int amg_spgemm_last_route(int *out, int n)
{
    const int f[AMG_SPGEMM_ROUTE_FIELDS] = {last_route.cplx, last_route.g_first, last_route.g_final, last_route.where,
                                            last_route.cap, last_route.blocks, last_route.big_rows};
    for (int q = 0; out && q < n && q < AMG_SPGEMM_ROUTE_FIELDS; ++q) out[q] = f[q];
    return AMG_SPGEMM_ROUTE_FIELDS;
}

// columns and interleaved values (Cp[n] entries each) of a complex128 product to the host; releases it
int amg_galerkin_fetch_c128(amg_galerkin *g, int *Cj, void *Cx)
{
    if (!g) return AMG_EINVAL;
    if (!g->is_c128) { set_error("galerkin: a float64 product is fetched with amg_galerkin_fetch"); return AMG_EINVAL; }
    std::unique_ptr<amg_galerkin> own(g);
    if (g->Cz.nnz > 0) {
        if (!Cj || !Cx) { set_error("galerkin fetch: null array"); return AMG_EINVAL; }
        if (hipMemcpy(Cj, g->Cz.Aj, sizeof(int) * (size_t)g->Cz.nnz, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(Cx, g->Cz.Ax, sizeof(c128) * (size_t)g->Cz.nnz, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("galerkin: download failed");
            return AMG_ENODEV;
        }
    }
    return 0;
}

}   // extern "C"
