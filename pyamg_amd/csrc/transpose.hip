// R = P^T on the device, for the flat entry below and for the chain of classical.hip.
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
#include "graph_dev.hpp"

#include <memory>

using namespace amg;

namespace {

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
thread_local TransposeRoute last_transpose;

}   // namespace

// R = P^T for P (n_row x n_col, nnz entries, columns inside the matrix) in HBM into Rp (n_col + 1 offsets) and freshly
// allocated Rj, Rx.  Without entries or rows: the offsets are zeroed and nothing is launched.
int amg::transpose_device(int n_row, int n_col, long nnz, const int *Pp, const int *Pj, const double *Px, DBuf &Rp, DBuf &Rj, DBuf &Rx,
                          TransposeRoute &how)
{
    how = last_transpose = TransposeRoute{};
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
    how = last_transpose = TransposeRoute{1, n_col - longer[0] - longer[1], longer[0], longer[1]};
    return 0;
}

// the columns and values of a transpose, held for amg_csr_transpose_fetch
struct __attribute__((visibility("hidden"))) amg_transpose {
    long nnz = 0;
    DBuf Rj, Rx;
};

extern "C" {

// ---- R = P^T as a flat entry: host arrays in, the offsets out at once, columns and values through a handle

int amg_csr_transpose_device(int n_row, int n_col, const int *Pp, const int *Pj, const double *Px, int *Rp, amg_transpose **out)
{
    const char *who = "transpose";
    if (!out || !Rp) return bad(who, "bad arguments");
    *out = nullptr;
    if (n_col < 0) return bad(who, "negative size");
    CHK(check_csr_arrays(who, n_row, n_col, Pp, n_row + 1, Pj, 0x7fffffff, Px, 0x7fffffff));
    last_transpose = TransposeRoute{};
    std::unique_ptr<amg_transpose> h(new amg_transpose);
    h->nnz = n_row > 0 ? Pp[n_row] : 0;
    if (h->nnz == 0) {                      // no rows or no entries: the empty result, without a launch
        std::fill(Rp, Rp + (size_t)n_col + 1, 0);
        *out = h.release();
        return 0;
    }
    CHK(require_device());
    HbmCsr P;
    DBuf dRp;
    TransposeRoute how;
    CHK(P.upload(n_row, Pp, Pj, Px));
    CHK(transpose_device(n_row, n_col, h->nnz, P.p.i(), P.j.i(), P.x.d(), dRp, h->Rj, h->Rx, how));
    CHK(dRp.to_host(Rp, sizeof(int) * ((size_t)n_col + 1)));
    *out = h.release();
    return 0;
}

int amg_csr_transpose_fetch(amg_transpose *h, int *Rj, double *Rx)
{
    if (!h) return AMG_EINVAL;
    std::unique_ptr<amg_transpose> own(h);
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

}   // extern "C"
