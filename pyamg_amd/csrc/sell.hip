// Sliced form of irregular operators (DevCsr::sl_*, SELL-64-sigma) and its application kernel.
//
// csr_stream_kernel serves every operator without grid structure (the Galerkin operators A_1, A_2, ..., restriction,
// prolongation).  A workgroup of it makes three DEPENDENT round trips -- row pointer, entries, gathered operands --
// with barriers in between, and rocprofv3 shows ~80 % of its wave cycles waiting: it is bound
// by that chain, not by bytes.  Here a wave owns a slice of 64 rows, a lane one row; the slice's entries are stored
// entry-major (entry k of the 64 rows side by side, padded to the slice's longest row), so a lane's loads are
// coalesced with its neighbours', need no row pointer and no LDS, and a row's entries are requested before any is
// consumed, no barrier.  Rows are sorted by length inside windows
// of 256 (restrictions: 64) rows (longest first, ties in row order) so that slices are nearly rectangular.
// Every lane adds ITS row's products in stored order with separate multiply and add: bit-identical to the CSR kernel
// (scipy csr_matvec / relaxation.h row loops) in every mode.
//
// The dependent round trips of a slice: (1) its header record (SellHdr: entry and code-word offsets, width, coded
// flag, window origins -- one address that depends on the slice number alone, scalar loads) together with the lane's
// slot (row and length, one 8-byte load); (2) the entries, up to SL_PASS per row at once, with the epilogue's streamed
// operands (b[row], v2[row]); (3) the gathered operands; (2) and (3) again for rows of more than SL_PASS entries;
// (4) the store.
#include "hier.hpp"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace amg {

namespace {

constexpr int SL_C = 64;            // rows per slice = lanes per wave
constexpr int SL_SIGMA_SQUARE = 256;   // rows per sorting window: square operators (A_l)
constexpr int SL_SIGMA_RECT = 64;      //                          restrictions (the gathers reach into the finer level: keep neighbours together)
constexpr int SL_PASS = 32;         // entries of a row requested at once (16: measured slower)
constexpr int SL_WG = 256;          // four slices per workgroup (one slice per workgroup: measured equal)
static_assert(SL_PASS % 2 == 0, "code words hold two entries");

__device__ __forceinline__ int remap(int b, int nb, int chunk)       // kernels.hip remap_block: consecutive blocks to one XCD
{
    if (chunk <= 0) return b;
    const int gsz = 8 * chunk, g = b / gsz, base = g * gsz;
    const int n_g = min(gsz, nb - base), l = b - base;
    const int xcd = l & 7, j = l >> 3, q = n_g >> 3, r = n_g & 7;
    return base + xcd * q + min(xcd, r) + j;
}

// window sort: key = ((length + 1) << 11) | (window size - 1 - position in window), sorted DESCENDING = longest row
// first, ties in row order.  Bitonic network over the keys of a window in LDS.
// Window size (tools/sell_ab.py with differently compiled libraries, 300^3 / 400^3 / 500^3): the wider the window, the
// less padding but the further apart the rows that end up side by side in a slice -- their gathers then share fewer
// cache lines.  2048: A_1 -11 % at 500^3 but +2 % / +10 % at 400^3 / 300^3 against the CSR kernel and R_0 up to +46 %;
// 256: A_1 -9 .. -12 % at all three sizes; restrictions (which gather from the finer level) want 64.
template <int SL_SIGMA>
__global__ __launch_bounds__(1024) void sell_sort_kernel(int row_lo, int n, const int *Ap, SellSlot *sl_slot, int *slice_w)
{          // rows row_lo .. row_lo + n - 1
    __shared__ unsigned key[SL_SIGMA];
    static_assert(SL_SIGMA <= 2048 && (SL_SIGMA & (SL_SIGMA - 1)) == 0, "window: a power of two up to 2048 (11-bit position in the sort key)");
    const int w0 = blockIdx.x * SL_SIGMA;
    for (int q = threadIdx.x; q < SL_SIGMA; q += (int)blockDim.x) {
        const int i = w0 + q;
        const unsigned len = (i < n) ? (unsigned)(Ap[row_lo + i + 1] - Ap[row_lo + i]) : 0u;
        key[q] = (i < n) ? (((len + 1u) << 11) | (unsigned)(SL_SIGMA - 1 - q)) : 0u;      // slots past the last row: key 0, sorted last
    }
    __syncthreads();
    for (int k = 2; k <= SL_SIGMA; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < SL_SIGMA; q += (int)blockDim.x) {
                const int p = q ^ j;
                if (p > q) {
                    const unsigned a = key[q], b = key[p];
                    const bool desc = (q & k) == 0;
                    if (desc ? (a < b) : (a > b)) { key[q] = b; key[p] = a; }
                }
            }
            __syncthreads();
        }
    for (int q = threadIdx.x; q < SL_SIGMA; q += (int)blockDim.x) {
        const unsigned kq = key[q];
        const bool is_row = kq != 0u;
        const int pos = SL_SIGMA - 1 - (int)(kq & 2047u);
        const int len = is_row ? (int)(kq >> 11) - 1 : 0;
        const int slot = w0 + q;
        sl_slot[slot] = SellSlot{is_row ? row_lo + w0 + pos : -1, len};
        if ((q & (SL_C - 1)) == 0) slice_w[slot / SL_C] = len;                    // the slice's longest row comes first
    }
}

// entries of the slices, entry-major; padding entries: column 0, value 0 (requested, never used)
__global__ __launch_bounds__(SL_WG) void sell_fill_kernel(int nslices, const int *Ap, const int *Aj, const double *Ax, const SellSlot *sl_slot,
                                                               const SellHdr *sl_hdr, int *sl_col, double *sl_val)
{
    const int s = blockIdx.x * (SL_WG / SL_C) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= nslices) return;
    const long off = sl_hdr[s].off;
    const int w = sl_hdr[s].w;
    const SellSlot sl = sl_slot[s * SL_C + lane];
    const int row = sl.row, len = sl.len;
    const int k0 = row >= 0 ? Ap[row] : 0;
    for (int k = 0; k < w; ++k) {
        const bool have = k < len;
        sl_col[off + (long)k * SL_C + lane] = have ? Aj[k0 + k] : 0;
        sl_val[off + (long)k * SL_C + lane] = have ? Ax[k0 + k] : 0.0;
    }
}

struct SellArgs {
    const SellSlot *slot;
    const SellHdr *hdr;
    const int *col;
    const double *val;
    int nslices;
    const unsigned *code;        // 16-bit column codes (DevCsr::sl_code) or null
};

// 16-bit codes of one slice (one wave per slice): the distinct values of column >> 12 over the slice's real entries,
// in order of first appearance (row of 64 entries by row, lanes in order) -- at most 16, else the slice keeps its
// 32-bit columns; then the codes, two per word.  Writes the header's origins and coded flag.
__global__ __launch_bounds__(SL_WG) void sell_code_kernel(int nslices, const SellSlot *sl_slot, SellHdr *sl_hdr, const int *sl_col, unsigned *sl_code)
{
    const int s = blockIdx.x * (SL_WG / SL_C) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= nslices) return;
    const long off = sl_hdr[s].off;
    const int w = sl_hdr[s].w;
    const int len = sl_slot[s * SL_C + lane].len;
    int tab = -1;                                   // lane t < 16 holds window t's value of column >> 12
    int cnt = 0;
    bool ok = true;
    for (int k = 0; k < w && ok; ++k) {
        const bool real = k < len;
        const int hi = real ? (sl_col[off + (long)k * SL_C + lane] >> 12) : -1;
        bool pending = real;
        while (true) {
            // drop the lanes whose window is already in the table
            bool found = false;
            for (int t = 0; t < cnt; ++t) found |= (__shfl(tab, t, 64) == hi);
            pending = pending && !found;
            const unsigned long long m = __ballot(pending);
            if (m == 0ULL) break;
            if (cnt >= 16) { ok = false; break; }
            const int first = __ffsll((long long)m) - 1;
            const int nv = __shfl(hi, first, 64);
            if (lane == cnt) tab = nv;
            ++cnt;
        }
    }
    if (lane < 16) sl_hdr[s].org[lane] = (ok && lane < cnt) ? (tab << 12) : 0;
    if (lane == 0) sl_hdr[s].coded = ok ? 1 : 0;
    if (!ok) return;
    const long coff = sl_hdr[s].coff;
    for (int k = 0; k < w; k += 2) {
        unsigned word = 0;
        for (int h = 0; h < 2; ++h) {
            // (every lane runs the table look-up -- the shuffles read lanes 0 .. 15, which must be active; a padding
            //  entry's column is 0 and its code is dropped)
            const int c = (k + h < w) ? sl_col[off + (long)(k + h) * SL_C + lane] : 0;
            int slot = 0;
            for (int t = 0; t < cnt; ++t) slot = (__shfl(tab, t, 64) == (c >> 12)) ? t : slot;
            const unsigned code = (k + h < len) ? (((unsigned)slot << 12) | ((unsigned)c & 4095u)) : 0u;
            word |= code << (16 * h);
        }
        sl_code[coff + (long)(k >> 1) * SL_C + lane] = word;
    }
}

// entries k0 .. k0 + N - 1 of the lane's row, requested: q holds the code words (N / 2, coded slice) or the columns (N);
// entries at or past the slice's width w are not requested (uniform over the wave) and read as column 0, value 0
template <int N, bool IDX16>
__device__ __forceinline__ void sell_request(bool coded, const unsigned *wp, const int *cp, const double *vp, int k0, int w, unsigned (&q)[N], double (&v)[N])
{
    if (IDX16 && coded) {
#pragma unroll
        for (int u = 0; u < N; u += 2) {
            q[u / 2] = 0u;
            if (k0 + u < w) q[u / 2] = __builtin_nontemporal_load(&wp[(long)((k0 + u) >> 1) * SL_C]);
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
            v[u] = 0.0;
            if (k0 + u < w) v[u] = __builtin_nontemporal_load(&vp[(long)(k0 + u) * SL_C]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            q[u] = 0u; v[u] = 0.0;
            if (k0 + u < w) {                                       // uniform: the whole wave requests or skips
                q[u] = (unsigned)__builtin_nontemporal_load(&cp[(long)(k0 + u) * SL_C]);
                v[u] = __builtin_nontemporal_load(&vp[(long)(k0 + u) * SL_C]);
            }
        }
    }
}

// the columns of what sell_request brought, and the operands gathered (entries past the row's length: not gathered)
template <int N, bool IDX16>
__device__ __forceinline__ void sell_gather(bool coded, int org, const unsigned (&q)[N], const double *xg, int k0, int len, double (&xv)[N])
{
    int c[N];
    if (IDX16 && coded) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            const unsigned code = (q[u / 2] >> (16 * (u & 1))) & 0xffffu;
            c[u] = __shfl(org, (int)(code >> 12), 64) + (int)(code & 4095u);
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) c[u] = (int)q[u];
    }
#pragma unroll
    for (int u = 0; u < N; ++u) xv[u] = (k0 + u < len) ? xg[c[u]] : 0.0;
}

template <int N>
__device__ __forceinline__ double sell_sum(double acc, double gscale, const double (&v)[N], const double (&xv)[N], int k0, int len)
{
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const double pr = v[u] * (gscale * xv[u]);
        const double nxt = acc + pr;
        acc = (k0 + u < len) ? nxt : acc;
    }
    return acc;
}

template <int MODE, bool IDX16>
__global__ __launch_bounds__(SL_WG) void sell_kernel(StreamArgs a, SellArgs S, int xcd_chunk)
{
    const int blk = remap((int)blockIdx.x, (int)gridDim.x, xcd_chunk);
    // the slice number is the same in every lane: said to the compiler, so that the header comes in as scalar loads
    const int s = __builtin_amdgcn_readfirstlane(blk * (SL_WG / SL_C) + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (s >= S.nslices) return;
    const SellHdr *h = S.hdr + s;
    const long off = h->off;
    const long coff = h->coff;                                      // fetched with the entry offset, coded or not
    const int w = h->w;
    const bool coded = IDX16 && h->coded != 0;
    const int org = IDX16 ? h->org[lane & 15] : 0;
    const SellSlot sl = S.slot[s * SL_C + lane];
    const int row = sl.row, len = sl.len;
    const double gscale = a.gscale;
    const int *cp = S.col + off + lane;
    const double *vp = S.val + off + lane;
    const unsigned *wp = IDX16 ? S.code + coff + lane : nullptr;
    double acc = 0.0;
    // the epilogue's streamed operands do not depend on the row sum: requested first
    double ep_b = 0.0, ep_v2 = 0.0;
    if (row >= 0) {
        if (MODE == SM_RESIDUAL || MODE == SM_POLY_FIRST || MODE == SM_POLY_STEP || MODE == SM_POLY_LAST) ep_b = a.b[row];
        if (MODE == SM_POLY_LAST) ep_v2 = a.v2[row];
        if (MODE == SM_MATVEC_ACC) ep_v2 = a.out[row];
    }
    for (int k0 = 0; k0 < w; k0 += SL_PASS) {
        unsigned q[SL_PASS];
        double v[SL_PASS], xv[SL_PASS];
        sell_request<SL_PASS, IDX16>(coded, wp, cp, vp, k0, w, q, v);
        sell_gather<SL_PASS, IDX16>(coded, org, q, a.xg, k0, len, xv);
        acc = sell_sum<SL_PASS>(acc, gscale, v, xv, k0, len);
    }
    if (row < 0) return;
    if (MODE == SM_MATVEC) {
        __builtin_nontemporal_store(acc, &a.out[row]);
    } else if (MODE == SM_MATVEC_ACC) {
        __builtin_nontemporal_store(ep_v2 + acc, &a.out[row]);
    } else if (MODE == SM_RESIDUAL) {
        __builtin_nontemporal_store(ep_b - acc, &a.out[row]);
    } else if (MODE == SM_POLY_FIRST) {
        const double r = ep_b - acc;
        a.out[row] = r;
        a.out2[row] = a.c0 * r;
    } else if (MODE == SM_POLY_STEP) {
        const double cr = a.c0 * ep_b;
        a.out[row] = cr + acc;
    } else if (MODE == SM_POLY_LAST) {
        const double cr = a.c0 * ep_b;
        const double h2 = cr + acc;
        __builtin_nontemporal_store(ep_v2 + h2, &a.out[row]);
    }
}

int g_sell = 1;
int g_sell_idx16 = std::getenv("AMG_SELL_IDX16") ? std::atoi(std::getenv("AMG_SELL_IDX16")) : 1;

}   // namespace

void free_sell(DevCsr &M)
{
    M.sl_slot.reset(); M.sl_hdr.reset(); M.sl_col.reset(); M.sl_val.reset();
    M.sl_code.reset(); M.sl_frac16 = 0.0;
    M.sl_nslices = 0; M.sl_entries = 0; M.sl_lo = M.sl_hi = 0;
}

bool sell_supports(StreamMode mode)
{
    return mode == SM_MATVEC || mode == SM_MATVEC_ACC || mode == SM_RESIDUAL || mode == SM_POLY_FIRST || mode == SM_POLY_STEP ||
           mode == SM_POLY_LAST;
}
bool sell_enabled() { return g_sell != 0; }
void set_sell_form(int on) { g_sell = on; bump_config_epoch(); }
void set_sell_index16(int on) { g_sell_idx16 = on; bump_config_epoch(); }
bool sell_index16_enabled() { return g_sell_idx16 != 0; }

int launch_sell(StreamMode mode, const StreamArgs &a, const DevCsr &M, hipStream_t st)
{
    StreamArgs b = a;
    if (b.gscale == 0.0) b.gscale = 1.0;
    const bool idx16 = M.sl_code != nullptr && g_sell_idx16 != 0;
    SellArgs S{M.sl_slot, M.sl_hdr, M.sl_col, M.sl_val, M.sl_nslices, M.sl_code};
    const int grid = (M.sl_nslices + SL_WG / SL_C - 1) / (SL_WG / SL_C);
    // consecutive workgroups per XCD (speed only).  Measured at 400^3: 8 .. 128 equal within 1 %, 0 (round-robin over
    // the XCDs) 20 % slower, 512 2 % slower.  AMG_SELL_CHUNK overrides for A/B runs.
    static const int chunk_env = std::getenv("AMG_SELL_CHUNK") ? std::atoi(std::getenv("AMG_SELL_CHUNK")) : 32;
    const int chunk = grid >= 4096 ? chunk_env : 0;
    switch (mode) {
#define SELL_CASE(MODE) case MODE: if (idx16) hipLaunchKernelGGL((sell_kernel<MODE, true>), dim3(grid), dim3(SL_WG), 0, st, b, S, chunk); \
                        else hipLaunchKernelGGL((sell_kernel<MODE, false>), dim3(grid), dim3(SL_WG), 0, st, b, S, chunk); break
    SELL_CASE(SM_MATVEC);
    SELL_CASE(SM_MATVEC_ACC);
    SELL_CASE(SM_RESIDUAL);
    SELL_CASE(SM_POLY_FIRST);
    SELL_CASE(SM_POLY_STEP);
    SELL_CASE(SM_POLY_LAST);
#undef SELL_CASE
    default: set_error("launch_sell: mode not supported"); return -1;
    }
    LAUNCH_RETURN("sell launch");
}

// Built from the CSR arrays in HBM.  Only where it pays (measured on the 500^3 hierarchy, tools/sell_ab.py and the
// kernel trace): rows of 8 to 48 entries on average -- short rows (P_0: 3.4 entries) were 2x SLOWER here (a wave's 64 rows
// carry too few entries for its scattered row bookkeeping and result accesses) and stream well through the CSR kernel; longer rows (R_1: 150 entries, A_2: 67) need several dependent passes per
// slice with few slices to overlap them and were 5-70 % slower -- at least 2^16 rows, no row longer than 2046
// entries, and at most 15 % padding.
int build_sell(DevCsr &M, long *acct, int row_lo, int row_hi)
{
    const char *env = std::getenv("AMG_SELL");
    if (env && std::atoi(env) == 0) return 0;
    if (row_hi < 0) row_hi = M.nrows;
    if (row_lo < 0 || row_hi > M.nrows || row_hi <= row_lo || !M.Ap || !M.Aj || !M.Ax) return 0;
    const int n = row_hi - row_lo;
    const int sigma = (M.ncols >= 2L * M.nrows) ? SL_SIGMA_RECT : SL_SIGMA_SQUARE;
    const int nwin = (n + sigma - 1) / sigma;
    const int nslices = nwin * (sigma / SL_C);
    DevArr<int> w_dev;
    DevArr<SellSlot> slot;
    // longest row must fit the 11 + 21-bit sort key; average row length 8 .. 48 (see above)
    long nnz_range = 0;
    {
        std::vector<int> hp((size_t)n + 1);
        AMG_HIP(hipMemcpy(hp.data(), M.Ap + row_lo, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        int longest = 0;
        for (int i = 0; i < n; ++i) longest = std::max(longest, hp[(size_t)i + 1] - hp[(size_t)i]);
        if (longest > 2046) return 0;
        nnz_range = (long)hp[(size_t)n] - hp[0];
    }
    if (n < (1 << 16) || nnz_range < 8L * n || nnz_range > 48L * n) return 0;
    AMG_HIP(slot.malloc_bytes(sizeof(SellSlot) * (size_t)nslices * SL_C));
    AMG_HIP(w_dev.malloc_bytes(sizeof(int) * (size_t)nslices));
    if (sigma == SL_SIGMA_RECT) hipLaunchKernelGGL((sell_sort_kernel<SL_SIGMA_RECT>), dim3(nwin), dim3(64), 0, nullptr, row_lo, n, M.Ap, slot, w_dev);
    else hipLaunchKernelGGL((sell_sort_kernel<SL_SIGMA_SQUARE>), dim3(nwin), dim3(256), 0, nullptr, row_lo, n, M.Ap, slot, w_dev);
    LAUNCH_CHECK("sell sort launch");
    std::vector<int> hw((size_t)nslices);
    AMG_HIP(hipMemcpy(hw.data(), w_dev, sizeof(int) * (size_t)nslices, hipMemcpyDeviceToHost));
    w_dev.reset();
    // headers: entry offsets now; code-word offsets, origins and flags when the codes are built
    std::vector<SellHdr> hdr((size_t)nslices);
    long entries = 0;
    for (int s = 0; s < nslices; ++s) {
        hdr[(size_t)s] = SellHdr{};
        hdr[(size_t)s].off = entries;
        hdr[(size_t)s].w = hw[(size_t)s];
        entries += (long)hw[(size_t)s] * SL_C;
    }
    if ((double)entries > 1.15 * (double)nnz_range) return 0;
    const bool want16 = g_sell_idx16 && M.ncols >= 4096;
    long words = 0;
    if (want16)           // 16-bit column codes, two per word: ceil(width / 2) rows of 64 words per slice
        for (int s = 0; s < nslices; ++s) { hdr[(size_t)s].coff = words; words += (long)((hw[(size_t)s] + 1) / 2) * SL_C; }
    DevArr<SellHdr> hdr_dev;
    DevArr<int> col;
    DevArr<double> val;
    AMG_HIP(hdr_dev.malloc_bytes(sizeof(SellHdr) * (size_t)nslices));
    AMG_HIP(col.malloc_bytes(sizeof(int) * (size_t)std::max(entries, 1L)));
    AMG_HIP(val.malloc_bytes(sizeof(double) * (size_t)std::max(entries, 1L)));
    AMG_HIP(hipMemcpy(hdr_dev, hdr.data(), sizeof(SellHdr) * (size_t)nslices, hipMemcpyHostToDevice));
    const int bgrid = (nslices + SL_WG / SL_C - 1) / (SL_WG / SL_C);
    hipLaunchKernelGGL(sell_fill_kernel, dim3(bgrid), dim3(SL_WG), 0, nullptr, nslices, M.Ap, M.Aj, M.Ax, slot, hdr_dev, col, val);
    LAUNCH_CHECK("sell fill launch");
    AMG_HIP(hipDeviceSynchronize());
    M.sl_slot = std::move(slot); M.sl_hdr = std::move(hdr_dev); M.sl_col = std::move(col); M.sl_val = std::move(val);
    M.sl_nslices = nslices; M.sl_entries = entries; M.sl_lo = row_lo; M.sl_hi = row_hi;
    if (want16) {
        AMG_HIP(M.sl_code.malloc_bytes(sizeof(unsigned) * (size_t)std::max(words, 1L)));
        hipLaunchKernelGGL(sell_code_kernel, dim3(bgrid), dim3(SL_WG), 0, nullptr, nslices, M.sl_slot, M.sl_hdr, M.sl_col, M.sl_code);
        LAUNCH_CHECK("sell code launch");
        std::vector<SellHdr> back((size_t)nslices);
        AMG_HIP(hipMemcpy(back.data(), M.sl_hdr, sizeof(SellHdr) * (size_t)nslices, hipMemcpyDeviceToHost));
        long coded = 0;
        for (const SellHdr &r : back) coded += r.coded ? 1 : 0;
        M.sl_frac16 = nslices ? (double)coded / (double)nslices : 0.0;
        if (M.sl_frac16 < 0.5) {                                    // mostly fall-back slices: not worth the second array
            M.sl_code.reset(); M.sl_frac16 = 0.0;
            for (SellHdr &r : hdr) r.coff = 0;                       // headers as of an operator without codes
            AMG_HIP(hipMemcpy(M.sl_hdr, hdr.data(), sizeof(SellHdr) * (size_t)nslices, hipMemcpyHostToDevice));
        } else if (acct) *acct += 4L * words;
    }
    if (acct) *acct += (long)(sizeof(SellSlot) * (size_t)nslices * SL_C + sizeof(SellHdr) * (size_t)nslices + 12L * entries);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same for block operators (BASELINE configuration C5: BSR 3x3): DevBsr::bsl_*.  Block rows are sorted by block
// count inside windows of 32 slices, a slice holds NBR = 64 / bs block rows, a lane one SCALAR row (lane = block row
// in slice * bs + r).  Block k of the slice: its NBR block columns side by side, then its values as bs planes
// [c][lane] -- a lane's loads are coalesced with its neighbours', the three lanes of a block row read the same column
// and the same operands.  Arithmetic and order are bsr_stream_kernel's: BM_SPMV one running sum per scalar row across
// blocks and columns (scipy bsr_matvec); block Jacobi v = sum_c a[r][c] x[c] from 0 per block, rsum += v block by
// block, diagonal block skipped, then Dinv * (b - rsum) and the weighted update (relaxation.h:686-720).
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int BSL_WIN = 32;          // slices per sorting window
constexpr int BSL_PASS = 8;          // blocks of a row requested at once

// windows: consecutive runs of WIN block rows, or (win_start / win_len given) listed runs of at most WIN block rows --
// the level-ordered copy of a Gauss-Seidel schedule is cut so that no window, hence no slice, straddles two levels
template <int NBR>
__global__ __launch_bounds__(1024) void bsell_sort_kernel(int nb, const int *Ap, int *brow, unsigned short *blen, int *slice_w,
                                                          const int *win_start, const int *win_len)
{
    constexpr int WIN = BSL_WIN * NBR;            // block rows per window (<= 1024)
    __shared__ unsigned key[1024];
    const int w0 = win_start ? win_start[blockIdx.x] : blockIdx.x * WIN;
    const int cnt = win_start ? win_len[blockIdx.x] : min(WIN, nb - w0);
    const int q = threadIdx.x;
    {
        const int i = w0 + q;
        const bool real = q < cnt && i < nb;
        const unsigned len = real ? (unsigned)(Ap[i + 1] - Ap[i]) : 0u;
        key[q] = real ? (((len + 1u) << 10) | (unsigned)(1023 - q)) : 0u;
    }
    __syncthreads();
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int p = q ^ j;
            if (p > q) {
                const unsigned a = key[q], b = key[p];
                const bool desc = (q & k) == 0;
                if (desc ? (a < b) : (a > b)) { key[q] = b; key[p] = a; }
            }
            __syncthreads();
        }
    if (q < WIN) {
        const unsigned kq = key[q];
        const bool is_row = kq != 0u;
        const int pos = 1023 - (int)(kq & 1023u);
        const int len = is_row ? (int)(kq >> 10) - 1 : 0;
        const int slot = blockIdx.x * WIN + q;
        brow[slot] = is_row ? w0 + pos : -1;
        blen[slot] = (unsigned short)len;
        if (q % NBR == 0) slice_w[slot / NBR] = len;
    }
}

template <int BS>
__global__ __launch_bounds__(256) void bsell_fill_kernel(int nslices, const int *Ap, const int *Aj, const double *Ax, const int *brow,
                                                         const unsigned short *blen, const long *off, int *col, double *val)
{
    constexpr int NBR = 64 / BS, LW = NBR * BS;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= nslices || lane >= LW) return;
    const long o = off[s];
    const int w = (int)(off[s + 1] - o);
    const int br = lane / BS, r = lane - br * BS;
    const int row = brow[s * NBR + br], len = blen[s * NBR + br];
    const long k0 = row >= 0 ? Ap[row] : 0;
    for (int k = 0; k < w; ++k) {
        const bool have = k < len;
        if (r == 0) col[(o + k) * NBR + br] = have ? Aj[k0 + k] : 0;
        for (int c = 0; c < BS; ++c)
            val[((o + k) * BS + c) * LW + lane] = have ? Ax[(k0 + k) * (BS * BS) + r * BS + c] : 0.0;
    }
}

struct BsellArgs {
    const int *brow; const unsigned short *blen; const long *off; const int *col; const double *val; int nslices;
};

template <int BMODE, int BS>
__global__ __launch_bounds__(256) void bsell_kernel(BsrStreamArgs a, BsellArgs S, int xcd_chunk, int slice_lo, int slice_n)
{
    constexpr int NBR = 64 / BS, LW = NBR * BS, B2 = BS * BS;
    const int blk = remap((int)blockIdx.x, (int)gridDim.x, xcd_chunk);
    const int sl = blk * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (sl >= slice_n) return;
    const int s = slice_lo + sl;
    const long o = S.off[s];
    const int w = (int)(S.off[s + 1] - o);                          // uniform over the wave
    const bool lane_ok = lane < LW;
    const int br = lane_ok ? lane / BS : 0, r = lane_ok ? lane - br * BS : 0;
    const int brow = lane_ok ? S.brow[s * NBR + br] : -1;
    const int len = lane_ok ? (int)S.blen[s * NBR + br] : 0;
    const bool active = brow >= 0;
    const long ib = (long)brow * BS;
    const double gscale = (a.gscale == 0.0) ? 1.0 : a.gscale;
    double ep_b = 0.0, ep_v2 = 0.0, ep_x = 0.0;
    if (active) {
        if (BMODE == BM_BLOCK_JACOBI) { ep_b = a.b[ib + r]; ep_x = a.xin[ib + r]; }
        else if (BMODE == BM_BLOCK_GS) ep_b = a.b[ib + r];
        else {
            if (a.smode == SM_RESIDUAL || a.smode == SM_POLY_STEP || a.smode == SM_POLY_LAST) ep_b = a.b[ib + r];
            if (a.smode == SM_POLY_LAST) ep_v2 = a.v2[ib + r];
            if (a.smode == SM_MATVEC_ACC) ep_v2 = a.xout[ib + r];
        }
    }
    const int *cp = S.col + o * NBR + br;
    const double *vp = S.val + o * BS * LW + lane;
    double rsum = 0.0;
    for (int k0 = 0; k0 < w; k0 += BSL_PASS) {
        int bc[BSL_PASS];
        double v[BSL_PASS][BS], xv[BSL_PASS][BS];
#pragma unroll
        for (int u = 0; u < BSL_PASS; ++u) {
            bc[u] = 0;
#pragma unroll
            for (int c = 0; c < BS; ++c) v[u][c] = 0.0;
            if (k0 + u < w && lane_ok) {                            // (k0 + u < w is uniform)
                bc[u] = cp[(long)(k0 + u) * NBR];
#pragma unroll
                for (int c = 0; c < BS; ++c) v[u][c] = __builtin_nontemporal_load(&vp[((long)(k0 + u) * BS + c) * LW]);
            }
        }
#pragma unroll
        for (int u = 0; u < BSL_PASS; ++u)
#pragma unroll
            for (int c = 0; c < BS; ++c) xv[u][c] = (k0 + u < len) ? a.xin[(long)bc[u] * BS + c] : 0.0;
#pragma unroll
        for (int u = 0; u < BSL_PASS; ++u) {
            const bool take = k0 + u < len;
            if (BMODE == BM_SPMV) {
#pragma unroll
                for (int c = 0; c < BS; ++c) { const double nxt = rsum + v[u][c] * (gscale * xv[u][c]); rsum = take ? nxt : rsum; }
            } else {
                double vb = 0.0;
#pragma unroll
                for (int c = 0; c < BS; ++c) vb = vb + v[u][c] * xv[u][c];
                const double nxt = rsum + vb;
                rsum = (take && bc[u] != brow) ? nxt : rsum;        // the diagonal block is not part of the sum
            }
        }
    }
    if (BMODE == BM_SPMV) {
        if (!active) return;
        const long i = ib + r;
        if (a.smode == SM_MATVEC) a.xout[i] = rsum;
        else if (a.smode == SM_MATVEC_ACC) a.xout[i] = ep_v2 + rsum;
        else if (a.smode == SM_RESIDUAL) a.xout[i] = ep_b - rsum;
        else if (a.smode == SM_POLY_STEP) { const double cr = a.c0 * ep_b; a.xout[i] = cr + rsum; }
        else if (a.smode == SM_POLY_LAST) { const double cr = a.c0 * ep_b; const double h = cr + rsum; a.xout[i] = ep_v2 + h; }
        return;
    }
    // block Jacobi: x_i = (1 - omega) temp_i + omega * Dinv_i (b_i - rsum); the lanes of a block row exchange their t
    const double t = ep_b - rsum;
    double vD = 0.0;
#pragma unroll
    for (int c = 0; c < BS; ++c) {
        const double tc = __shfl(t, br * BS + c, 64);
        const double d = active ? a.Dinv[(long)brow * B2 + r * BS + c] : 0.0;
        vD = vD + d * tc;
    }
    if (active) {
        if (BMODE == BM_BLOCK_GS) a.xout[ib + r] = vD;                  // relaxation.h:756-810: x_i = Dinv_i (b_i - rsum)
        else {
            const double t1 = (1.0 - a.omega) * ep_x;
            const double t2 = a.omega * vD;
            a.xout[ib + r] = t1 + t2;
        }
    }
}

__global__ void bsell_remap_kernel(int nslots, const int *rowmap, int *brow)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nslots && brow[k] >= 0) brow[k] = rowmap[brow[k]];
}

template <int BS>
int build_bsell_bs(DevBsr &M, long *acct, const std::vector<int> *level_ptr = nullptr, const int *rowmap_dev = nullptr,
                   std::vector<int> *level_slice = nullptr)
{
    constexpr int NBR = 64 / BS, WIN = BSL_WIN * NBR;
    const int nb = M.nbrows;
    std::vector<int> ws, wl;
    if (level_ptr) {
        const int nl = (int)level_ptr->size() - 1;
        level_slice->assign((size_t)nl + 1, 0);
        for (int l = 0; l < nl; ++l) {
            (*level_slice)[(size_t)l] = (int)ws.size() * BSL_WIN;
            for (int w0 = (*level_ptr)[(size_t)l]; w0 < (*level_ptr)[(size_t)l + 1]; w0 += WIN) {
                ws.push_back(w0);
                wl.push_back(std::min(WIN, (*level_ptr)[(size_t)l + 1] - w0));
            }
        }
        (*level_slice)[(size_t)nl] = (int)ws.size() * BSL_WIN;
    }
    const int nwin = level_ptr ? (int)ws.size() : (nb + WIN - 1) / WIN;
    const int nslices = nwin * BSL_WIN;
    DevArr<int> ws_dev, wl_dev;
    if (level_ptr && nwin > 0) {
        AMG_HIP(ws_dev.malloc_bytes(sizeof(int) * (size_t)nwin));
        AMG_HIP(wl_dev.malloc_bytes(sizeof(int) * (size_t)nwin));
        AMG_HIP(hipMemcpy(ws_dev, ws.data(), sizeof(int) * (size_t)nwin, hipMemcpyHostToDevice));
        AMG_HIP(hipMemcpy(wl_dev, wl.data(), sizeof(int) * (size_t)nwin, hipMemcpyHostToDevice));
    }
    {
        std::vector<int> hp((size_t)nb + 1);
        AMG_HIP(hipMemcpy(hp.data(), M.Ap, sizeof(int) * ((size_t)nb + 1), hipMemcpyDeviceToHost));
        int longest = 0;
        for (int i = 0; i < nb; ++i) longest = std::max(longest, hp[(size_t)i + 1] - hp[(size_t)i]);
        if (longest > 60000) return 0;
    }
    DevArr<int> brow, w_dev;
    DevArr<unsigned short> blen;
    AMG_HIP(brow.malloc_bytes(sizeof(int) * (size_t)nslices * NBR));
    AMG_HIP(blen.malloc_bytes(sizeof(unsigned short) * (size_t)nslices * NBR));
    AMG_HIP(w_dev.malloc_bytes(sizeof(int) * (size_t)nslices));
    hipLaunchKernelGGL((bsell_sort_kernel<NBR>), dim3(nwin), dim3(1024), 0, nullptr, nb, M.Ap, brow, blen, w_dev, (const int *)ws_dev, (const int *)wl_dev);
    LAUNCH_CHECK("bsell sort launch");
    std::vector<int> hw((size_t)nslices);
    AMG_HIP(hipMemcpy(hw.data(), w_dev, sizeof(int) * (size_t)nslices, hipMemcpyDeviceToHost));
    w_dev.reset();
    std::vector<long> off((size_t)nslices + 1);
    off[0] = 0;
    for (int s = 0; s < nslices; ++s) off[(size_t)s + 1] = off[(size_t)s] + hw[(size_t)s];
    const long cols = off[(size_t)nslices];                          // block slot columns
    ws_dev.reset(); wl_dev.reset();
    if ((double)cols * NBR > (level_ptr ? 1.3 : 1.15) * (double)M.nblocks) return 0;
    DevArr<long> off_dev; DevArr<int> col; DevArr<double> val;
    AMG_HIP(off_dev.malloc_bytes(sizeof(long) * ((size_t)nslices + 1)));
    AMG_HIP(col.malloc_bytes(sizeof(int) * (size_t)std::max(cols * NBR, 1L)));
    AMG_HIP(val.malloc_bytes(sizeof(double) * (size_t)std::max(cols * BS * NBR * BS, 1L)));
    AMG_HIP(hipMemcpy(off_dev, off.data(), sizeof(long) * ((size_t)nslices + 1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL((bsell_fill_kernel<BS>), dim3((nslices + 3) / 4), dim3(256), 0, nullptr, nslices, M.Ap, M.Aj, M.Ax, brow, blen, off_dev, col, val);
    LAUNCH_CHECK("bsell fill launch");
    if (rowmap_dev) {                                                // x / b / Dinv are indexed by the ORIGINAL block row
        const int nslots = nslices * NBR;
        hipLaunchKernelGGL(bsell_remap_kernel, dim3((nslots + 255) / 256), dim3(256), 0, nullptr, nslots, rowmap_dev, brow);
    }
    AMG_HIP(hipDeviceSynchronize());
    M.bsl_brow = std::move(brow); M.bsl_len = std::move(blen); M.bsl_off = std::move(off_dev); M.bsl_col = std::move(col); M.bsl_val = std::move(val);
    M.bsl_nslices = nslices;
    if (acct) *acct += (long)(6L * nslices * NBR + 8L * (nslices + 1) + 4L * cols * NBR + 8L * cols * BS * NBR * BS);
    return 0;
}

}   // namespace

// from the BSR arrays in HBM; blocks of 2x2 and 3x3, at least 2^15 block rows of 4 to 48 blocks on average
int build_bsell(DevBsr &M, long *acct)
{
    const char *env = std::getenv("AMG_SELL");
    if (env && std::atoi(env) == 0) return 0;
    if (M.nbrows < (1 << 15) || M.nblocks < 4L * M.nbrows || M.nblocks > 48L * M.nbrows || !M.Ap) return 0;
    if (M.bs == 3) return build_bsell_bs<3>(M, acct);
    if (M.bs == 2) return build_bsell_bs<2>(M, acct);
    return 0;
}

// the level-ordered copy of a block Gauss-Seidel schedule: slices cut at the level boundaries; level l is slices
// level_slice[l] .. level_slice[l+1]
int build_bsell_levels(DevBsr &M, const std::vector<int> &level_ptr, const int *rowmap_dev, std::vector<int> &level_slice, long *acct)
{
    const char *env = std::getenv("AMG_SELL");
    level_slice.clear();
    if (env && std::atoi(env) == 0) return 0;
    if (M.nbrows < (1 << 15) || M.nblocks < 4L * M.nbrows || M.nblocks > 48L * M.nbrows || !M.Ap) return 0;
    // only levels of thousands of block rows: a level of 2 500 block rows (C5 at 150^3) is a launch of 30 workgroups that
    // the streamed kernel finishes in 4.8 us -- measured 20 % slower from slices; AMG_SELL_LEVELS=1 forces it (tests)
    const char *force = std::getenv("AMG_SELL_LEVELS");
    if (!(force && std::atoi(force) == 1) && (long)(level_ptr.size() - 1) * 8192L > (long)M.nbrows) return 0;
    int rc = 0;
    if (M.bs == 3) rc = build_bsell_bs<3>(M, acct, &level_ptr, rowmap_dev, &level_slice);
    else if (M.bs == 2) rc = build_bsell_bs<2>(M, acct, &level_ptr, rowmap_dev, &level_slice);
    if (!M.bsl_val) level_slice.clear();
    return rc;
}

int launch_bsell_level(const DevBsr &M, BlockMode m, const BsrStreamArgs &a, int slice_lo, int slice_hi, hipStream_t st)
{
    if (slice_hi <= slice_lo) return 0;
    BsellArgs S{M.bsl_brow, M.bsl_len, M.bsl_off, M.bsl_col, M.bsl_val, M.bsl_nslices};
    const int n = slice_hi - slice_lo;
    const int grid = (n + 3) / 4;
    if (m != BM_BLOCK_GS) { set_error("launch_bsell_level: block Gauss-Seidel only"); return -1; }
    if (M.bs == 3) hipLaunchKernelGGL((bsell_kernel<BM_BLOCK_GS, 3>), dim3(grid), dim3(256), 0, st, a, S, 0, slice_lo, n);
    else if (M.bs == 2) hipLaunchKernelGGL((bsell_kernel<BM_BLOCK_GS, 2>), dim3(grid), dim3(256), 0, st, a, S, 0, slice_lo, n);
    else { set_error("launch_bsell_level: block size not supported"); return -1; }
    LAUNCH_RETURN("bsell level launch");
}

bool bsell_level_enabled() { return g_sell != 0; }

bool bsell_applies(const DevBsr &M, BlockMode m, const BsrStreamArgs &a)
{
    if (!M.bsl_val || !g_sell || a.rowmap || a.brow_lo != 0 || a.brow_hi != M.nbrows || a.Aj != M.Aj) return false;
    if (m == BM_BLOCK_JACOBI) return true;
    if (m != BM_SPMV) return false;
    return a.smode == SM_MATVEC || a.smode == SM_MATVEC_ACC || a.smode == SM_RESIDUAL || a.smode == SM_POLY_STEP || a.smode == SM_POLY_LAST;
}

int launch_bsell(const DevBsr &M, BlockMode m, const BsrStreamArgs &a, hipStream_t st)
{
    BsellArgs S{M.bsl_brow, M.bsl_len, M.bsl_off, M.bsl_col, M.bsl_val, M.bsl_nslices};
    const int grid = (M.bsl_nslices + 3) / 4;
    const int chunk = grid >= 4096 ? 32 : 0;
    if (M.bs == 3 && m == BM_SPMV) hipLaunchKernelGGL((bsell_kernel<BM_SPMV, 3>), dim3(grid), dim3(256), 0, st, a, S, chunk, 0, M.bsl_nslices);
    else if (M.bs == 3) hipLaunchKernelGGL((bsell_kernel<BM_BLOCK_JACOBI, 3>), dim3(grid), dim3(256), 0, st, a, S, chunk, 0, M.bsl_nslices);
    else if (M.bs == 2 && m == BM_SPMV) hipLaunchKernelGGL((bsell_kernel<BM_SPMV, 2>), dim3(grid), dim3(256), 0, st, a, S, chunk, 0, M.bsl_nslices);
    else if (M.bs == 2) hipLaunchKernelGGL((bsell_kernel<BM_BLOCK_JACOBI, 2>), dim3(grid), dim3(256), 0, st, a, S, chunk, 0, M.bsl_nslices);
    else { set_error("launch_bsell: block size not supported"); return -1; }
    LAUNCH_RETURN("bsell launch");
}

}   // namespace amg
