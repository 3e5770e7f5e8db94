// Host-side scaffold of the two plain resident engines (include/amgcore_hip.h, sections 5 and 6), shared by
// hier_c128.hip (complex128 values) and hier_multi.hip (several float64 right-hand sides): launch helpers, counted
// device buffers, the dependency levels of a sweep, the engine's lifetime and bookkeeping, the V / W / F recursion,
// the skeleton of finalize and the slot checks of the setters.  Kernels, operator loading, smoothers, norms and the
// solve loops stay with each engine; the templates below reach them through a small ops object the engine passes.
#pragma once
#include "hier.hpp"
#include "flat.hpp"

#include <string>
#include <vector>

namespace amg {
namespace {

enum { COARSE_NONE = 0, COARSE_DENSE = 1, COARSE_SMOOTHER = 2, COARSE_CALLBACK = 3 };

int blocks_of(long n, int per) { return (int)((n + per - 1) / per); }

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

// dependency levels of a sweep over the (block) rows of a pattern (rows in level order on the device)
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

// what every resident engine holds besides its levels; an engine derives from it and adds `lv` (levels with A, P, R
// and sm[2]) and `csm` (the relaxation-named coarse solver)
struct Core {
    int device = 0, nlev = 0;
    bool finalized = false;
    bool sealed = false;                  // finalize has run: the operators, smoothers and coarse solver are fixed
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int coarse = COARSE_NONE;
    DBuf M;                               // dense coarse operator, nM x nM
    int nM = 0;
    DBuf part, res;                       // partial sums of a norm; the residual history
    int nres_cap = 0;                     // iteration slots of res
    double last_ms = 0.0;
    Pool pool;
    ~Core()
    {
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (st) hipStreamDestroy(st);
    }
    int open(int dev, int nlevels)
    {
        device = dev;
        nlev = nlevels;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&ev0) != hipSuccess ||
            hipEventCreate(&ev1) != hipSuccess) {
            set_error("hipStreamCreate / hipEventCreate failed");
            return AMG_ENODEV;
        }
        return 0;
    }
    // res holds maxiter + 2 slots of `per_slot` doubles (the last one: ||b||); it only ever grows
    int reserve_history(int maxiter, int per_slot)
    {
        if (nres_cap >= maxiter + 2) return 0;
        pool.bytes -= (long)sizeof(double) * nres_cap * per_slot;
        res.reset();
        nres_cap = 0;
        CHK(pool.alloc(res, sizeof(double) * (size_t)(maxiter + 2) * per_slot));
        nres_cap = maxiter + 2;
        return 0;
    }
    // last_ms = the time of run() on the stream; store() brings the result to the host and synchronises
    template <class Run, class Store>
    int timed(Run run, Store store)
    {
        AMG_HIP(hipEventRecord(ev0, st));
        CHK(run());
        AMG_HIP(hipEventRecord(ev1, st));
        CHK(store());
        float ms = 0.f;
        AMG_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        last_ms = ms;
        return 0;
    }
};

// ----------------------------------------------------------------------------------------------- cycle
// multilevel.py:473-548 on level l (V, W, F); x_l and b_l live in the level's vectors.  Ops: relax(l, 0 pre | 1 post),
// residual(l): r_l = b_l - A_l x_l, restrict_residual(l): b_{l+1} = R_l r_l, zero_x(l), coarse_solve() on the last
// level's x and b, prolong_add(l): x_l += P_l x_{l+1}
template <class Ops>
int cycle_level(Ops &o, int nlev, int l, int cyc)
{
    CHK(o.relax(l, 0));
    CHK(o.residual(l));
    CHK(o.restrict_residual(l));
    CHK(o.zero_x(l + 1));
    if (l == nlev - 2) {
        CHK(o.coarse_solve());
    } else if (cyc == AMG_CYCLE_V) {
        CHK(cycle_level(o, nlev, l + 1, AMG_CYCLE_V));
    } else if (cyc == AMG_CYCLE_W) {
        CHK(cycle_level(o, nlev, l + 1, AMG_CYCLE_W));
        CHK(cycle_level(o, nlev, l + 1, AMG_CYCLE_W));
    } else {
        CHK(cycle_level(o, nlev, l + 1, AMG_CYCLE_F));
        CHK(cycle_level(o, nlev, l + 1, AMG_CYCLE_V));
    }
    CHK(o.prolong_add(l));
    return o.relax(l, 1);
}

template <class Ops>
int one_cycle(Ops o, int nlev, int cyc)
{
    if (nlev == 1) return o.coarse_solve();          // multilevel.py:456-458: x = coarse_solver(A, b)
    return cycle_level(o, nlev, 0, cyc);
}

// ----------------------------------------------------------------------------------------------- setup
template <class Mat>
void drop_pattern(Mat &M)
{
    std::vector<int>().swap(M.hAp);
    std::vector<int>().swap(M.hAj);
}

// `api`: the engine's finalize entry, for the messages.  Own: square(A) refuses an A the engine cannot take,
// build_smoother(L, s), level_vectors(l) allocates the level's work vectors, finish() the engine's scratch buffers
// (and drops the host patterns it keeps besides A, P and R)
template <class E, class Own>
int finalize(E &e, const char *api, Own own)
{
    if (e.sealed) {
        if (e.finalized) return 0;
        set_error(std::string("an earlier ") + api + " failed; build a new hierarchy");
        return AMG_ESTATE;
    }
    e.sealed = true;                      // the schedules below consume the host patterns: no setter may follow
    for (int l = 0; l < e.nlev; ++l) {
        auto &L = e.lv[l];
        if (!L.A.set) { set_error("level " + std::to_string(l) + ": A missing"); return AMG_ESTATE; }
        CHK(own.square(L.A));
        const int n = L.A.nrows;
        if (l < e.nlev - 1) {
            const auto &An = e.lv[l + 1].A;
            if (!L.P.set || !L.R.set) { set_error("level " + std::to_string(l) + ": P or R missing"); return AMG_ESTATE; }
            if (L.P.nrows != n || L.P.ncols != An.nrows || L.R.nrows != An.nrows || L.R.ncols != n) {
                set_error("level " + std::to_string(l) + ": P / R shapes do not match A");
                return AMG_EINVAL;
            }
            for (int w = 0; w < 2; ++w) CHK(own.build_smoother(L, L.sm[w]));
        }
        CHK(own.level_vectors(l));
    }
    auto &Lc = e.lv[e.nlev - 1];
    if (e.coarse == COARSE_SMOOTHER) CHK(own.build_smoother(Lc, e.csm));
    if (e.coarse == COARSE_DENSE && e.nM != Lc.A.nrows) { set_error("dense coarse operator has the wrong size"); return AMG_EINVAL; }
    CHK(own.finish());
    for (auto &L : e.lv) {                // the patterns served the schedules
        drop_pattern(L.A);
        drop_pattern(L.P);
        drop_pattern(L.R);
    }
    e.finalized = true;
    return 0;
}

// the slot of a smoother descriptor (which: 0 pre, 1 post, 2 coarse) of kind 0 .. kind_max; `where` ends the message
// about a kind the engine does not have
template <class E, class Desc, class Sm>
int smoother_slot(E &e, int lvl, int which, const Desc *d, int kind_max, const char *where, Sm *&s)
{
    if (lvl < 0 || lvl >= e.nlev || which < 0 || which > 2 || !d) { set_error("bad smoother slot"); return AMG_EINVAL; }
    if (which == 2 && lvl != e.nlev - 1) { set_error("the coarse smoother belongs to the last level"); return AMG_EINVAL; }
    if (which < 2 && lvl == e.nlev - 1) { set_error("the last level has no pre/post smoother"); return AMG_EINVAL; }
    if (d->kind < 0 || d->kind > kind_max) {
        set_error("smoother kind " + std::to_string(d->kind) + " has no implementation " + where);
        return AMG_ENOTIMPL;
    }
    s = which == 2 ? &e.csm : &e.lv[lvl].sm[which];
    if (s->set) { set_error("smoother already set"); return AMG_ESTATE; }
    if (which == 2 && e.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    return 0;
}

template <class Desc>
int check_sweeps(const Desc *d)
{
    if (d->iterations < 0 || d->sweep < 0 || d->sweep > 2) { set_error("bad iterations / sweep"); return AMG_EINVAL; }
    return 0;
}

// the operator a set_matrix call names (which: 0 A, 1 P, 2 R), nullptr (AMG_EINVAL) for a slot that does not exist
template <class E>
auto operator_slot(E &e, int lvl, int which) -> decltype(&e.lv[0].A)
{
    if (lvl < 0 || lvl >= e.nlev || which < 0 || which > 2 || (which > 0 && lvl == e.nlev - 1)) {
        set_error("bad level / operator slot");
        return nullptr;
    }
    auto &L = e.lv[lvl];
    return which == 0 ? &L.A : which == 1 ? &L.P : &L.R;
}

// M: n x n values of `elem` bytes, row-major
int set_coarse_dense(Core &e, const void *M, int n, size_t elem)
{
    if (n < 0 || (!M && n)) { set_error("bad dense operator"); return AMG_EINVAL; }
    if (e.coarse != COARSE_NONE) { set_error("coarse solver already set"); return AMG_ESTATE; }
    CHK(e.pool.upload(e.M, M, elem * (size_t)n * n));
    e.nM = n;
    e.coarse = COARSE_DENSE;
    return 0;
}

// ----------------------------------------------------------------------------------------------- handles
// H: a handle struct whose member `e` is the engine; the caller has checked its own arguments
template <class H>
int open_handle(int nlevels, int device, H **out)
{
    CHK(require_device());
    AMG_HIP(hipSetDevice(device));
    H *h = new H();
    h->e.lv.resize(nlevels);
    const int rc = h->e.open(device, nlevels);
    if (rc != 0) {
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

template <class H>
void close_handle(H *h)
{
    if (!h) return;
    hipSetDevice(h->e.device);
    hipDeviceSynchronize();
    delete h;
}

}  // namespace
}  // namespace amg

#define ENTER(h)                                                        \
    if (!(h)) { amg::set_error("null hierarchy"); return AMG_EINVAL; }  \
    AMG_HIP(hipSetDevice((h)->e.device))
// setters: only before the engine's finalize entry `api`
#define UNSEALED(h, api)                                                                                        \
    if ((h)->e.sealed) {                                                                                        \
        amg::set_error(std::string("hierarchy already finalised: operators and solvers are set before ") + api); \
        return AMG_ESTATE;                                                                                      \
    }
