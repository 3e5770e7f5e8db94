// The distance-k maximal independent set (amg_core/graph.h:455-589) and the MIS(2) aggregation built on it (DESIGN.md
// section 8l) on the device.  One lane per vertex.  Every pass is written out of place: a kernel reads its neighbours
// only from arrays the previous launch wrote and writes only its own vertex, so the integers are those of the
// reference's sequential loops however the lanes are scheduled, and there is nothing for a stale read to change.
// Offsets are widened to 64 bits inside the kernels.
#include "graph_dev.hpp"

namespace amg {
namespace {

// The state of the propagation, one 16-byte record per vertex so that a neighbour costs one gather.
struct alignas(16) Pair {
    double value;
    int key;
    int pad;
};

// Round 0: nobody is in the set, everybody is active and carries its own (key, y).
__global__ __launch_bounds__(TB) void misk_start_kernel(int n, const double *y, Pair *state, int *x, int *active)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    state[i] = Pair{y[i], i, 0};
    x[i] = 0;
    active[i] = 1;
}

// csr_propagate_max (graph.h:469-499): the (value, key) maximum over the vertex and the columns of its row, the larger
// key on equal values.  Equal keys carry equal values, so the maximum does not depend on the order of the row.
__global__ __launch_bounds__(TB) void misk_propagate_kernel(int n, const int *Ap, const int *Aj, const Pair *in, Pair *out)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    Pair best = in[i];
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi; ++jj) {
        const Pair c = in[Aj[jj]];
        if (c.key == best.key) continue;
        if (c.value < best.value) continue;
        if (c.value > best.value || c.key > best.key) best = c;
    }
    out[i] = best;
}

// End of phase 1: an active vertex whose own key came back joins the set.  reach[i] starts phase 2 as x[i]; lane 0
// clears the round's flag for misk_retire_kernel.
__global__ __launch_bounds__(TB) void misk_join_kernel(int n, const Pair *state, const int *active, int *x, int *reach, int *work_left)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i == 0) *work_left = 0;
    if (i >= n) return;
    int member = x[i];
    if (state[i].key == i && active[i]) member = 1;
    x[i] = member;
    reach[i] = member;
}

// Phase 2 only ever asks whether the propagated value is 1.  The reference propagates the pairs (i, x[i]) with x in
// {0, 1}; equal keys carry equal values within a phase, so the value component of the (value, key) maximum is the
// maximum of the values, which is 1 exactly where a member is within the hops taken so far: plain reachability, one
// int per vertex.
__global__ __launch_bounds__(TB) void misk_reach_kernel(int n, const int *Ap, const int *Aj, const int *in, int *out)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    int hit = in[i];
    const long hi = Ap[i + 1];
    for (long jj = Ap[i]; jj < hi && !hit; ++jj) hit = in[Aj[jj]];
    out[i] = hit;
}

// End of the round (graph.h:572-583): a vertex a member reached retires with the value -1, the others carry y again
// and ask for another round.
__global__ __launch_bounds__(TB) void misk_retire_kernel(int n, const int *reach, const double *y, int *active, Pair *state, int *work_left)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    if (reach[i]) {
        active[i] = 0;
        state[i] = Pair{-1.0, i, 0};
    } else {
        state[i] = Pair{y[i], i, 0};
        *work_left = 1;
    }
}

// The rounds on a graph that is already in HBM.  x: n ints, written (1 = member, 0 = not).  *rounds: rounds run.
// One 4-byte read per round tells the host whether work is left.
int mis_k_rounds_device(int n, const int *Ap, const int *Aj, int k, const double *y, int max_iters, int *x, int *rounds)
{
    const size_t vbytes = sizeof(int) * (size_t)n;
    DBuf state_a, state_b, reach_a, reach_b, active, flag;
    CHK(state_a.alloc(sizeof(Pair) * (size_t)n)); CHK(state_b.alloc(sizeof(Pair) * (size_t)n));
    CHK(reach_a.alloc(vbytes)); CHK(reach_b.alloc(vbytes)); CHK(active.alloc(vbytes));
    CHK(flag.alloc(sizeof(int)));
    hipLaunchKernelGGL(misk_start_kernel, grid_for(n), dim3(TB), 0, nullptr, n, y, state_a.as<Pair>(), x, active.i());
    LAUNCH_CHECK("mis_k: start launch");
    int done = 0, again = 1;
    while (again && (max_iters == -1 || done < max_iters)) {
        // a round that leaves work adds a member unless an active weight lies below a retired vertex's -1: the
        // reference's loop never ends on such weights
        if (done > n) { set_error("mis_k: no vertex joined in a round (an active weight at or below -1?)"); return AMG_ESTATE; }
        Pair *cur = state_a.as<Pair>(), *nxt = state_b.as<Pair>();
        for (int t = 0; t < k; ++t) {
            hipLaunchKernelGGL(misk_propagate_kernel, grid_for(n), dim3(TB), 0, nullptr, n, Ap, Aj, (const Pair *)cur, nxt);
            LAUNCH_CHECK("mis_k: propagation launch");
            std::swap(cur, nxt);
        }
        int *rcur = reach_a.i(), *rnxt = reach_b.i();
        hipLaunchKernelGGL(misk_join_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const Pair *)cur, (const int *)active.i(), x, rcur,
                           flag.i());
        LAUNCH_CHECK("mis_k: join launch");
        for (int t = 0; t < k; ++t) {
            hipLaunchKernelGGL(misk_reach_kernel, grid_for(n), dim3(TB), 0, nullptr, n, Ap, Aj, (const int *)rcur, rnxt);
            LAUNCH_CHECK("mis_k: reach launch");
            std::swap(rcur, rnxt);
        }
        hipLaunchKernelGGL(misk_retire_kernel, grid_for(n), dim3(TB), 0, nullptr, n, (const int *)rcur, y, active.i(),
                           state_a.as<Pair>(), flag.i());
        LAUNCH_CHECK("mis_k: retire launch");
        AMG_HIP(hipMemcpy(&again, flag.p, sizeof(int), hipMemcpyDeviceToHost));
        ++done;
    }
    *rounds = done;
    return 0;
}

// ------------------------------------------------------------------------------------------------ MIS(2) aggregation
// root[i]: a member of the set with an off-diagonal entry; lane n writes the scan's last addend
__global__ __launch_bounds__(TB) void agg_root_kernel(int n, const int *Ap, const int *Aj, const int *x, int *root)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i > n) return;
    int is_root = 0;
    if (i < n && x[i]) {
        const long hi = Ap[i + 1];
        for (long jj = Ap[i]; jj < hi && !is_root; ++jj) is_root = Aj[jj] != i;
    }
    root[i] = is_root;
}

// Round 1 and the list of roots: a root takes its number (the scan of root), a vertex next to a root that root's.
// Roots are at least three edges apart, so a row holds at most one of them, however often.
__global__ __launch_bounds__(TB) void agg_round1_kernel(int n, const int *Ap, const int *Aj, const int *root, const int *number, int *agg,
                                                        int *cpts)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    int a = -1;
    if (root[i]) {
        a = number[i];
        cpts[a] = i;
    } else {
        const long hi = Ap[i + 1];
        for (long jj = Ap[i]; jj < hi; ++jj) {
            const int j = Aj[jj];
            if (root[j]) { a = number[j]; break; }
        }
    }
    agg[i] = a;
}

// Round 2 reads round 1's result and writes a new array: a vertex still unassigned joins, among the aggregates of its
// round-1 neighbours, the one whose root has the largest (y[root], root).
__global__ __launch_bounds__(TB) void agg_round2_kernel(int n, const int *Ap, const int *Aj, const int *agg1, const int *cpts,
                                                        const double *y, int *agg2)
{
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    int a = agg1[i];
    if (a < 0) {
        int best = -1;
        double y_best = 0.0;
        const long hi = Ap[i + 1];
        for (long jj = Ap[i]; jj < hi; ++jj) {
            const int aj = agg1[Aj[jj]];
            if (aj < 0) continue;
            const int r = cpts[aj];
            const double yr = y[r];
            if (best < 0 || yr > y_best || (yr == y_best && r > best)) { best = r; y_best = yr; a = aj; }
        }
    }
    agg2[i] = a;
}

}   // namespace

// The aggregation of a graph that is already in HBM (p, j: its n + 1 offsets and columns; y: the n weights) into freshly
// allocated agg (n ints, -1: no aggregate) and cpts (the roots, *n_agg of them, ascending).  *rounds: rounds of the set.
// Crosses units (graph_dev.hpp): the smoothed-aggregation chain of prolong.hip calls it.
int mis_aggregation_resident(int n, const int *p, const int *j, const double *y, DBuf &agg, DBuf &cpts, int *n_agg, int *rounds)
{
    const size_t vbytes = sizeof(int) * (size_t)n;
    DBuf dx, root, number, agg1;
    CHK(dx.alloc(vbytes)); CHK(agg1.alloc(vbytes)); CHK(agg.alloc(vbytes)); CHK(cpts.alloc(vbytes));
    CHK(root.alloc(vbytes + sizeof(int)));
    CHK(mis_k_rounds_device(n, p, j, 2, y, -1, dx.i(), rounds));
    hipLaunchKernelGGL(agg_root_kernel, grid_for((long)n + 1), dim3(TB), 0, nullptr, n, p, j, (const int *)dx.i(), root.i());
    LAUNCH_CHECK("mis_aggregation: root launch");
    long count = 0;
    CHK(offsets_from_counts("mis_aggregation", n, root.i(), n, number, &count));
    hipLaunchKernelGGL(agg_round1_kernel, grid_for(n), dim3(TB), 0, nullptr, n, p, j, (const int *)root.i(), (const int *)number.i(),
                       agg1.i(), cpts.i());
    LAUNCH_CHECK("mis_aggregation: round 1 launch");
    hipLaunchKernelGGL(agg_round2_kernel, grid_for(n), dim3(TB), 0, nullptr, n, p, j, (const int *)agg1.i(), (const int *)cpts.i(), y,
                       agg.i());
    LAUNCH_CHECK("mis_aggregation: round 2 launch");
    AMG_HIP(hipDeviceSynchronize());
    *n_agg = (int)count;
    return 0;
}

}   // namespace amg

extern "C" {

int amg_mis_k_device(int n, const int *Ap, const int *Aj, int k, const double *y, int max_iters, int *x, int *rounds, double *times_ms)
{
    using namespace amg;
    if (n < 0 || k < 1 || (n > 0 && (!y || !x))) { set_error("mis_k: bad arguments"); return AMG_EINVAL; }
    if (rounds) *rounds = 0;
    clear_times(times_ms);
    if (n == 0) return 0;
    CHK(check_graph("mis_k", n, Ap, Aj));
    CHK(require_device());
    LapClock timer;
    HbmCsr G;
    DBuf dy, dx;
    CHK(G.upload(n, Ap, Aj, nullptr));
    CHK(dy.from_host(y, sizeof(double) * (size_t)n));
    CHK(dx.alloc(sizeof(int) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    int done = 0;
    CHK(mis_k_rounds_device(n, G.p.i(), G.j.i(), k, dy.d(), max_iters, dx.i(), &done));
    AMG_HIP(hipDeviceSynchronize());
    const double rounds_ms = timer.lap();
    CHK(dx.to_host(x, sizeof(int) * (size_t)n));
    if (rounds) *rounds = done;
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = rounds_ms; times_ms[2] = timer.lap(); }
    return 0;
}

int amg_mis_aggregation_device(int n, const int *Ap, const int *Aj, const double *y, int *agg, int *cpts, int *n_agg, int *rounds,
                               double *times_ms)
{
    using namespace amg;
    if (n < 0 || !n_agg || (n > 0 && (!y || !agg || !cpts))) { set_error("mis_aggregation: bad arguments"); return AMG_EINVAL; }
    *n_agg = 0;
    if (rounds) *rounds = 0;
    clear_times(times_ms);
    if (n == 0) return 0;
    CHK(check_graph("mis_aggregation", n, Ap, Aj));
    CHK(require_device());
    LapClock timer;
    HbmCsr G;
    DBuf dy, dagg, dcpts;
    CHK(G.upload(n, Ap, Aj, nullptr));
    CHK(dy.from_host(y, sizeof(double) * (size_t)n));
    AMG_HIP(hipDeviceSynchronize());
    const double upload_ms = timer.lap();
    int done = 0, count = 0;
    CHK(mis_aggregation_resident(n, G.p.i(), G.j.i(), dy.d(), dagg, dcpts, &count, &done));
    const double rounds_ms = timer.lap();
    CHK(dagg.to_host(agg, sizeof(int) * (size_t)n));
    CHK(dcpts.to_host(cpts, sizeof(int) * (size_t)count));
    *n_agg = count;
    if (rounds) *rounds = done;
    if (times_ms) { times_ms[0] = upload_ms; times_ms[1] = rounds_ms; times_ms[2] = timer.lap(); }
    return 0;
}

}   // extern "C"
