// Host-side checks of the transpose, chain and prolong entries under AddressSanitizer and UBSan, on the CPU: the validation
// that runs before any launch (check_csr_arrays, check_unique_columns), the empty results and the argument refusals, on heap
// arrays of exactly the stated sizes so that a read past them is caught.  No GPU is used: every call here returns
// before the first device call, or with AMG_ENODEV where there is no device.  Build and run from pyamg_amd/csrc after
// `make` (classical.hip, transpose.hip and prolong.hip instrumented, the other objects as they are):
//
//   for u in classical transpose prolong; do
//     hipcc -O1 -g -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//           -c $u.hip -o /tmp/${u}_san.o; done
//   $(hipconfig -l)/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c ../../tools/sanitize_classical_chain.cpp \
//         -o /tmp/main_san.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/main_san.o /tmp/classical_san.o /tmp/transpose_san.o \
//         /tmp/prolong_san.o $(ls _obj/*.o | grep -v -e /classical.o -e /transpose.o -e /prolong.o) -ldl \
//         -o /tmp/sanitize_classical_chain \
//     && /tmp/sanitize_classical_chain
#include <cstdint>

#include "../include/amgcore_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main()
{
    // P: 3 x 4, rows stored unsorted, one column twice
    const std::vector<int> Pp{0, 2, 5, 6}, Pj{3, 0, 1, 1, 2, 0};
    const std::vector<double> Px{1, 2, 3, 4, 5, 6};
    std::vector<int> Rp(5, -7);
    amg_transpose *t = nullptr;

    auto transpose = [&](const std::vector<int> &p, const std::vector<int> &j, int n_row, int n_col) {
        std::vector<int> hp(p), hj(j);                   // exact-size heap copies
        std::vector<double> hx(Px.begin(), Px.begin() + (long)hj.size());
        return amg_csr_transpose_device(n_row, n_col, hp.data(), hj.data(), hx.data(), Rp.data(), &t);
    };
    EXPECT(transpose({1, 2, 5, 6}, Pj, 3, 4) == AMG_EINVAL && !t);             // offsets do not start at 0
    EXPECT(transpose({0, 3, 2, 6}, Pj, 3, 4) == AMG_EINVAL && !t);             // offsets decrease
    EXPECT(transpose(Pp, {3, 0, 1, 4, 2, 0}, 3, 4) == AMG_EINVAL && !t);       // a column outside the matrix
    EXPECT(transpose(Pp, {3, 0, -1, 1, 2, 0}, 3, 4) == AMG_EINVAL && !t);
    EXPECT(transpose(Pp, Pj, 3, -1) == AMG_EINVAL && !t);
    EXPECT(Rp[0] == -7 && Rp[4] == -7);                                        // refusals leave the offsets alone
    EXPECT(amg_csr_transpose_device(3, 4, Pp.data(), Pj.data(), Px.data(), nullptr, &t) == AMG_EINVAL);
    EXPECT(amg_csr_transpose_device(3, 4, Pp.data(), Pj.data(), Px.data(), Rp.data(), nullptr) == AMG_EINVAL);
    // no rows / no entries: the empty result without a device
    EXPECT(transpose({0}, {}, 0, 4) == 0 && t && Rp[0] == 0 && Rp[4] == 0);
    EXPECT(amg_csr_transpose_fetch(t, nullptr, nullptr) == 0);
    Rp.assign(5, -7);
    EXPECT(transpose({0, 0, 0, 0}, {}, 3, 4) == 0 && t && Rp[2] == 0);
    EXPECT(amg_csr_transpose_fetch(t, nullptr, nullptr) == 0);
    EXPECT(amg_csr_transpose_fetch(nullptr, nullptr, nullptr) == AMG_EINVAL);
    int route[AMG_TRANSPOSE_ROUTE_FIELDS] = {-1, -1, -1, -1};
    EXPECT(amg_transpose_last_route(route, 2) == AMG_TRANSPOSE_ROUTE_FIELDS && route[0] == 0 && route[2] == -1);
    // with entries the call goes on to the device: without one it is AMG_ENODEV, and nothing is held
    const int rc = transpose(Pp, Pj, 3, 4);
    EXPECT(rc == 0 || rc == AMG_ENODEV);
    if (rc == 0) EXPECT(amg_csr_transpose_fetch(t, nullptr, nullptr) == AMG_EINVAL);

    // the chain's begin: a square operator with a column twice, outside, bad offsets
    amg_classical_chain *c = nullptr;
    auto begin = [&](const std::vector<int> &p, const std::vector<int> &j, int n) {
        std::vector<int> hp(p), hj(j);
        std::vector<double> hx(hj.size(), 1.0);
        return amg_classical_chain_begin(n, hp.data(), hj.data(), hx.data(), 0, &c);
    };
    EXPECT(begin({0, 2, 4}, {0, 1, 1, 1}, 2) == AMG_EINVAL && !c);             // a column twice in a row
    EXPECT(begin({0, 2, 4}, {0, 1, 0, 2}, 2) == AMG_EINVAL && !c);             // outside
    EXPECT(begin({0, 2, 1}, {0, 1, 0, 1}, 2) == AMG_EINVAL && !c);
    EXPECT(begin({0}, {}, 0) == AMG_EINVAL && !c);
    EXPECT(amg_classical_chain_begin(2, nullptr, nullptr, nullptr, 0, &c) == AMG_EINVAL);
    long sizes[5];
    int flags[AMG_CHAIN_FLAG_FIELDS];
    double r[2] = {0.1, 0.2};
    EXPECT(amg_classical_chain_level(nullptr, 0.25, 0, r, 0, 0, sizes, flags, nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_classical_chain_fetch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr) == AMG_EINVAL);
    amg_classical_chain_free(nullptr);
    const int rb = begin({0, 2, 4}, {0, 1, 0, 1}, 2);
    EXPECT(rb == 0 || rb == AMG_ENODEV);
    if (rb == 0) amg_classical_chain_free(c);

    // the smoothed-aggregation chain: the same refusals at its begin, and what its level and fetch refuse without a chain
    {
        amg_sa_chain *s = nullptr;
        auto sa_begin = [&](const std::vector<int> &p, const std::vector<int> &j, int n, bool with_B = true) {
            std::vector<int> hp(p), hj(j);
            std::vector<double> hx(hj.size(), 1.0), hB((size_t)(n > 0 ? n : 0), 1.0);
            return amg_sa_chain_begin(n, hp.data(), hj.data(), hx.data(), with_B ? hB.data() : nullptr, &s);
        };
        EXPECT(sa_begin({0, 2, 4}, {0, 1, 1, 1}, 2) == AMG_EINVAL && !s);          // a column twice in a row
        EXPECT(sa_begin({0, 2, 4}, {0, 1, 0, 2}, 2) == AMG_EINVAL && !s);          // outside
        EXPECT(sa_begin({0, 2, 1}, {0, 1, 0, 1}, 2) == AMG_EINVAL && !s);          // offsets decrease
        EXPECT(sa_begin({0}, {}, 0) == AMG_EINVAL && !s);                          // an empty operator
        EXPECT(sa_begin({0, 2, 4}, {0, 1, 0, 1}, 2, false) == AMG_EINVAL && !s);   // no candidate
        EXPECT(amg_sa_chain_begin(2, nullptr, nullptr, nullptr, r, &s) == AMG_EINVAL);
        EXPECT(amg_sa_chain_begin(2, nullptr, nullptr, nullptr, r, nullptr) == AMG_EINVAL);
        int sa_flags[AMG_SA_CHAIN_FLAG_FIELDS];
        EXPECT(amg_sa_chain_level(nullptr, 2, 0.25, AMG_SA_STRENGTH_CSR, r, r, 1.0, 1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr)
               == AMG_EINVAL);
        EXPECT(amg_sa_chain_fetch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == AMG_EINVAL);
        amg_sa_chain_free(nullptr);
        const int sb = sa_begin({0, 2, 4}, {0, 1, 0, 1}, 2);
        EXPECT(sb == 0 || sb == AMG_ENODEV);
        if (sb == 0) {
            // with a chain: the options a level refuses before it touches the device, each leaving the chain as it was
            EXPECT(amg_sa_chain_level(s, 2, -0.5, AMG_SA_STRENGTH_CSR, r, r, 1.0, 1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr) == AMG_EINVAL);
            EXPECT(amg_sa_chain_level(s, 2, 0.25, 3, r, r, 1.0, 1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr) == AMG_EINVAL);
            EXPECT(amg_sa_chain_level(s, 2, 0.25, AMG_SA_STRENGTH_CSR, r, r, 1.0, -1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr) == AMG_EINVAL);
            EXPECT(amg_sa_chain_level(s, 2, 0.25, AMG_SA_STRENGTH_CSR, nullptr, r, 1.0, 1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr)
                   == AMG_EINVAL);
            EXPECT(amg_sa_chain_level(s, 3, 0.25, AMG_SA_STRENGTH_CSR, r, r, 1.0, 1, nullptr, 1e-10, sizes, sa_flags, nullptr, nullptr)
                   == AMG_EINVAL);         // not the resident operator's size: refused before y is read
            EXPECT(amg_sa_chain_fetch(s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr) == AMG_ESTATE);
            amg_sa_chain_free(s);
        }
    }

    // extended+i without rows: the empty prolongator without a device, and its fetch releases it
    {
        std::vector<int> Ap0{0}, Sp0{0}, Pp0{-7};
        amg_interpolation *e = nullptr;
        EXPECT(amg_extended_interpolation_device(0, Ap0.data(), nullptr, nullptr, Sp0.data(), nullptr, nullptr, 0, Pp0.data(), &e,
                                                 nullptr) == 0 && e && Pp0[0] == 0);
        EXPECT(amg_extended_interpolation_fetch(e, nullptr, nullptr) == 0);
    }
    // the three prolong entries: what they refuse, and return for no rows, before any device call
    {
        const std::vector<int> Ap{0, 2, 3}, Aj{0, 1, 1}, outside{0, 2, 1};
        const std::vector<double> Ax{2.0, -1.0, 2.0}, dinv{0.5, 0.5};
        std::vector<int> Sp(3, -7);
        amg_prolong *h = nullptr;
        double ms[3] = {-1.0, -1.0, -1.0};
        EXPECT(amg_symmetric_strength_device(2, Ap.data(), outside.data(), Ax.data(), 0.25, Sp.data(), &h, ms) == AMG_EINVAL && !h);
        EXPECT(amg_symmetric_strength_device(2, Ap.data(), Aj.data(), Ax.data(), -0.5, Sp.data(), &h, ms) == AMG_EINVAL && !h);
        EXPECT(Sp[0] == -7 && ms[0] == 0.0 && ms[1] == 0.0 && ms[2] == 0.0);
        const std::vector<int> none{0};
        EXPECT(amg_symmetric_strength_device(0, none.data(), nullptr, nullptr, 0.25, Sp.data(), &h, nullptr) == 0 && h && Sp[0] == 0);
        EXPECT(amg_symmetric_strength_fetch(h, nullptr, nullptr, ms) == 0);
        // AggOp 2 x 2 with node 0 in both aggregates; then no nodes
        const std::vector<int> two_p{0, 2, 2}, two_j{0, 1};
        const std::vector<double> B{1.0, 1.0};
        std::vector<double> Tx(2, -7.0), R(2, -7.0);
        EXPECT(amg_fit_candidates_device(2, 2, 1, 1, two_p.data(), two_j.data(), B.data(), 1e-10, Tx.data(), R.data(), ms) == AMG_EINVAL);
        EXPECT(amg_fit_candidates_device(2, 2, 1, 0, Ap.data(), Aj.data(), B.data(), 1e-10, Tx.data(), R.data(), ms) == AMG_EINVAL);
        EXPECT(amg_fit_candidates_device(0, 2, 1, 1, none.data(), nullptr, nullptr, 1e-10, nullptr, R.data(), ms) == 0);
        EXPECT(Tx[0] == -7.0 && R[0] == -7.0);
        // T 2 x 2 with column 1 twice in row 1; then a column of S outside; then no rows
        const std::vector<int> twice_j{0, 1, 1}, Tp{0, 1, 3};
        h = nullptr;
        EXPECT(amg_jacobi_prolongation_device(2, 2, Ap.data(), Aj.data(), Ax.data(), dinv.data(), 1.0, 1, Tp.data(), twice_j.data(),
                                              Ax.data(), Sp.data(), &h, ms) == AMG_EINVAL && !h);
        EXPECT(amg_jacobi_prolongation_device(2, 2, Ap.data(), outside.data(), Ax.data(), dinv.data(), 1.0, 1, Ap.data(), Aj.data(),
                                              Ax.data(), Sp.data(), &h, ms) == AMG_EINVAL && !h);
        Sp[0] = -7;
        EXPECT(amg_jacobi_prolongation_device(0, 2, none.data(), nullptr, nullptr, nullptr, 1.0, 1, none.data(), nullptr, nullptr,
                                              Sp.data(), &h, ms) == 0 && h && Sp[0] == 0);
        EXPECT(amg_jacobi_prolongation_fetch(h, nullptr, nullptr, ms) == 0);
        EXPECT(amg_symmetric_strength_fetch(nullptr, nullptr, nullptr, nullptr) == AMG_EINVAL);
        EXPECT(amg_jacobi_prolongation_fetch(nullptr, nullptr, nullptr, nullptr) == AMG_EINVAL);
    }
    // every fetch refuses a null handle
    EXPECT(amg_extended_interpolation_fetch(nullptr, nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_classical_level_fetch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_strength_fetch(nullptr, nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_energy_fetch(nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_galerkin_fetch(nullptr, nullptr, nullptr) == AMG_EINVAL);
    EXPECT(amg_galerkin_fetch_c128(nullptr, nullptr, nullptr) == AMG_EINVAL);
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
