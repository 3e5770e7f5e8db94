// What the graph stages of the setup share on the host side of their drivers (split.hip, misagg.hpp): the check every
// host graph passes before anything is launched on it, and the int scan that numbers what a kernel flagged.
#pragma once
#include "flat.hpp"

#include <rocprim/device/device_scan.hpp>

#include <string>

namespace amg {
namespace {

// n + 1 offsets from 0 up, never decreasing, every column inside the matrix: nothing is launched on less
[[maybe_unused]] int check_graph(const char *who, int n, const int *p, const int *j)
{
    if (!p || p[0] != 0) { set_error(std::string(who) + ": offsets do not start at 0"); return AMG_EINVAL; }
    for (int i = 0; i < n; ++i)
        if (p[i + 1] < p[i]) { set_error(std::string(who) + ": offsets decrease"); return AMG_EINVAL; }
    if (p[n] > 0 && !j) { set_error(std::string(who) + ": null index array"); return AMG_EINVAL; }
    for (int e = 0; e < p[n]; ++e)
        if (j[e] < 0 || j[e] >= n) { set_error(std::string(who) + ": column index outside the graph"); return AMG_EINVAL; }
    return 0;
}

// out[k] = in[0] + ... + in[k - 1] for k < count
[[maybe_unused]] int exclusive_scan(const int *in, int *out, size_t count)
{
    size_t bytes = 0;
    AMG_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, count, rocprim::plus<int>(), nullptr));
    DBuf tmp;
    CHK(tmp.alloc(bytes));
    AMG_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, 0, count, rocprim::plus<int>(), nullptr));
    return 0;
}

}  // namespace
}  // namespace amg
