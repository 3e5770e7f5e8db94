// Host-side helpers of the flat amg_core entries (include/amgcore_hip.h, section 1), shared by
// capi.hip (float64) and typed.hip (float32 / complex64 / complex128): argument checks and the row
// list of a sweep.  The owning device buffer they stage their operands in is driver.hpp's.
#pragma once
#include "amg_dev.hpp"
#include "../../include/amgcore_hip.h"

#include <vector>

namespace amg {
namespace {

int require_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (amgcore_hip has no CPU fallback)");
        return AMG_ENODEV;
    }
    return 0;
}

// the rows visited by for(i = start; i != stop; i += step)
[[maybe_unused]] int sweep_rows(int start, int stop, int step, int limit, std::vector<int> &rows)
{
    rows.clear();
    if (step == 0) { set_error("row_step == 0"); return AMG_EINVAL; }
    long span = (long)stop - start;
    if (span == 0) return 0;
    if (span % step != 0 || span / step < 0) {
        set_error("row_start/row_stop/row_step never terminate");
        return AMG_EINVAL;
    }
    long cnt = span / step;
    rows.resize((size_t)cnt);
    for (long t = 0; t < cnt; ++t) {
        long i = start + t * step;
        if (i < 0 || i >= limit) { set_error("sweep leaves the matrix"); return AMG_EINVAL; }
        rows[(size_t)t] = (int)i;
    }
    return 0;
}

[[maybe_unused]] int check_csr(const int *Ap, int Ap_size, int Aj_size, int Ax_size, int per_entry)
{
    if (!Ap || Ap_size < 1) { set_error("bad Ap"); return AMG_EINVAL; }
    long nnz = Ap[Ap_size - 1];
    if (nnz < 0 || nnz > Aj_size || nnz * per_entry > Ax_size) {
        set_error("Aj/Ax shorter than Ap[-1]");
        return AMG_EINVAL;
    }
    return 0;
}

}  // namespace
}  // namespace amg
