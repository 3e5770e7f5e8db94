"""What every setup stage with a host route and a device route shares: the binding of the CPU-side setup library
(csrc/setup_host.cpp -> lib/libamgsetup_host.so), the array and pointer helpers of its call sites, and the policy that
reads a stage's ``device`` argument.

``device=True`` is the device entry with its refusals raised, ``device=None`` the device entry with its refusals answered
by the host route, ``device=False`` the host route.  What ``None`` means when a GPU is present is each stage's own
decision (its ``DEVICE_AUTO`` and whatever gates it adds); ``route`` only combines that decision with
``device_present``.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import VALUE_CTYPES, dp, ip  # noqa: F401  (ip, dp: the int32 / float64 pointer helpers, used from here)

HERE = os.path.dirname(os.path.abspath(__file__))
_loaded = None


def _signatures():
    """every amgsetup_* entry of csrc/setup_host.cpp: name -> (restype, argtypes)"""
    I, L, D, V = C.c_int, C.c_int64, C.c_double, C.c_void_p
    i, l, d = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    sig = {
        # smoothed aggregation (aggregation.py, util.py, gallery.py)
        "amgsetup_standard_aggregation": (I, [I, i, i, i, i]),
        "amgsetup_gauss_seidel": (None, [i, i, d, d, d, I, I, I]),
        "amgsetup_block_gauss_seidel": (None, [i, i, d, d, d, d, I, I, I, I]),
        "amgsetup_gauss_seidel_c128": (None, [i, i, V, V, V, I, I, I]),
        "amgsetup_block_gauss_seidel_c128": (None, [i, i, V, V, V, V, I, I, I, I]),
        "amgsetup_pinv_blocks_c128": (None, [V, I, I]),
        "amgsetup_csr_diagonal_inv": (None, [I, l, i, d, d]),
        "amgsetup_gauss_seidel_pipelined": (I, [i, i, d, d, d, I, I, I]),
        "amgsetup_block_gauss_seidel_pipelined": (I, [i, i, d, d, d, d, I, I, I, I]),
        "amgsetup_csr_matmat_count": (L, [I, I, l, i, l, i, l]),
        "amgsetup_csr_matmat_fill": (L, [I, I, l, i, d, l, i, d, l, i, d]),
        "amgsetup_csr_sort_indices": (None, [I, l, i, d]),
        "amgsetup_csr_transpose": (None, [I, I, l, i, d, l, i, d]),
        "amgsetup_fit_candidates_scalar": (None, [I, i, i, d, d, d, D]),
        "amgsetup_poisson_nnz": (L, [I, I, I]),
        "amgsetup_poisson": (None, [I, I, I, D, l, i, d]),
        "amgsetup_tentative_scalar": (L, [I, I, i, d, D, l, i, d, d]),
        "amgsetup_smooth_prolongator": (L, [I, I, l, i, d, d, D, l, i, d, l, i, d]),
        "amgsetup_bsr_matmat_count": (L, [I, l, i, l, i, l]),
        "amgsetup_bsr_matmat_fill": (None, [I, I, I, I, l, i, d, l, i, d, l, i, d]),
        "amgsetup_bsr_transpose": (None, [I, I, I, I, l, i, d, l, i, d]),
        "amgsetup_smooth_prolongator_block": (L, [I, I, I, l, i, d, d, D, i, d, l, i, d, i]),
        "amgsetup_kuhn_p1_diffusion": (L, [I, d, d, l, i, d]),
        "amgsetup_greedy_coloring": (I, [I, i, i, i]),
        "amgsetup_pattern_symmetric": (I, [I, i, i]),
        "amgsetup_extract_subblocks": (None, [i, i, d, d, i, i, i, I, I]),
        # evolution strength (strength.py)
        "amgsetup_incomplete_mat_mult_csr": (None, [i, i, d, i, i, d, i, i, d, I]),
        "amgsetup_apply_distance_filter": (None, [I, D, i, i, d, I]),
        # energy smoothing (smooth.py, util.py)
        "amgsetup_incomplete_mat_mult_bsr": (None, [i, i, d, i, i, d, i, i, d] + [I] * 5),
        "amgsetup_satisfy_constraints_helper": (None, [I] * 4 + [d, d, d, i, i, d]),
        "amgsetup_calc_BtB": (None, [I, I, I, d, I, d, i, i]),
        "amgsetup_energy_block_row_product": (None, [I] * 4 + [i, i, d, d, d]),
        "amgsetup_energy_inner_product": (None, [I, I, i, d, d, d]),
        "amgsetup_truncate_rows_csr": (None, [I, I, i, i, d]),
        # independent sets, colourings and the CLJP splitting (graph.py, classical.py)
        "amgsetup_mis_serial": (I, [I, i, i, I, I, I, i]),
        "amgsetup_mis_parallel": (I, [I, i, i, I, I, I, i, d, I]),
        "amgsetup_mis_k_parallel": (I, [I, i, i, I, i, d, I]),
        "amgsetup_mis_aggregation": (I, [I, i, i, d, i, i, i]),
        "amgsetup_vertex_coloring_mis": (I, [I, i, i, i]),
        "amgsetup_vertex_coloring_first_fit": (None, [I, i, i, i, I]),
        "amgsetup_vertex_coloring_jones_plassmann": (I, [I, i, i, i, d]),
        "amgsetup_vertex_coloring_LDF": (I, [I, i, i, i, d]),
        "amgsetup_cljp_weights": (None, [I, i, i, I, d]),
        "amgsetup_cljp_random": (None, [I, d]),
        "amgsetup_cljp_select": (I, [I, i, i, i, i, d, i]),
        "amgsetup_cljp_naive_splitting": (None, [I, i, i, i, i, i, I]),
        # the classical setup (classical.py)
        "amgsetup_classical_strength": (I, [I, D, i, i, d, i, i, d]),
        "amgsetup_rs_cf_splitting": (None, [I, i, i, i, i, i]),
        "amgsetup_rs_direct_interpolation_pass1": (I, [I, i, i, i, i]),
        "amgsetup_rs_direct_interpolation_pass2": (None, [I, i, i, d, i, i, d, i, i, i, d]),
        "amgsetup_extended_interpolation_count": (I, [I, i, i, i, i]),
        "amgsetup_extended_interpolation_fill": (None, [I, i, i, d, i, i, i, i, i, d]),
        "amgsetup_truncate_interpolation": (I, [I, I, i, i, d, i, i, d]),
        # the thread team
        "amgsetup_num_threads": (I, []),
        "amgsetup_set_num_threads": (None, [I]),
    }
    for suffix in ("f32", "c64", "c128"):
        v = VALUE_CTYPES[suffix][0]
        sig["amgsetup_extract_subblocks_" + suffix] = (None, [i, i, v, v, i, i, i, I, I])
    return sig


def host_lib():
    global _loaded
    if _loaded is None:
        path = os.path.join(HERE, "lib", "libamgsetup_host.so")
        if not os.path.exists(path):
            raise ImportError("%s missing: run `make -C pyamg_amd/csrc`" % path)
        L = C.CDLL(path)
        for name, (restype, argtypes) in _signatures().items():
            f = getattr(L, name)
            f.restype = restype
            f.argtypes = argtypes
        # Row-parallel setup kernels keep O(columns) scratch per thread: cap the team at the CPUs this
        # process may use (launchers such as torchrun export OMP_NUM_THREADS=1; a bare run on a big
        # host would otherwise start hundreds of threads).  AMG_SETUP_THREADS overrides.
        try:
            avail = len(os.sched_getaffinity(0))
        except AttributeError:
            avail = os.cpu_count() or 1
        want = int(os.environ.get("AMG_SETUP_THREADS", min(32, avail)))
        L.amgsetup_set_num_threads(max(1, want))
        _loaded = L
    return _loaded


def lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def i32(a):
    return np.ascontiguousarray(a, dtype=np.intc)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def outside(what):
    return NotImplementedError("%s is outside the restated setup" % what)


def device_present():
    return _lib.device_count() > 0


def route(device, auto):
    """True: the device entry, its refusals raised.  None: the device entry, its refusals answered by the host route.
    False: the host route.  auto: what the calling stage decided for device=None when a GPU is present; the library is
    only asked for one when that is true."""
    if device is None:
        return None if (auto and device_present()) else False
    return bool(device)


def attempt(way, on_device, on_host, refusals=(NotImplementedError,)):
    """on_device() where way (what route returned) allows it; one of refusals from it is raised under True and answered
    by on_host() under None"""
    if way is not False:
        try:
            return on_device()
        except refusals:
            if way is True:
                raise
    return on_host()
