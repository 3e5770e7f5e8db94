"""ctypes binding of libamgcore_hip.so (include/amgcore_hip.h).

The HIP library is the product: there is no CPU fallback.  If the shared
object is missing, import fails loudly; if no GPU is present every compute
call raises ``AmgDeviceError``.
"""
import ctypes as C
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMGCORE_HIP_LIB") or os.path.join(HERE, "lib", "libamgcore_hip.so")   # env: A/B builds

c_int_p = C.POINTER(C.c_int)
c_dbl_p = C.POINTER(C.c_double)

AMG_OK, AMG_EINVAL, AMG_ENODEV, AMG_ENOMEM, AMG_ESTATE, AMG_ENOTIMPL = 0, -1, -2, -3, -4, -5


class AmgError(RuntimeError):
    pass


class AmgDeviceError(AmgError):
    pass


RELAX_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
COARSE_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, c_dbl_p, c_dbl_p)


class SmootherDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("iterations", C.c_int), ("sweep", C.c_int),
                ("omega", C.c_double), ("ncoef", C.c_int), ("coef", c_dbl_p),
                ("blocksize", C.c_int), ("Dinv", c_dbl_p), ("indices", c_int_p),
                ("nindices", C.c_int),
                ("Sj", c_int_p), ("Sp", c_int_p), ("Tp", c_int_p), ("Tx", c_dbl_p), ("nsdomains", C.c_int)]


# include/amgcore_hip.h section 5: resident hierarchies of other value types (complex128)
AMG_VALUE_F64, AMG_VALUE_F32, AMG_VALUE_C64, AMG_VALUE_C128 = 0, 1, 2, 3
COARSE_CALLBACK_X = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)


class SmootherDescX(C.Structure):
    _fields_ = [("kind", C.c_int), ("iterations", C.c_int), ("sweep", C.c_int), ("omega", C.c_void_p),
                ("ncoef", C.c_int), ("coef", c_dbl_p), ("blocksize", C.c_int), ("Dinv", C.c_void_p)]


# The flat amg_core table (include/amgcore_hip.h section 1): each entry's arguments in the SWIG call order.
# "I" int32 array, "V" value array, "i" int, "F" real scalar (the real type of the values); a `sized` entry
# passes every array followed by its length, as the C++ prototypes of amg_core do.
FLAT_TABLE = {
    "gauss_seidel": ("IIVVViii", True),
    "bsr_gauss_seidel": ("IIVVViiii", True),
    "jacobi": ("IIVVVViiiV", True),
    "bsr_jacobi": ("IIVVVViiiiV", True),
    "gauss_seidel_indexed": ("IIVVVIiii", True),
    "jacobi_ne": ("IIVVVVViiiV", True),
    "overlapping_schwarz_csr": ("IIVVVVIIIiiiii", True),
    "gauss_seidel_ne": ("IIVVViiiVF", True),
    "gauss_seidel_nr": ("IIVVViiiVF", True),
    "block_jacobi": ("IIVVVVViiiVi", True),
    "block_gauss_seidel": ("IIVVVViiii", True),
    "csr_matvec": ("iiIIVVV", False),
    "bsr_matvec": ("iiiiIIVVV", False),
    # amg_core/evolution_strength.h (csrc/strength.hip)
    "incomplete_mat_mult_csr": ("IIVIIVIIVi", True),
    "apply_distance_filter": ("iFIIV", True),
    "apply_absolute_distance_filter": ("iFIIV", True),
    "min_blocks": ("iiVV", True),
    # amg_core/smoothed_aggregation.h, the helpers of energy smoothing (csrc/energy.hip)
    "incomplete_mat_mult_bsr": ("IIVIIVIIViiiii", True),
    "satisfy_constraints_helper": ("iiiiVVVIIV", True),
    "calc_BtB": ("iiiViVII", True),
    "truncate_rows_csr": ("iiIIV", True),
    # amg_core/ruge_stuben.h, the row-parallel stages of the classical setup (csrc/classical.hip)
    "classical_strength_of_connection": ("iFIIVIIV", True),
    "maximum_row_value": ("iVIIV", True),
    "rs_direct_interpolation_pass1": ("iIIII", True),
    "rs_direct_interpolation_pass2": ("iIIVIIVIIIV", True),
}
# entries whose values are float64 only: another value dtype is the table's overload error
FLAT_F64_ONLY = frozenset(["incomplete_mat_mult_csr", "apply_distance_filter", "apply_absolute_distance_filter",
                           "min_blocks", "incomplete_mat_mult_bsr", "satisfy_constraints_helper", "calc_BtB",
                           "truncate_rows_csr", "classical_strength_of_connection", "maximum_row_value",
                           "rs_direct_interpolation_pass1", "rs_direct_interpolation_pass2"])
# value dtype -> symbol suffix, and per suffix the C types of a value pointer and of the real scalar F
VALUE_SUFFIX = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32",
                np.dtype(np.complex64): "c64", np.dtype(np.complex128): "c128"}
VALUE_CTYPES = {"f64": (c_dbl_p, C.c_double), "f32": (C.POINTER(C.c_float), C.c_float),
                "c64": (C.c_void_p, C.c_float), "c128": (C.c_void_p, C.c_double)}


def flat_argtypes(kinds, sized, suffix):
    vptr, real = VALUE_CTYPES[suffix]
    out = []
    for k in kinds:
        if k in "IV":
            out.append(c_int_p if k == "I" else vptr)
            if sized:
                out.append(C.c_int)
        else:
            out.append(C.c_int if k == "i" else real)
    return out


def build_library():
    """Compile the HIP sources in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "csrc")], check=True)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pyamg_amd: %s is missing -- build it with `make -C pyamg_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    # When PyTorch is present, load it first: torch ships its own libamdhip64 and both libraries
    # must share ONE HIP runtime in the process (the multi-GPU driver hands torch tensors to the
    # kernels); loaded in the other order torch finds "No HIP GPUs".
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    I, D, V = C.c_int, C.c_double, C.c_void_p
    sig = {
        "amgcore_norm2_f64": [c_dbl_p, C.c_long, c_dbl_p],
        "amg_hier_set_matrix": [V, I, I, I, I, I, I, I, V, V, V, I],
        "amg_hier_set_smoother": [V, I, I, C.POINTER(SmootherDesc)],
        "amg_hier_set_block_matrix": [V, I, I, I, I, c_int_p, c_int_p, c_dbl_p],
        "amg_hier_set_aux_matrix": [V, I, I, I, I, I, c_int_p, c_int_p, c_dbl_p],
        "amg_hier_set_coarse_dense": [V, c_dbl_p, I],
        "amg_hier_set_coarse_smoother": [V, C.POINTER(SmootherDesc)],
        "amg_hier_finalize": [V],
        "amg_hier_solve": [V, V, V, D, I, I, c_dbl_p, c_int_p, I],
        "amg_hier_cycle": [V, V, V, I, I],
        "amg_hier_pcg": [V, V, V, D, I, I, c_dbl_p, c_int_p, c_int_p, I],
        "amg_hier_relax": [V, I, I, c_dbl_p, c_dbl_p],
        "amg_hier_block_info": [V, I, I, V, I],
        "amg_hier_matvec": [V, I, I, c_dbl_p, c_dbl_p],
        "amg_hier_time_spmv": [V, I, I, I, I, c_dbl_p],
        "amg_hier_time_relax": [V, I, I, I, c_dbl_p],
        "amg_mat_apply": [V, I, V, V, V, V, V, D, D, V],
        "amg_mat_apply_rows": [V, I, I, I, V, V, V, V, V, D, D, V],
        "amg_dev_axpy_scaled": [V, V, D, C.c_long, V],
        "amg_mat_build_gs": [V, c_int_p, I],
        "amg_mat_gs_sweep": [V, V, V, I, I, V],
        "amg_mat_gs_sweeps": [V, V, V, V, I, I, V],
        "amg_dev_scale": [V, V, D, C.c_long, V],
        "amg_dev_axpy": [V, V, C.c_long, V],
        "amg_dev_norm2": [V, C.c_long, V, V, V],
        "amg_dev_dot": [V, V, C.c_long, V, V, V],
        "amg_dev_dense_apply": [V, V, V, I, V],
        "amg_dev_gather": [V, V, V, C.c_long, V],
        "amg_hier_set_callback_smoother": [V, I, I, RELAX_CALLBACK, V],
        "amg_hier_set_coarse_callback": [V, COARSE_CALLBACK, V],
        "amg_hier_apply": [V, I, I, V, V],
        "amg_hier_apply_aux": [V, I, I, I, V, V],
        "amg_dev_copy": [V, V, C.c_long, I, V],
        "amg_dev_fill": [V, D, C.c_long, V],
        "amg_dev_axmy": [V, V, D, C.c_long, V],
        "amg_dev_scale_add": [V, D, V, C.c_long, V],
        "amg_dev_sub": [V, V, V, C.c_long, V],
        "amg_dev_divide": [V, D, C.c_long, V],
        "amg_dev_dot_host": [V, V, C.c_long, V, C.POINTER(C.c_double), V],
        "amg_dev_norm_host": [V, C.c_long, V, C.POINTER(C.c_double), V],
        "amg_comm_add_channel": [V, c_int_p],
        "amg_comm_commit": [V, V],
        "amg_comm_connect": [V, V],
        "amg_comm_rccl_unique_id": [C.c_char_p, V],
        "amg_comm_rccl_init": [V, C.c_char_p, V],
        "amg_comm_exchange": [V, I, V, V, V, V],
        "amg_comm_allreduce_sqrt": [V, I, V, V, V],
        "amg_comm_check": [V],
        "amg_hier_set_comm": [V, V, I],
        "amg_hier_set_partition": [V, I, I, I, I, c_int_p, I, I],
        "amg_hier_set_gather": [V, I, I, I],
        "amg_hier_set_coarse_gather": [V, I, I],
        "amg_hier_comm_check": [V],
        "amg_arnoldi": [V, I, c_dbl_p, c_dbl_p, I, D, c_dbl_p, c_int_p, c_int_p],
        "amg_arnoldi_combine": [V, c_dbl_p, I, c_dbl_p],
        "amg_hier_galerkin": [V, I, I, V, V, V, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_galerkin_fetch": [V, V, V],
        "amg_csr_matmat_device": [I, I, I, V, V, V, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_csr_matmat_device_c128": [I, I, I, V, V, V, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_galerkin_device_c128": [I, I, V, V, V, V, V, V, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_galerkin_fetch_c128": [V, V, V],
        "amg_spgemm_last_route": [c_int_p, I],
        "amg_evolution_strength_device": [I, V, V, V, V, D, D, I, I, V, C.POINTER(C.c_void_p), c_dbl_p],
        "amg_strength_fetch": [V, V, V],
        "amg_energy_smooth_device": [I, I, I, I, I, V, V, V, V, V, V, V, V, V, I, D, C.POINTER(C.c_void_p), c_int_p, V, c_dbl_p],
        "amg_energy_smooth_rootnode_device": [I, I, I, I, I, V, V, V, V, V, V, V, V, V, V, V, I, D, C.POINTER(C.c_void_p), c_int_p, V,
                                              c_dbl_p],
        "amg_energy_fetch": [V, V],
        "amg_mis_device": [I, V, V, V, I, I, I, V, c_int_p, c_dbl_p],
        "amg_cljp_device": [I, V, V, V, V, V, V, c_int_p, c_dbl_p],
        "amg_mis_k_device": [I, V, V, I, V, I, V, c_int_p, c_dbl_p],
        "amg_mis_aggregation_device": [I, V, V, V, V, V, c_int_p, c_int_p, c_dbl_p],
        "amg_symmetric_strength_device": [I, V, V, V, D, V, C.POINTER(C.c_void_p), c_dbl_p],
        "amg_symmetric_strength_fetch": [V, V, V, c_dbl_p],
        "amg_fit_candidates_device": [I, I, I, I, V, V, V, D, V, V, c_dbl_p],
        "amg_jacobi_prolongation_device": [I, I, V, V, V, V, D, I, V, V, V, V, C.POINTER(C.c_void_p), c_dbl_p],
        "amg_jacobi_prolongation_fetch": [V, V, V, c_dbl_p],
        "amg_classical_level_device": [I, V, V, V, D, I, I, V, C.POINTER(C.c_void_p), C.POINTER(C.c_long), c_int_p, c_dbl_p],
        "amg_classical_level_fetch": [V, V, V, V, V, V, V, V, c_dbl_p],
        "amg_classical_level_build": [I, V, V, V, D, I, I, V, I, I, C.POINTER(C.c_void_p), C.POINTER(C.c_long), c_int_p, c_dbl_p],
        "amg_csr_transpose_device": [I, I, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_csr_transpose_fetch": [V, V, V],
        "amg_transpose_last_route": [c_int_p, I],
        "amg_classical_chain_begin": [I, V, V, V, I, C.POINTER(C.c_void_p)],
        "amg_classical_chain_level": [V, D, I, V, I, I, C.POINTER(C.c_long), c_int_p, c_int_p, c_dbl_p],
        "amg_classical_chain_fetch": [V] * 14 + [c_dbl_p],
        "amg_sa_chain_begin": [I, V, V, V, V, C.POINTER(C.c_void_p)],
        "amg_sa_chain_level": [V, I, D, I, V, V, D, I, V, D, C.POINTER(C.c_long), c_int_p, c_int_p, c_dbl_p],
        "amg_sa_chain_fetch": [V] * 16 + [c_dbl_p],
        "amg_extended_interpolation_device": [I, V, V, V, V, V, V, I, V, C.POINTER(C.c_void_p), c_dbl_p],
        "amg_extended_interpolation_fetch": [V, V, V],
        "amg_hierx_create": [I, I, I, C.POINTER(C.c_void_p)],
        "amg_hierx_set_matrix": [V, I, I, I, I, I, I, I, V, V, V],
        "amg_hierx_set_smoother": [V, I, I, C.POINTER(SmootherDescX)],
        "amg_hierx_set_block_matrix": [V, I, I, I, I, V, V, V],
        "amg_hierx_set_coarse_dense": [V, V, I],
        "amg_hierx_set_coarse_callback": [V, COARSE_CALLBACK_X, V],
        "amg_hierx_finalize": [V],
        "amg_hierx_solve": [V, V, V, D, I, I, c_dbl_p, c_int_p, I],
        "amg_hierx_cycle": [V, V, V, I, I],
        "amg_hierx_apply": [V, I, V, V],
        "amg_hierx_norm": [V, V, C.c_long, C.POINTER(C.c_double)],
        "amg_devx_zdotc": [V, V, C.c_long, V, I, C.POINTER(C.c_double), V],
        "amg_devx_axpy": [V, V, D, D, C.c_long, V],
        "amg_devx_axpy_slot": [V, V, V, I, D, C.c_long, V],
        "amg_devx_xpby": [V, D, D, V, C.c_long, V],
        "amg_devx_scale": [V, V, D, D, C.c_long, V],
        "amg_devx_sub": [V, V, V, C.c_long, V],
        "amg_devx_fill": [V, D, D, C.c_long, V],
        "amg_devx_copy": [V, V, C.c_long, I, V],
        "amg_devx_householders": [V, C.POINTER(V), I, C.c_long, I, I, I, V, V],
        "amg_devx_horner": [V, C.POINTER(V), I, V, C.c_long, I, I, I, V, V],
        # section 6: several right-hand sides
        "amg_hierm_create": [I, I, I, C.POINTER(C.c_void_p)],
        "amg_hierm_set_matrix": [V, I, I, I, I, I, I, I, V, V, V],
        "amg_hierm_set_smoother": [V, I, I, C.POINTER(SmootherDesc)],
        "amg_hierm_set_coarse_dense": [V, c_dbl_p, I],
        "amg_hierm_set_coarse_smoother": [V, C.POINTER(SmootherDesc)],
        "amg_hierm_finalize": [V],
        "amg_hierm_solve": [V, I, V, V, D, I, I, c_dbl_p, c_int_p, I],
        "amg_hierm_cycle": [V, I, V, V, I, I],
    }
    for name, (kinds, sized) in FLAT_TABLE.items():
        for suffix in VALUE_SUFFIX.values():
            if name in FLAT_F64_ONLY and suffix != "f64":
                continue
            sig["amgcore_%s_%s" % (name, suffix)] = flat_argtypes(kinds, sized, suffix)
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = I
    L.amg_last_error.restype = C.c_char_p
    L.amg_device_count.restype = I
    if hasattr(L, "amg_dev_live_buffers"):     # (an older build named by AMGCORE_HIP_LIB for an A/B run has no counter)
        L.amg_dev_live_buffers.argtypes = []
        L.amg_dev_live_buffers.restype = C.c_long
    L.amg_device_name.argtypes = [I]
    L.amg_device_name.restype = C.c_char_p
    L.amg_classical_chain_free.argtypes = [V]
    L.amg_classical_chain_free.restype = None
    L.amg_sa_chain_free.argtypes = [V]
    L.amg_sa_chain_free.restype = None
    L.amg_hier_create.argtypes = [I, I]
    L.amg_hier_create.restype = V
    L.amg_hier_destroy.argtypes = [V]
    L.amg_hier_destroy.restype = None
    L.amg_hierx_destroy.argtypes = [V]
    L.amg_hierx_destroy.restype = None
    L.amg_hierx_device_bytes.argtypes = [V]
    L.amg_hierx_device_bytes.restype = C.c_long
    L.amg_hierx_last_solve_ms.argtypes = [V]
    L.amg_hierx_last_solve_ms.restype = D
    L.amg_hierx_stream.argtypes = [V]
    L.amg_hierx_stream.restype = V
    L.amg_hierx_scratch.argtypes = [V]
    L.amg_hierx_scratch.restype = V
    L.amg_hierx_level_size.argtypes = [V, I]
    L.amg_hierx_level_size.restype = I
    L.amg_hierx_vec_alloc.argtypes = [V, C.c_long]
    L.amg_hierx_vec_alloc.restype = V
    L.amg_hierx_vec_free.argtypes = [V, V, C.c_long]
    L.amg_hierx_vec_free.restype = None
    L.amg_hierm_destroy.argtypes = [V]
    L.amg_hierm_destroy.restype = None
    L.amg_hierm_device_bytes.argtypes = [V]
    L.amg_hierm_device_bytes.restype = C.c_long
    L.amg_hierm_last_solve_ms.argtypes = [V]
    L.amg_hierm_last_solve_ms.restype = D
    L.amg_hier_cycle_bytes.argtypes = [V, I]
    L.amg_hier_cycle_bytes.restype = D
    L.amg_hier_value_index.argtypes = [V, I, I]
    L.amg_hier_value_index.restype = I
    L.amg_set_value_index.argtypes = [I]
    L.amg_set_value_index.restype = None
    L.amg_set_level0_fusion.argtypes = [I]
    L.amg_set_level0_fusion.restype = None
    L.amg_hier_level0_fused.argtypes = [V]
    L.amg_hier_level0_fused.restype = I
    L.amg_set_level0_plane_reuse.argtypes = [I]
    L.amg_set_level0_plane_reuse.restype = None
    L.amg_hier_level0_plane_reuse.argtypes = [V]
    L.amg_hier_level0_plane_reuse.restype = I
    L.amg_set_level0_zero_slots.argtypes = [I]
    L.amg_set_level0_zero_slots.restype = None
    L.amg_value_index_enabled.argtypes = []
    L.amg_value_index_enabled.restype = I
    L.amg_hier_gs_natural.argtypes = [V, I, V, V, V, I]
    L.amg_hier_gs_natural.restype = I
    L.amg_hier_operator_form.argtypes = [V, I]
    L.amg_hier_operator_form.restype = I
    L.amg_hier_operator_bytes.argtypes = [V, I, I]
    L.amg_hier_operator_bytes.restype = D
    L.amg_hier_cycle_bytes_moved.argtypes = [V, I]
    L.amg_hier_cycle_bytes_moved.restype = D
    L.amg_hier_last_solve_ms.argtypes = [V]
    L.amg_hier_last_solve_ms.restype = D
    L.amg_hier_device_bytes.argtypes = [V]
    L.amg_hier_device_bytes.restype = C.c_long
    L.amg_hier_stream.argtypes = [V]
    L.amg_hier_stream.restype = V
    L.amg_hier_dev_x.argtypes = [V]
    L.amg_hier_dev_x.restype = V
    L.amg_hier_dev_b.argtypes = [V]
    L.amg_hier_dev_b.restype = V
    L.amg_dev_alloc.argtypes = [C.c_long]
    L.amg_dev_alloc.restype = V
    L.amg_dev_free.argtypes = [V]
    L.amg_dev_free.restype = None
    L.amg_hier_scratch.argtypes = [V]
    L.amg_hier_scratch.restype = V
    L.amg_comm_create.argtypes = [I, I, I, I]
    L.amg_comm_create.restype = V
    L.amg_comm_destroy.argtypes = [V]
    L.amg_comm_destroy.restype = None
    L.amg_hier_release_sources.argtypes = [V]
    L.amg_hier_release_sources.restype = C.c_long
    L.amg_mat_create.argtypes = [I, I, I, c_int_p, c_int_p, c_dbl_p]
    L.amg_mat_create.restype = V
    L.amg_mat_destroy.argtypes = [V]
    L.amg_mat_destroy.restype = None
    L.amg_mat_gs_levels.argtypes = [V]
    L.amg_mat_gs_levels.restype = I
    L.amg_mat_gs_info.argtypes = [V, V, I]
    L.amg_mat_gs_info.restype = I
    L.amg_mat_form.argtypes = [V]
    L.amg_mat_form.restype = I
    L.amg_mat_nnz.argtypes = [V]
    L.amg_mat_nnz.restype = C.c_long
    L.amg_mat_rows_per_block.argtypes = [V]
    L.amg_mat_rows_per_block.restype = I
    L.amg_mat_index16_fraction.argtypes = [V]
    L.amg_mat_index16_fraction.restype = C.c_double
    L.amg_arnoldi_free.argtypes = [V]
    L.amg_arnoldi_free.restype = None
    L.amg_set_stream_variant.argtypes = [I]
    L.amg_set_stream_variant.restype = None
    L.amg_set_stream_pipe.argtypes = [I]
    L.amg_set_stream_pipe.restype = None
    L.amg_hier_use_graphs.argtypes = [V, I]
    L.amg_hier_use_graphs.restype = None
    L.amg_hier_keep_residual.argtypes = [V, I]
    L.amg_hier_keep_residual.restype = None
    L.amg_set_tile_target.argtypes = [I]
    L.amg_set_tile_target.restype = None
    L.amg_set_index16.argtypes = [I]
    L.amg_set_index16.restype = None
    L.amg_set_bsr_spmv.argtypes = [I]
    L.amg_set_bsr_spmv.restype = None
    L.amg_set_gs_chain.argtypes = [I]
    L.amg_set_gs_chain.restype = None
    L.amg_set_gs_level_hint.argtypes = [I]
    L.amg_set_gs_level_hint.restype = None
    L.amg_set_gs_flow.argtypes = [I]
    L.amg_set_gs_flow.restype = None
    L.amg_set_gs_flow_lookahead.argtypes = [I]
    L.amg_set_gs_flow_lookahead.restype = None
    L.amg_gs_flow_status.argtypes = []
    L.amg_gs_flow_status.restype = I
    L.amg_set_stencil_form.argtypes = [I]
    L.amg_set_stencil_form.restype = None
    L.amg_set_stencil_pairs.argtypes = [I]
    L.amg_set_stencil_pairs.restype = None
    L.amg_set_sell_form.argtypes = [I]
    L.amg_set_sell_form.restype = None
    L.amg_set_sell_index16.argtypes = [I]
    L.amg_set_sell_index16.restype = None
    L.amg_set_xcd_period.argtypes = [I]
    L.amg_set_xcd_period.restype = None
    L.amg_set_xcd_chunk.argtypes = [I]
    L.amg_set_xcd_chunk.restype = None
    _lib = L
    return L


def check(rc):
    if rc == 0:
        return
    msg = lib().amg_last_error().decode("utf-8", "replace")
    if rc == AMG_ENODEV:
        raise AmgDeviceError(msg)
    if rc == AMG_ENOMEM:
        raise MemoryError(msg)
    if rc == AMG_ENOTIMPL:
        raise NotImplementedError(msg)
    if rc == AMG_EINVAL:
        raise ValueError(msg)
    raise AmgError(msg)


def ip(a):
    return a.ctypes.data_as(c_int_p)


def dp(a):
    return a.ctypes.data_as(c_dbl_p)


def allocate(specs):
    """One uninitialised array per (count or shape, dtype) of specs, None where specs holds None."""
    return [None if s is None else np.empty(s[0], dtype=s[1]) for s in specs]


def fetch_result(handle, fetch, specs, *tail):
    """The second call of a device stage: `fetch` (an amg_*_fetch entry) downloads the arrays the handle holds and
    releases it.  specs: the (count, dtype) of each array the entry takes, None for one that is not wanted; tail: what
    the entry takes after the arrays.  Where the host arrays cannot be allocated the entry is called with null arrays,
    which releases the result all the same, before the error goes on.  Returns (arrays, milliseconds of the fetch)."""
    try:
        arrays = allocate(specs)
    except BaseException:
        fetch(handle, *([None] * len(specs)), *tail)
        raise
    t0 = time.perf_counter()
    check(fetch(handle, *(None if a is None else a.ctypes.data for a in arrays), *tail))
    return arrays, (time.perf_counter() - t0) * 1e3


def device_count():
    return lib().amg_device_count()


def live_buffers():
    """Device allocations the library made and still holds (amg_dev_live_buffers)."""
    return lib().amg_dev_live_buffers()


SPGEMM_ROUTE_FIELDS = ("complex", "lanes_first", "lanes", "tables", "entries", "blocks", "second_tier_rows")
SPGEMM_TABLES = ("none", "lds", "hbm_wave", "hbm_thread", "refused")


def spgemm_last_route():
    """What this thread's most recent device product did (amg_spgemm_last_route, csrc/spgemm.hip): a dict of
    SPGEMM_ROUTE_FIELDS, `tables` as one of SPGEMM_TABLES."""
    out = (C.c_int * len(SPGEMM_ROUTE_FIELDS))()
    n = lib().amg_spgemm_last_route(out, len(SPGEMM_ROUTE_FIELDS))
    if n != len(SPGEMM_ROUTE_FIELDS):
        raise AmgError("amg_spgemm_last_route: %d fields, %d expected" % (n, len(SPGEMM_ROUTE_FIELDS)))
    rec = dict(zip(SPGEMM_ROUTE_FIELDS, (int(v) for v in out)))
    rec["tables"] = SPGEMM_TABLES[rec["tables"]]
    return rec


TRANSPOSE_ROUTE_FIELDS = ("launched", "lane_rows", "lds_rows", "hbm_rows")
# a row of R of at most TRANSPOSE_LANE_MAX entries is ordered by one lane, of at most TRANSPOSE_LDS_MAX by one wave in LDS,
# a longer one by one workgroup in HBM (TR_LANE_MAX, TR_LDS_MAX of csrc/transpose.hip)
TRANSPOSE_LANE_MAX, TRANSPOSE_LDS_MAX = 32, 2048
CHAIN_PRODUCT_REFUSED = 1
CHAIN_FLAG_FIELDS = 8
# amg_sa_chain_level: the fields of its flags, its strength modes and why a level stopped (include/amgcore_hip.h)
SA_CHAIN_FLAG_FIELDS = 10
SA_STRENGTH_CSR, SA_STRENGTH_SQUARED, SA_STRENGTH_ONES = 0, 1, 2
SA_NO_AGGREGATE, SA_SMOOTHING_REFUSED = 1, 2


def transpose_last_route():
    """What this thread's most recent device transpose did (amg_transpose_last_route, csrc/transpose.hip): a dict of
    TRANSPOSE_ROUTE_FIELDS."""
    out = (C.c_int * len(TRANSPOSE_ROUTE_FIELDS))()
    n = lib().amg_transpose_last_route(out, len(TRANSPOSE_ROUTE_FIELDS))
    if n != len(TRANSPOSE_ROUTE_FIELDS):
        raise AmgError("amg_transpose_last_route: %d fields, %d expected" % (n, len(TRANSPOSE_ROUTE_FIELDS)))
    return dict(zip(TRANSPOSE_ROUTE_FIELDS, (int(v) for v in out)))
