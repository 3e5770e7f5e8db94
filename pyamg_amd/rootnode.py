"""Root-node smoothed aggregation (pyamg/aggregation/rootnode.py) on the CPU, restated as aggregation.py restates SA.

Root-node SA keeps the prolongator at the identity on one root node per aggregate, so that the coarse candidates are the
fine candidates injected at the roots, and leaves the rest to energy minimisation (smooth.py) with the root-node rules.
The setup differs from SA in its order: the candidates are improved AFTER strength and aggregation.

Supported subset (anything else raises NotImplementedError before any level is built):
  strength   'symmetric' | 'evolution' / 'ode' (one candidate) | None | ('predefined', {'C': csr})
  aggregate  'standard' | 'mis' / ('mis', {'device'}) (the roots of the MIS(2) aggregation are the root nodes) |
             ('predefined', {'AggOp': csr, 'Cnodes': array})
  smooth     'energy' / ('energy', {'krylov': 'cg', 'maxiter', 'tol', 'degree', 'weighting': 'local' | 'diagonal',
             'prefilter', 'postfilter', 'device'}) | None
  symmetry   'hermitian' | 'symmetric', real operators
"""
import numpy as np
from scipy.sparse import bsr_matrix, csr_matrix, isspmatrix_bsr, isspmatrix_csr

from ._host import outside as _outside
from .aggregation import (_improve, _levelize_sa, _levelize_smooth, blocksize, fit_candidates, mis_aggregation,
                          standard_aggregation, symmetric_strength_of_connection, unpack_arg)
from .multilevel import multilevel_solver
from .smooth import energy_prolongation_smoother
from .smoothing import change_smoothers
from .util import get_Cpt_params, scale_T

__all__ = ["rootnode_solver"]

_STRENGTH = ("symmetric", "evolution", "ode", "predefined", None)
_AGGREGATE = ("standard", "mis", "predefined")
_SMOOTH = ("energy", None)


def _check_options(strength, aggregate, smooth):
    """every per-level descriptor against the supported subset, before any level is built"""
    for desc in strength:
        fn, _ = unpack_arg(desc)
        if fn not in _STRENGTH:
            raise _outside("strength=%r" % (fn,))
    for desc in aggregate:
        fn, kw = unpack_arg(desc)
        if fn not in _AGGREGATE:
            raise _outside("aggregate=%r" % (fn,))
        if fn == "predefined" and not ("AggOp" in kw and "Cnodes" in kw):
            raise ValueError("a predefined aggregation of the root-node solver needs 'AggOp' and 'Cnodes'")
    for desc in smooth:
        fn, kw = unpack_arg(desc)
        if fn not in _SMOOTH:
            raise _outside("smooth=%r" % (fn,))
        if fn == "energy" and kw.get("krylov", "cg") != "cg":
            raise _outside("energy smoothing with krylov=%r" % (kw.get("krylov"),))
        if fn == "energy" and kw.get("weighting", "local") == "block":
            raise _outside("energy smoothing with weighting='block'")


def rootnode_solver(A, B=None, BH=None, symmetry="hermitian", strength="symmetric", aggregate="standard", smooth="energy",
                    presmoother=("block_gauss_seidel", {"sweep": "symmetric"}),
                    postsmoother=("block_gauss_seidel", {"sweep": "symmetric"}),
                    improve_candidates=[("block_gauss_seidel", {"sweep": "symmetric", "iterations": 4}), None],
                    max_levels=10, max_coarse=500, diagonal_dominance=False, keep=False, **kwargs):
    """Create a multilevel solver using root-node smoothed aggregation (pyamg/aggregation/rootnode.py:33-313);
    returns a pyamg_amd.multilevel_solver.

    A : csr_matrix or bsr_matrix with square blocks, real.  B : the near-nullspace candidates, at least blocksize(A)
    columns (default: the constant of every block variable).  smooth='energy' means CG energy minimisation with
    maxiter 4, tol 1e-8, degree 1 and 'local' weighting.  Every level keeps its root dofs in level.Cpts; with keep=True
    also C, AggOp, T, Fpts, P_I, I_F and I_C."""
    if not (isspmatrix_csr(A) or isspmatrix_bsr(A)):
        try:
            A = csr_matrix(A)
        except Exception:
            raise TypeError("Argument A must have type csr_matrix or bsr_matrix, or be convertible to csr_matrix")
    if symmetry not in ("symmetric", "hermitian", "nonsymmetric"):
        raise ValueError("expected 'symmetric', 'nonsymmetric' or 'hermitian' for the symmetry parameter")
    if symmetry == "nonsymmetric":
        raise _outside("symmetry='nonsymmetric'")
    if A.dtype.kind == "c" or (B is not None and np.iscomplexobj(B)):
        raise _outside("root-node setup of a complex operator")
    if unpack_arg(diagonal_dominance)[0]:
        raise _outside("diagonal_dominance")
    A = A.astype(np.float64) if A.dtype != np.float64 else A
    if A.shape[0] != A.shape[1]:
        raise ValueError("expected square matrix")
    if isspmatrix_bsr(A) and A.blocksize[0] != A.blocksize[1]:
        raise ValueError("expected square blocks")
    A.symmetry = symmetry
    bs = blocksize(A)
    if B is None:
        B = np.kron(np.ones((A.shape[0] // bs, 1), dtype=A.dtype), np.eye(bs))
    else:
        B = np.asarray(B, dtype=A.dtype)
        if len(B.shape) == 1:
            B = B.reshape(-1, 1)
        if B.shape[0] != A.shape[0]:
            raise ValueError("The near null-space modes B have incorrect dimensions for matrix A")
        if B.shape[1] < bs:
            raise ValueError("B.shape[1] must be >= the blocksize of A")

    max_levels, max_coarse, strength = _levelize_sa(strength, max_levels, max_coarse)
    max_levels, max_coarse, aggregate = _levelize_sa(aggregate, max_levels, max_coarse)
    improve_candidates = _levelize_smooth(list(improve_candidates) if isinstance(improve_candidates, list)
                                          else improve_candidates, max_levels)
    smooth = _levelize_smooth(smooth, max_levels)
    _check_options(strength, aggregate, smooth)

    levels = [multilevel_solver.level()]
    levels[-1].A = A
    levels[-1].B = B
    while len(levels) < max_levels and int(levels[-1].A.shape[0] / blocksize(levels[-1].A)) > max_coarse:
        extend_hierarchy(levels, strength, aggregate, smooth, improve_candidates, keep)
    ml = multilevel_solver(levels, **kwargs)
    change_smoothers(ml, presmoother, postsmoother)
    return ml


def extend_hierarchy(levels, strength, aggregate, smooth, improve_candidates, keep=True):
    """rootnode.py:316-470, in the reference's order: strength on the un-improved candidates, aggregation, candidate
    improvement, tentative prolongator from the first blocksize candidates, root-node operators, scaling, injected
    coarse candidates, energy smoothing, restriction, Galerkin product."""
    A = levels[-1].A
    B = levels[-1].B
    li = len(levels) - 1
    bs = blocksize(A)

    fn, kwargs = unpack_arg(strength[li])
    if fn == "symmetric":
        Cm = symmetric_strength_of_connection(A, **kwargs)
    elif fn in ("ode", "evolution"):
        from .strength import evolution_strength_of_connection
        Cm = evolution_strength_of_connection(A, **kwargs) if "B" in kwargs else evolution_strength_of_connection(A, B, **kwargs)
    elif fn == "predefined":
        Cm = kwargs["C"].tocsr()
    elif fn is None:
        Cm = A.tocsr()
    else:
        raise _outside("strength=%r" % (fn,))

    fn, kwargs = unpack_arg(aggregate[li])
    if fn == "standard":
        AggOp, Cnodes = standard_aggregation(Cm, **kwargs)
    elif fn == "mis":
        AggOp, Cnodes = mis_aggregation(Cm, **kwargs)
    elif fn == "predefined":
        AggOp, Cnodes = kwargs["AggOp"].tocsr(), np.asarray(kwargs["Cnodes"])
    else:
        raise _outside("aggregate=%r" % (fn,))

    fn, kwargs = unpack_arg(improve_candidates[li])
    if fn is not None:
        B = _improve((fn, kwargs), A, B)
        levels[-1].B = B

    T, _ = fit_candidates(AggOp, B[:, :bs])
    params = get_Cpt_params(A, Cnodes, AggOp, T)
    T = scale_T(T, params["P_I"], params["I_F"])
    Bc = params["P_I"].T * B                # the coarse candidates: the fine ones injected at the roots, all columns

    fn, kwargs = unpack_arg(smooth[li])
    if fn == "energy":
        P = energy_prolongation_smoother(A, T, Cm, Bc, B, (True, params), **kwargs)
    elif fn is None:
        P = T
    else:
        raise _outside("smooth=%r" % (fn,))

    symmetry = A.symmetry
    R = P.conj().T.asformat(P.format) if symmetry == "hermitian" else P.T.asformat(P.format)
    if keep:
        levels[-1].C = Cm
        levels[-1].AggOp = AggOp
        levels[-1].T = T
        levels[-1].Fpts = params["Fpts"]
        levels[-1].P_I = params["P_I"]
        levels[-1].I_F = params["I_F"]
        levels[-1].I_C = params["I_C"]
    levels[-1].P = P
    levels[-1].R = R
    levels[-1].Cpts = params["Cpts"]

    levels.append(multilevel_solver.level())
    A = R * A * P
    A.symmetry = symmetry
    levels[-1].A = A
    levels[-1].B = Bc
