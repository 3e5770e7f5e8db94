"""Generic AMG solver -- the ``multilevel_solver`` object API of the reference
(pyamg/multilevel.py) with the solve phase running on MI355X.

The object keeps the reference's attributes (``levels[i].A/P/R``,
``presmoother``/``postsmoother`` closures, ``coarse_solver``) as host-side
scipy matrices -- that is how setup code builds and inspects a hierarchy --
and mirrors them ONCE into HBM (operators, smoother constants, work vectors)
the first time ``solve`` runs.  ``solve``/``aspreconditioner`` then execute
multilevel.py:316-548 entirely on the device through libamgcore_hip.so.
"""
from warnings import warn

import os

import numpy as np
import scipy.linalg
import scipy.sparse as sparse

from . import _lib

__all__ = ["multilevel_solver", "coarse_grid_solver"]

_SM_KIND = {None: 0, "None": 0, "jacobi": 1, "gauss_seidel": 2, "sor": 3, "polynomial": 4,
            "block_jacobi": 5, "block_gauss_seidel": 6, "gauss_seidel_indexed": 7, "schwarz": 8,
            "gauss_seidel_ne": 9, "gauss_seidel_nr": 10, "jacobi_ne": 11}
# The kinds of every engine: the complex128 and the multi-RHS engine implement the subsets _C128_KIND and _MULTI_KIND
# under the same numbers.  (name "krylov": a callback smoother of the float64 mirror, _set_krylov_smoother)
_SWEEP = {"forward": 0, "backward": 1, "symmetric": 2}
_CYCLE = {"V": 0, "W": 1, "F": 2, "AMLI": 3}
_X0_ZERO, _NO_EARLY_STOP, _DEVICE_VECTORS = 1, 2, 4


def _cycle_name(cycle):
    cycle = str(cycle).upper()
    if cycle not in _CYCLE:
        raise TypeError("Unrecognized cycle type (%s)" % cycle)
    return cycle


def _flags(x0_zero=False, fixed=False, device_vectors=False):
    return (_X0_ZERO if x0_zero else 0) | (_NO_EARLY_STOP if fixed else 0) | (_DEVICE_VECTORS if device_vectors else 0)


def _is_own_krylov(accel):
    """is accel one of pyamg_amd.krylov's own methods, named or passed as the function itself?"""
    from . import krylov
    name = accel if isinstance(accel, str) else getattr(accel, "__name__", None)
    return name in krylov.METHODS and (isinstance(accel, str) or accel is krylov.METHODS[name])


def _desc_struct(desc, keep, struct=_lib.SmootherDesc):
    """descriptor dict (smoothing.py closures' .desc) -> amg_smoother_desc, or amg_smoother_desc_x (struct =
    SmootherDescX), whose omega and Dinv are complex128 arrays passed by address; keep receives the arrays the
    struct points to"""
    d = struct()
    cplx = struct is _lib.SmootherDescX
    name = None if desc is None else desc.get("name")
    if name not in _SM_KIND:
        raise NotImplementedError("smoother %r has no device implementation" % (name,))
    d.kind = _SM_KIND[name]
    if d.kind == 0:
        return d
    d.iterations = int(desc.get("iterations", 1))
    sweep = desc.get("sweep", "forward")
    if sweep not in _SWEEP:
        raise ValueError("valid sweep directions are 'forward', 'backward', and 'symmetric'")
    d.sweep = _SWEEP[sweep]
    co = desc.get("coefficients")
    if cplx:
        omega = np.array([desc.get("omega", 1.0)], dtype=np.complex128)     # type_prep(A.dtype, [omega])
        keep.append(omega)
        d.omega = omega.ctypes.data
        co = [0.0] if co is None else co
    else:
        d.omega = float(desc.get("omega", 1.0))
    if co is not None:
        co = np.ascontiguousarray(co, dtype=np.float64)
        keep.append(co)
        d.ncoef, d.coef = len(co), _lib.dp(co)
    d.blocksize = int(desc.get("blocksize", 1) or 1)
    if desc.get("Dinv") is not None:
        Dinv = np.ascontiguousarray(np.ravel(desc["Dinv"]), dtype=np.complex128 if cplx else np.float64)
        keep.append(Dinv)
        d.Dinv = Dinv.ctypes.data if cplx else _lib.dp(Dinv)
    if cplx:
        return d                # the complex128 engine has no indexed or Schwarz smoother
    if desc.get("indices") is not None:
        idx = np.ascontiguousarray(desc["indices"], dtype=np.intc)
        keep.append(idx)
        d.indices, d.nindices = _lib.ip(idx), len(idx)
    if name == "schwarz":
        arrs = [np.ascontiguousarray(desc[k], dtype=np.intc) for k in ("subdomain", "subdomain_ptr", "inv_subblock_ptr")]
        Tx = np.ascontiguousarray(desc["inv_subblock"], dtype=np.float64)
        keep.extend(arrs + [Tx])
        d.Sj, d.Sp, d.Tp, d.Tx = _lib.ip(arrs[0]), _lib.ip(arrs[1]), _lib.ip(arrs[2]), _lib.dp(Tx)
        d.nsdomains = len(arrs[1]) - 1
    return d


_C128_KIND = {None: 0, "None": 0, "jacobi": 1, "gauss_seidel": 2, "sor": 3, "polynomial": 4, "block_jacobi": 5,
              "block_gauss_seidel": 6}


_SCIPY_ONLY_COARSE = ("cgs", "qmr", "minres", "bicg")     # coarse Krylov names run by scipy on complex128 vectors


class _ResidentHierarchy(object):
    """What the mirrors of the three resident engines share: the handle's lifetime, the descriptor of a smoother, the
    order in which a hierarchy goes into the engine, and the calls that cycle on one vector.  A mirror names its
    engine's entries (_PREFIX), its value type, its smoother kinds and its refusals, and adds to _set_smoother(lvl,
    which, fn, A) (which = 2: the coarse solver of the last level; A: the level's operator, for a smoother that needs
    it in another form) and to the forms of coarse solver (_COARSE) what only its engine has."""
    _PREFIX = None          # of the engine's entries: amg_hier_, amg_hierx_ or amg_hierm_
    _DTYPE = None           # of the operators' values
    _DESC = _lib.SmootherDesc       # the engine's smoother descriptor, which _desc_struct fills
    _KIND = None            # smoother name -> the engine's kind
    _NO_SMOOTHER = None     # the refusal of any other smoother (% its name)
    _NO_COARSE = "coarse solver %s has no device implementation"    # a form that is not in _COARSE (% the solver's name)
    _COARSE_CALLBACK = None     # the ctypes type of a coarse solver callback, where the engine takes one

    def _fn(self, name):
        return getattr(self.L, self._PREFIX + name)

    def _open(self, ml, coarse, *create):
        """makes the handle (create: the arguments of the engine's create entry) and builds the hierarchy into it
        (coarse: what check_levels returned, where the mirror has one); the handle is closed again if that fails"""
        self.L = _lib.lib()
        self.n = ml.levels[0].A.shape[0]
        self._keep = []                  # what the descriptors point to, until the engine has taken it
        self._callbacks = []             # ctypes callbacks must outlive the hierarchy
        self._callback_error = None
        self.h = self._create(*create)
        try:
            self._build(ml, coarse)
        except Exception:
            self.close()
            raise
        self._keep = []

    def _create(self, *args):
        h = _lib.C.c_void_p()
        _lib.check(self._fn("create")(*args, _lib.C.byref(h)))
        return h.value

    @classmethod
    def _desc_of(cls, lvl, fn):
        desc = getattr(fn, "desc", None)
        if fn is not None and desc is None:
            raise NotImplementedError(
                "level %d: smoother %r carries no device descriptor; use pyamg_amd.smoothing."
                "change_smoothers with one of the device smoothers" % (lvl, fn))
        name = None if desc is None else desc.get("name")
        if name not in cls._KIND:
            raise NotImplementedError(cls._NO_SMOOTHER % (name,))
        return desc

    @staticmethod
    def _pattern(M):
        """a BSR operator as it is, any other as CSR: (fmt, M, indptr, indices), the index arrays as C ints"""
        fmt = 1 if sparse.isspmatrix_bsr(M) else 0
        if not fmt:
            M = sparse.csr_matrix(M)
        return fmt, M, np.ascontiguousarray(M.indptr, dtype=np.intc), np.ascontiguousarray(M.indices, dtype=np.intc)

    def _set_matrix(self, lvl, which, M, *more):
        fmt, M, Ap, Aj = self._pattern(M)
        R, C = M.blocksize if fmt else (1, 1)
        # a real P / R of a complex hierarchy: astype(complex128), as scipy converts it inside a mixed product
        data = np.ascontiguousarray(np.ravel(M.data), dtype=self._DTYPE)
        _lib.check(self._fn("set_matrix")(self.h, lvl, which, fmt, M.shape[0], M.shape[1], R, C,
                                          Ap.ctypes.data, Aj.ctypes.data, data.ctypes.data, *more))

    def _set_smoother(self, lvl, which, fn, A):
        d = _desc_struct(self._desc_of(lvl, fn), self._keep, self._DESC)
        self._set_desc(lvl, which, d)
        if d.kind in (5, 6):
            # the block smoothers sweep A in blocks of their own size (relaxation.py:471,563)
            bs = d.blocksize
            if not (sparse.isspmatrix_bsr(A) and A.blocksize == (bs, bs)):
                _, Ab, Ap, Aj = self._pattern(A.tobsr(blocksize=(bs, bs)))
                Ax = np.ascontiguousarray(np.ravel(Ab.data), dtype=self._DTYPE)
                _lib.check(self._fn("set_block_matrix")(self.h, lvl, which, Ab.shape[0] // bs, bs,
                                                        _lib.ip(Ap), _lib.ip(Aj), _lib.dp(Ax)))
        return d

    def _set_desc(self, lvl, which, d):
        if which == 2:
            _lib.check(self._fn("set_coarse_smoother")(self.h, d))
        else:
            _lib.check(self._fn("set_smoother")(self.h, lvl, which, d))

    def _set_coarse_dense(self, M, Ac):         # Ac: only the callback form needs it
        M = np.ascontiguousarray(M, dtype=self._DTYPE)
        _lib.check(self._fn("set_coarse_dense")(self.h, _lib.dp(M), M.shape[0]))

    def _set_coarse_callback(self, fn, Ac):
        """multilevel.py:642-692: Krylov names and callables as coarse solver -- host code on the coarsest level's few
        hundred unknowns, called from inside the cycle"""
        owner, dtype = self, np.dtype(self._DTYPE)

        def vector(ptr, n):
            words = (_lib.C.c_double * (n * dtype.itemsize // 8)).from_address(_lib.C.cast(ptr, _lib.C.c_void_p).value)
            return np.frombuffer(words, dtype=dtype)

        def solve(user, n, b_ptr, x_ptr):
            try:
                b = vector(b_ptr, n).copy()
                vector(x_ptr, n)[:] = np.asarray(fn(Ac, b), dtype=dtype).ravel()
                return 0
            except Exception as e:          # noqa: BLE001 -- must not propagate through the C frames
                owner._callback_error = e
                return 1
        cb = self._COARSE_CALLBACK(solve)
        self._callbacks.append(cb)
        _lib.check(self._fn("set_coarse_callback")(self.h, cb, None))

    # form of _CoarseSolver.device_form -> setter(self, payload, Ac); Ac: the coarsest operator
    _COARSE = {"dense": _set_coarse_dense, "callback": _set_coarse_callback}

    def _build(self, ml, coarse=None):
        levels = ml.levels
        for i, lvl in enumerate(levels):
            self._set_matrix(i, 0, lvl.A)
            if i < len(levels) - 1:
                self._set_matrix(i, 1, lvl.P)
                self._set_matrix(i, 2, lvl.R)
                self._set_smoother(i, 0, getattr(lvl, "presmoother", None), lvl.A)
                self._set_smoother(i, 1, getattr(lvl, "postsmoother", None), lvl.A)
        # coarse is None for a mirror without check_levels: its refusals come from here, in this order
        kind, payload = ml.coarse_solver.device_form(levels[-1].A) if coarse is None else coarse
        if kind == "smoother":
            self._set_smoother(len(levels) - 1, 2, payload, levels[-1].A)
        elif kind != "none":
            if kind not in self._COARSE:
                raise NotImplementedError(self._NO_COARSE % ml.coarse_solver.name())
            self._COARSE[kind](self, payload, levels[-1].A)
        _lib.check(self._fn("finalize")(self.h))

    def _check(self, rc):
        """the engine's return code after a call that may have run a callback: the exception a callback parked is
        raised in place of the engine's report that the callback failed"""
        err, self._callback_error = self._callback_error, None
        if err is not None:
            raise err
        _lib.check(rc)

    def solve(self, b, x, tol, maxiter, cycle, x0_zero=False, fixed=False, device_vectors=False):
        """b, x: contiguous host arrays of the engine's value type, or (device_vectors) addresses in HBM; x is
        overwritten.  Returns the residual history."""
        res = np.zeros(maxiter + 2, dtype=np.float64)
        nres = _lib.C.c_int(0)
        b, x = (b, x) if device_vectors else (b.ctypes.data, x.ctypes.data)
        self._check(self._fn("solve")(self.h, b, x, float(tol), int(maxiter), _CYCLE[cycle], _lib.dp(res),
                                      _lib.C.byref(nres), _flags(x0_zero, fixed, device_vectors)))
        return res[:nres.value]

    def cycle(self, b, x, cycle, x0_zero=False, device_vectors=False):
        b, x = (b, x) if device_vectors else (b.ctypes.data, x.ctypes.data)
        self._check(self._fn("cycle")(self.h, b, x, _CYCLE[cycle], _flags(x0_zero, device_vectors=device_vectors)))

    def cycle_device(self, b_dev, x_dev, cycle):
        """x_dev = one cycle from a zero guess for the right-hand side b_dev (DEVICE pointers): the preconditioner
        M of multilevel.py:306-314 for the device-resident Krylov methods"""
        self.cycle(b_dev, x_dev, cycle, x0_zero=True, device_vectors=True)

    def last_solve_ms(self):
        return self._fn("last_solve_ms")(self.h)

    def device_bytes(self):
        return self._fn("device_bytes")(self.h)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceHierarchy(_ResidentHierarchy):
    """A float64 hierarchy in HBM: an amg_hier handle (include/amgcore_hip.h section 2), the engine of solve()."""

    _PREFIX, _DTYPE, _KIND = "amg_hier_", np.float64, _SM_KIND
    _NO_SMOOTHER = "smoother %r has no device implementation"
    _COARSE_CALLBACK = _lib.COARSE_CALLBACK

    def __init__(self, ml, device=0):
        self._shapes = {}
        self._open(ml, None, len(ml.levels), int(device))

    def _create(self, *args):           # this engine's create returns the handle
        h = self.L.amg_hier_create(*args)
        if not h:
            raise _lib.AmgDeviceError(self.L.amg_last_error().decode())
        return h

    def _set_matrix(self, lvl, which, M):
        if M.dtype != np.float64:
            raise NotImplementedError("device hierarchy supports float64 operators only")
        self._shapes[(lvl, which)] = M.shape
        super()._set_matrix(lvl, which, M, 0)

    def _set_smoother(self, lvl, which, fn, A):
        desc = getattr(fn, "desc", None)
        if desc is not None and desc.get("name") == "krylov":
            return self._set_krylov_smoother(lvl, which, desc, A)
        d = super()._set_smoother(lvl, which, fn, A)
        if d.kind in (10, 11):
            # gauss_seidel_nr sweeps / jacobi_ne gathers through A by columns (lvl.Acsc, smoothing.py:472-478)
            self._set_aux(lvl, which, 0, A.tocsc())
        if d.kind == 10 and not A.tocsr().has_sorted_indices:
            # its starting residual is a CSC product: terms in ascending column order (relaxation.py:992)
            As = A.tocsr().copy()
            As.sort_indices()
            self._set_aux(lvl, which, 1, As)

    def _set_krylov_smoother(self, lvl, which, desc, A):
        """smoothing.py:481-509: a few iterations of an unpreconditioned Krylov method as the level's smoother, run by
        pyamg_amd.krylov on the level's resident vectors from a callback inside the cycle"""
        from . import krylov
        if which == 2:
            raise NotImplementedError("Krylov methods as coarse solver go through coarse_grid_solver('cg' ...)")
        method = desc["method"]
        tol, maxiter, restrt = float(desc["tol"]), desc["maxiter"], desc.get("restrt")
        aux = (which, 0) if method in ("cgne", "cgnr") else None
        owner = self

        def relax(user, level, x_dev, b_dev):
            try:
                with krylov.DeviceSpace(owner, level, cycle=None, aux=aux) as V:
                    krylov.run(method, V, b_dev, x_dev, tol, maxiter, restrt=restrt)
                return 0
            except Exception as e:          # noqa: BLE001 -- must not propagate through the C frames
                owner._callback_error = e
                return 1
        cb = _lib.RELAX_CALLBACK(relax)
        self._callbacks.append(cb)
        _lib.check(self.L.amg_hier_set_callback_smoother(self.h, lvl, which, cb, None))
        if aux is not None:
            self._set_aux(lvl, which, 0, sparse.csc_matrix(A))        # A by columns = A^T by rows

    def _set_aux(self, lvl, which, slot, M):
        M.sort_indices()
        Ap = np.ascontiguousarray(M.indptr, dtype=np.intc)
        Aj = np.ascontiguousarray(M.indices, dtype=np.intc)
        Ax = np.ascontiguousarray(M.data, dtype=np.float64)
        nmajor = len(Ap) - 1
        nminor = M.shape[0] if sparse.isspmatrix_csc(M) else M.shape[1]
        _lib.check(self.L.amg_hier_set_aux_matrix(self.h, lvl, which, slot, nmajor, nminor, _lib.ip(Ap), _lib.ip(Aj),
                                                  _lib.dp(Ax)))

    def _build(self, ml, coarse=None):
        super()._build(ml, coarse)
        # Large hierarchies: the CSR arrays of operators that are only ever applied from their stencil / sliced form
        # are not kept beside it (500^3 Chebyshev hierarchy: 56.6 -> 34 GB in HBM, same bits).  The host copies stay in
        # ml.levels, so change_smoothers / a rebuilt mirror have everything they need.  AMG_RELEASE_SOURCES=0 keeps
        # them (A/B runs of the other kernels on a live hierarchy), =1 releases at any size.
        rel = os.environ.get("AMG_RELEASE_SOURCES")
        big = ml.levels[0].A.shape[0] >= 4000000
        self.released_bytes = 0
        if rel == "1" or (rel is None and big):
            self.released_bytes = int(self.L.amg_hier_release_sources(self.h))

    def pcg(self, b, x, tol, maxiter, cycle, x0_zero=False, device_vectors=False):
        """preconditioned CG around the cycle, b and x as in solve().  Returns the history and CG's info."""
        res = np.zeros(maxiter + 2, dtype=np.float64)
        nres, info = _lib.C.c_int(0), _lib.C.c_int(0)
        b, x = (b, x) if device_vectors else (b.ctypes.data, x.ctypes.data)
        self._check(self.L.amg_hier_pcg(self.h, b, x, float(tol), int(maxiter), _CYCLE[cycle], _lib.dp(res),
                                        _lib.C.byref(nres), _lib.C.byref(info),
                                        _flags(x0_zero, device_vectors=device_vectors)))
        return res[:nres.value], info.value

    def level_size(self, lvl):
        return self._shapes[(lvl, 0)][0]

    def relax(self, lvl, which, b, x):
        self._check(self.L.amg_hier_relax(self.h, lvl, which, _lib.dp(b), _lib.dp(x)))

    def matvec(self, lvl, which, x):
        rows, cols = self._shapes[(lvl, which)]
        x = np.ascontiguousarray(np.ravel(x), dtype=np.float64)
        if x.size != cols:
            raise ValueError("dimension mismatch")
        y = np.zeros(rows, dtype=np.float64)
        _lib.check(self.L.amg_hier_matvec(self.h, lvl, which, _lib.dp(x), _lib.dp(y)))
        return y

    def cycle_bytes(self, cycle="V"):
        return self.L.amg_hier_cycle_bytes(self.h, _CYCLE[cycle])

    def cycle_bytes_moved(self, cycle="V"):
        return self.L.amg_hier_cycle_bytes_moved(self.h, _CYCLE[cycle])

    def time_spmv(self, lvl, which, mode=0, reps=10):
        ms = _lib.C.c_double(0.0)
        _lib.check(self.L.amg_hier_time_spmv(self.h, lvl, which, mode, reps, _lib.C.byref(ms)))
        return ms.value

    def time_relax(self, lvl, which, reps=5):
        ms = _lib.C.c_double(0.0)
        self._check(self.L.amg_hier_time_relax(self.h, lvl, which, reps, _lib.C.byref(ms)))
        return ms.value


class _DeviceHierarchyC128(_ResidentHierarchy):
    """A complex128 hierarchy in HBM: an amg_hierx handle (include/amgcore_hip.h section 5).  Plain CSR / BSR
    operators, eager launches; the cycle gives the reference's bits."""

    _PREFIX, _DTYPE, _DESC, _KIND = "amg_hierx_", np.complex128, _lib.SmootherDescX, _C128_KIND
    _NO_SMOOTHER = "smoother %r has no complex128 device implementation"
    _COARSE_CALLBACK = _lib.COARSE_CALLBACK_X

    def __init__(self, ml, device=0):
        self._open(ml, self.check_levels(ml), _lib.AMG_VALUE_C128, len(ml.levels), int(device))

    @staticmethod
    def check_levels(ml):
        """the refusals that need no device: every A complex128 and square, smoothers the engine implements"""
        for i, lvl in enumerate(ml.levels):
            if lvl.A.dtype != np.complex128:
                raise NotImplementedError("complex hierarchy: level %d operator A is %s, not complex128" % (i, lvl.A.dtype))
            if i < len(ml.levels) - 1:
                for side in ("presmoother", "postsmoother"):
                    _DeviceHierarchyC128._desc_of(i, getattr(lvl, side, None))
        s = ml.coarse_solver.solver
        if _is_own_krylov(s):
            # pyamg_amd.krylov runs float64 on the device: it would drop the imaginary parts of the coarse problem
            raise NotImplementedError(
                "coarse solver %r: the device Krylov methods are float64 only; for a complex128 hierarchy use a dense "
                "or relaxation coarse solver, a name only scipy has ('cgs', 'qmr', 'minres', 'bicg'), or a callable"
                % (getattr(s, "__name__", s),))
        if isinstance(s, str) and s not in _CoarseSolver._DENSE + _CoarseSolver._RELAX + _SCIPY_ONLY_COARSE:
            raise NotImplementedError("coarse solver %r has no complex128 device implementation" % (s,))
        kind, payload = ml.coarse_solver.device_form(ml.levels[-1].A)
        if kind == "smoother":
            _DeviceHierarchyC128._desc_of(len(ml.levels) - 1, payload)
        return kind, payload

    def _set_desc(self, lvl, which, d):         # the coarse smoother is slot 2 of the last level
        _lib.check(self.L.amg_hierx_set_smoother(self.h, lvl, which, d))


_MULTI_KIND = {None: 0, "None": 0, "jacobi": 1, "gauss_seidel": 2, "sor": 3, "polynomial": 4}
_MULTI_KMAX = 8          # widest column layout of the engine; more columns run in groups


def _rhs_groups(k, kmax=_MULTI_KMAX):
    """How k right-hand sides run: a list of (first column, columns, layout width).  Groups of kmax columns, the last
    one padded with zero columns to the next width of 1, 2, 4, 8."""
    if k < 1:
        raise ValueError("at least one right-hand side is needed")
    groups = []
    for first in range(0, k, kmax):
        cols = min(kmax, k - first)
        width = 1
        while width < cols:
            width *= 2
        groups.append((first, cols, width))
    return groups


# One batched cycle against one cycle per column, measured on SA hierarchies of 3-D Poisson problems with Chebyshev(2)
# smoothers (profiles/r07_multirhs.txt): (unknowns up to, speed-up of 4 columns, speed-up of 8 columns).  The batched
# engine runs the next width of 1, 2, 4, 8 columns, streams plain CSR and launches eagerly; the one-vector engine has
# compressed operator forms, fused level-0 passes, graph replay and dataflow Gauss-Seidel sweeps, so the batch wins
# where launches dominate (small problems, wide batches) and loses where bytes do.
_BATCHED_SPEEDUP = [(4096, 2.29, 5.22), (32768, 1.07, 2.58), (262144, 0.77, 1.95), (1000000, 0.66, 1.43),
                    (4096000, 0.45, 1.06)]
_BATCHED_MARGIN = 1.1


def _batched_cycle_pays(ml, k):
    """aspreconditioner().matmat: is one batched cycle of k columns faster than k cycles?  Only where it was
    measured to be, with a margin: never for one or two columns (0.54 and 0.97 at the smallest size), never on
    hierarchies with Gauss-Seidel / SOR sweeps (a launch per dependency level against the dataflow sweep: 0.62 for 8
    columns at 128^3), never above the largest size at which eight columns won; a group of k columns in a layout of
    w costs what w columns cost."""
    for lvl in ml.levels[:-1]:
        for side in ("presmoother", "postsmoother"):
            desc = getattr(getattr(lvl, side, None), "desc", None) or {}
            if desc.get("name") in ("gauss_seidel", "sor"):
                return False
    if k < 3:
        return False
    n = ml.levels[0].A.shape[0]
    k = min(k, _MULTI_KMAX)               # more columns run in groups of 8
    for nmax, speedup4, speedup8 in _BATCHED_SPEEDUP:
        if n <= nmax:
            width, speedup = (4, speedup4) if k <= 4 else (8, speedup8)
            return speedup * k / width >= _BATCHED_MARGIN
    return False


class _DeviceHierarchyMulti(_ResidentHierarchy):
    """A float64 hierarchy in HBM for several right-hand sides at once: an amg_hierm handle (include/amgcore_hip.h
    section 6).  Plain CSR operators, eager launches; per column the cycle gives the bits of the one-vector engine
    (DESIGN.md section 9c)."""

    _PREFIX, _DTYPE, _KIND = "amg_hierm_", np.float64, _MULTI_KIND
    _NO_SMOOTHER = ("solve_many: smoother %r is not implemented (jacobi, gauss_seidel, sor, "
                    "polynomial / chebyshev / richardson, None)")
    _NO_COARSE = "coarse solver %s has no implementation for several right-hand sides"
    _COARSE = {"dense": _ResidentHierarchy._set_coarse_dense}
    cycle_device = None             # the columns come from the host

    def __init__(self, ml, device=0, kmax=_MULTI_KMAX):
        self.kmax = int(kmax)
        self._cycles = 0
        self._open(ml, self.check_levels(ml), len(ml.levels), int(device), self.kmax)

    @staticmethod
    def check_levels(ml):
        """the refusals, none of which needs a device: float64 operators in CSR or BSR(1,1), smoothers and a coarse
        solver the engine implements.  Returns the coarse solver's device form."""
        for i, lvl in enumerate(ml.levels):
            ops = [("A", lvl.A)]
            if i < len(ml.levels) - 1:
                ops += [("P", lvl.P), ("R", lvl.R)]
            for name, M in ops:
                if np.iscomplexobj(M):
                    raise NotImplementedError("solve_many: complex hierarchies are not implemented (level %d %s)" % (i, name))
                if M.dtype != np.float64:
                    raise NotImplementedError("solve_many: float64 operators only (level %d %s is %s)" % (i, name, M.dtype))
                if sparse.isspmatrix_bsr(M) and tuple(M.blocksize) != (1, 1):
                    raise NotImplementedError("solve_many: BSR blocks larger than 1 x 1 are not implemented "
                                              "(level %d %s has %s blocks)" % (i, name, (M.blocksize,)))
            if i < len(ml.levels) - 1:
                for side in ("presmoother", "postsmoother"):
                    _DeviceHierarchyMulti._desc_of(i, getattr(lvl, side, None))
        s = ml.coarse_solver.solver
        if callable(s) or (s is not None and s not in _CoarseSolver._DENSE + tuple(
                n for n in _CoarseSolver._RELAX if not n.startswith("block_"))):
            raise NotImplementedError("solve_many: coarse solver %r is not implemented (dense solvers, jacobi, "
                                      "gauss_seidel, sor, richardson, chebyshev or None)" % (getattr(s, "__name__", s),))
        kind, payload = ml.coarse_solver.device_form(ml.levels[-1].A)
        if kind == "smoother":
            _DeviceHierarchyMulti._desc_of(len(ml.levels) - 1, payload)
        return kind, payload

    def solve(self, B, X, tol, maxiter, cycle, x0_zero=False, fixed=False):
        """B, X: C-contiguous float64 (n, k), k <= kmax; X is overwritten.  Returns the k residual histories."""
        k = B.shape[1]
        res = np.zeros((k, maxiter + 1), dtype=np.float64)
        nres = np.zeros(k, dtype=np.intc)
        _lib.check(self.L.amg_hierm_solve(self.h, k, B.ctypes.data, X.ctypes.data, float(tol), int(maxiter),
                                          _CYCLE[cycle], _lib.dp(res), _lib.ip(nres), _flags(x0_zero, fixed)))
        self._cycles += int(nres.max()) - 1
        return [res[j, :nres[j]] for j in range(k)]

    def cycle(self, B, X, cycle, x0_zero=False):
        _lib.check(self.L.amg_hierm_cycle(self.h, B.shape[1], B.ctypes.data, X.ctypes.data, _CYCLE[cycle],
                                          _flags(x0_zero)))
        self._cycles += 1

    def cycles_run(self):
        """batched cycles this mirror has run (one per cycle of a group of columns)"""
        return self._cycles


def _is_c128(ml):
    return ml.levels[0].A.dtype == np.complex128


class multilevel_solver:
    """Stores multigrid hierarchy and implements the multigrid cycle
    (multilevel.py:14-548).  Same attributes and methods as the reference."""

    class level:
        """One level: A, and (except on the coarsest) P, R, presmoother,
        postsmoother (multilevel.py:45-68)."""

        def __init__(self):
            pass

    def __init__(self, levels, coarse_solver="pinv2", device=0):
        self.levels = levels
        self.coarse_solver = coarse_grid_solver(coarse_solver)
        self.device = device
        self._dev = None
        self._devm = None
        for level in levels[:-1]:
            if not hasattr(level, "R"):
                level.R = level.P.conj().T.asformat(level.P.format)   # level.P.H (multilevel.py:154-156)

    # ------------------------------------------------------------------ reporting
    def _level_nnz(self):
        return [int(level.A.nnz) for level in self.levels]

    def __repr__(self):
        """Same text as the reference prints (multilevel.py:158-176): header lines, then one row
        per level with its share of the stored entries."""
        nnz = self._level_nnz()
        total = float(sum(nnz))
        lines = ["multilevel_solver",
                 "Number of Levels:     %d" % len(self.levels),
                 "Operator Complexity: %6.3f" % self.operator_complexity(),
                 "Grid Complexity:     %6.3f" % self.grid_complexity(),
                 "Coarse Solver:        %s" % self.coarse_solver.name(),
                 "  level   unknowns     nonzeros"]
        for i, level in enumerate(self.levels):
            lines.append("   %2d   %10d   %10d [%5.2f%%]" % (i, level.A.shape[1], nnz[i], 100 * nnz[i] / total))
        return "\n".join(lines) + "\n"

    def _level_visits(self, cycle):
        """How many times one cycle of the given type arrives at each level.  V goes down once;
        W arrives twice at every level below the first, except that the coarsest level is
        solved once per arrival at the level above it; F arrives once as F and once as V."""
        nlev = len(self.levels)
        visits = [0] * nlev

        def arrive(lvl, kind, times):
            visits[lvl] += times
            if lvl == nlev - 2:
                visits[nlev - 1] += times
            elif lvl < nlev - 2:
                if kind == "V":
                    arrive(lvl + 1, "V", times)
                elif kind == "W":
                    arrive(lvl + 1, "W", 2 * times)
                else:
                    arrive(lvl + 1, "F", times)
                    arrive(lvl + 1, "V", times)
        arrive(0, cycle, 1)
        return visits

    def cycle_complexity(self, cycle="V"):
        """Entries of the level operators touched by one cycle, relative to the finest operator:
        every arrival at a level costs two passes over A (pre- and post-smoothing), the coarsest
        level one (its solve) -- the values of multilevel.py:178-248."""
        kind = {"V": "V", "W": "W", "AMLI": "W", "F": "F"}[_cycle_name(cycle)]
        nnz = self._level_nnz()
        if len(nnz) == 1:
            return 1.0
        visits = self._level_visits(kind)
        work = sum(2 * v * z for v, z in zip(visits[:-1], nnz[:-1])) + visits[-1] * nnz[-1]
        return float(work) / float(nnz[0])

    def operator_complexity(self):
        """stored entries of all level operators over those of the finest (multilevel.py:250-259)"""
        nnz = self._level_nnz()
        return sum(nnz) / float(nnz[0])

    def grid_complexity(self):
        """unknowns of all levels over those of the finest (multilevel.py:261-269)"""
        sizes = [level.A.shape[0] for level in self.levels]
        return sum(sizes) / float(sizes[0])

    # ------------------------------------------------------------------ on-disk format
    def save(self, path):
        """Write the hierarchy (operators in stored order, smoother constants, the dense coarse operator) to the
        directory `path`; `multilevel_solver.load(path)` gives a solver with bit-identical iterates."""
        from .hierarchy_io import save_hierarchy
        return save_hierarchy(self, path)

    @staticmethod
    def load(path, mmap=False, device=0):
        from .hierarchy_io import load_hierarchy
        return load_hierarchy(path, mmap=mmap, device=device)

    # ------------------------------------------------------------------ device mirror
    def _invalidate_device(self):
        if self._dev is not None:
            self._dev.close()
        self._dev = None
        if getattr(self, "_devm", None) is not None:
            self._devm.close()
        self._devm = None

    def device_hierarchy(self):
        """The HBM-resident mirror of this hierarchy (built on first use)."""
        if self._dev is None:
            if _is_c128(self):
                self._dev = _DeviceHierarchyC128(self, self.device)
            else:
                self._dev = _DeviceHierarchy(self, self.device)
        return self._dev

    def device_hierarchy_multi(self):
        """The HBM-resident mirror that solve_many runs on (built on first use; several right-hand sides at once)."""
        if getattr(self, "_devm", None) is None:
            self._devm = _DeviceHierarchyMulti(self, self.device)
        return self._devm

    # ------------------------------------------------------------------ solve
    def psolve(self, b):
        return self.solve(b, maxiter=1)

    def aspreconditioner(self, cycle="V", batched=None):
        """multilevel.py:274-314.  The operator also has a matmat: M.matmat(X) is one batched cycle of solve_many
        for all columns (batched=True, or batched=None where that was measured faster than one cycle per column:
        _batched_cycle_pays) when the hierarchy is one solve_many takes, and the loop over columns scipy would have
        made otherwise (batched=False: always).  Either way column j is M.matvec(X[:, j]) bit for bit."""
        from scipy.sparse.linalg import LinearOperator
        shape = self.levels[0].A.shape
        dtype = self.levels[0].A.dtype

        def matvec(b):
            return self.solve(b, maxiter=1, cycle=cycle, tol=1e-12)

        def matmat(X):
            X = np.asarray(X)
            use = batched is not False and not np.iscomplexobj(X)
            if use and batched is None:
                use = _batched_cycle_pays(self, X.shape[1])
            if use:
                try:
                    self._check_many(cycle)
                except NotImplementedError:
                    use = False
            if not use:
                return np.hstack([matvec(X[:, j]).reshape(-1, 1) for j in range(X.shape[1])])
            return self.solve_many(X, maxiter=1, cycle=cycle, tol=1e-12)
        op = LinearOperator(shape, matvec, matmat=matmat, dtype=dtype)
        op.hierarchy, op.cycle = self, cycle          # what pyamg_amd.krylov_c128 looks for in its M
        return op

    def _check_many(self, cycle):
        """what solve_many refuses about the hierarchy and the cycle, before any device work; returns the cycle's name"""
        cycle = _cycle_name(cycle)
        if cycle == "AMLI":
            raise NotImplementedError("solve_many: AMLI cycles are not implemented")
        if getattr(self, "_devm", None) is None:
            _DeviceHierarchyMulti.check_levels(self)
        return cycle

    def solve_many(self, B, X0=None, tol=1e-5, maxiter=100, cycle="V", residuals=None, callback=None, accel=None):
        """solve() for the k columns of B at once: column j of the result and residuals[j] are what
        solve(B[:, j], x0=X0[:, j], tol=tol, maxiter=maxiter, cycle=cycle, residuals=r) returns -- the column stops by
        its own tol * ||b_j||, and what is returned for it is the iterate at which it stopped.  Every operator entry
        is read once per application for all columns.

        B, X0: real array-likes (n, k), k >= 1, on the host.  Returns a new C-contiguous float64 (n, k) array.
        residuals, when a list, receives k lists of floats.  callback(j, x_j) is called after every cycle for every
        column still iterating.  float64 hierarchies with CSR / BSR(1,1) operators, jacobi / gauss_seidel / sor /
        polynomial smoothers, a dense or relaxation coarse solver, V / W / F cycles; anything else raises
        NotImplementedError before any device work."""
        if _is_device_tensor(B) or (X0 is not None and _is_device_tensor(X0)):
            raise NotImplementedError("solve_many: torch device tensors are not implemented; pass host arrays")
        if accel is not None:
            raise NotImplementedError("solve_many: Krylov acceleration (accel) is not implemented")
        B = np.asarray(B)
        n = self.levels[0].A.shape[0]
        if B.ndim != 2:
            raise ValueError("B must be two-dimensional (n, k); solve() takes one vector")
        if B.shape[0] != n:
            raise ValueError("B must have %d rows" % n)
        k = B.shape[1]
        if k == 0:
            raise ValueError("B has no columns")
        if X0 is not None:
            X0 = np.asarray(X0)
            if X0.shape != B.shape:
                raise ValueError("X0 must have the shape of B, %s" % (B.shape,))
        cycle = self._check_many(cycle)
        if np.iscomplexobj(B) or (X0 is not None and np.iscomplexobj(X0)):
            raise NotImplementedError("solve_many: complex right-hand sides are not implemented")
        maxiter = int(maxiter)
        X = np.zeros((n, k), dtype=np.float64) if X0 is None else np.array(X0, dtype=np.float64, order="C")
        hist = [[] for _ in range(k)]
        dev = self.device_hierarchy_multi()
        for first, cols, _width in _rhs_groups(k, dev.kmax):
            Bg = np.ascontiguousarray(B[:, first:first + cols], dtype=np.float64)
            Xg = np.ascontiguousarray(X[:, first:first + cols])
            x0_zero = not np.any(Xg)
            if callback is None:
                res = dev.solve(Bg, Xg, tol, maxiter, cycle, x0_zero=x0_zero)
                for j in range(cols):
                    hist[first + j] = [float(r) for r in res[j]]
            else:
                self._solve_many_callback(dev, Bg, Xg, tol, maxiter, cycle, x0_zero, first, hist, callback)
            X[:, first:first + cols] = Xg
        if residuals is not None:
            residuals[:] = hist
        return X

    @staticmethod
    def _solve_many_callback(dev, Bg, Xg, tol, maxiter, cycle, x0_zero, first, hist, callback):
        """one cycle per engine call so that callback(j, x_j) sees every iterate of an active column
        (multilevel.py:454-466); a column that stopped keeps the iterate it stopped at"""
        cols = Bg.shape[1]
        res = dev.solve(Bg, Xg, 0.0, 0, cycle, x0_zero=x0_zero)
        normb = [float(r[0]) for r in dev.solve(np.ascontiguousarray(Bg), np.zeros_like(Xg), 0.0, 0, cycle, x0_zero=True)]
        atol = [tol * nb if nb != 0 else tol for nb in normb]
        for j in range(cols):
            hist[first + j] = [float(res[j][0])]
        active = [j for j in range(cols) if hist[first + j][-1] > atol[j]]
        work = Xg.copy()
        it = 0
        while active and it < maxiter:
            res = dev.solve(Bg, work, 0.0, 1, cycle, x0_zero=x0_zero, fixed=True)
            x0_zero = False
            it += 1
            still = []
            for j in active:
                hist[first + j].append(float(res[j][-1]))
                Xg[:, j] = work[:, j]
                callback(first + j, Xg[:, j].copy())
                if hist[first + j][-1] > atol[j]:
                    still.append(j)
            active = still

    def solve(self, b, x0=None, tol=1e-5, maxiter=100, cycle="V", accel=None, callback=None,
              residuals=None, return_residuals=False):
        """Main solution call to execute multigrid cycling (multilevel.py:316-471).

        Extension: b (and x0) may be torch CUDA tensors (float64, contiguous, on the hierarchy's device): the solve then
        never touches the host -- no PCIe copy of b / x0 in or x out (3 GB at 500^3) -- and returns a tensor.  Plain
        cycling and accel='cg' (the device PCG); same iterates and history as with host vectors."""
        if _is_device_tensor(b):
            return self._solve_device_tensors(b, x0, tol, maxiter, cycle, accel, callback, residuals)
        A = self.levels[0].A
        c128 = _is_c128(self)       # V, W and F cycles on the complex128 engine: the reference's bits
        b = np.asarray(b)
        x = np.zeros_like(b) if x0 is None else np.array(x0)   # copy
        cycle = _cycle_name(cycle)
        if cycle == "AMLI":
            if c128:
                raise NotImplementedError("AMLI cycles are not implemented for complex128 hierarchies")
            if hasattr(A, "symmetry") and A.symmetry != "hermitian":
                raise ValueError("AMLI cycles require symmetry to be hermitian")

        if accel is not None:
            return self._solve_accel(b, x0, tol, maxiter, cycle, accel, callback, residuals)

        if return_residuals:
            warn("return_residuals is deprecated.  Use residuals instead")
            residuals = []
        if residuals is None:
            residuals = []
        else:
            residuals[:] = []

        n = A.shape[0]

        def check_size():
            if b.size != n or x.size != n:
                raise ValueError("b and x0 must have %d entries" % n)
        if c128:
            check_size()
            tp = np.result_type(b.dtype, x.dtype, A.dtype)     # upcast(b, x, A)
            if tp != np.complex128:
                raise NotImplementedError("complex128 hierarchy: b and x0 of type %s" % tp)
            if self._dev is None:
                _DeviceHierarchyC128.check_levels(self)          # refusals before any device work
        else:
            tp = np.result_type(b.dtype, x.dtype, A.dtype)
            if tp != np.float64 and not (np.issubdtype(tp, np.floating) or np.issubdtype(tp, np.integer)):
                raise NotImplementedError("device solve supports real float64 systems only")
            check_size()
        shape = b.shape
        b1 = np.ascontiguousarray(np.ravel(b), dtype=np.complex128 if c128 else np.float64)
        x1 = np.ascontiguousarray(np.ravel(x), dtype=b1.dtype)
        x0_zero = not np.any(x1)
        dev = self.device_hierarchy()

        if callback is None:
            res = dev.solve(b1, x1, tol, maxiter, cycle, x0_zero=x0_zero)
            residuals.extend(float(r) for r in res)
        else:
            # one cycle per call so that callback(x) sees every iterate (multilevel.py:454-466)
            normb = float(np.sqrt(np.vdot(b1, b1).real if c128 else np.inner(b1, b1)))
            atol = tol * normb if normb != 0 else tol
            res = dev.solve(b1, x1, 0.0, 0, cycle, x0_zero=x0_zero)
            residuals.append(float(res[0]))
            while len(residuals) <= maxiter and residuals[-1] > atol:
                res = dev.solve(b1, x1, 0.0, 1, cycle, x0_zero=x0_zero, fixed=True)
                x0_zero = False
                residuals.append(float(res[-1]))
                callback(x1.reshape(shape))
        xout = x1.reshape(shape)
        if return_residuals:
            return xout, residuals
        return xout

    def _solve_device_tensors(self, b, x0, tol, maxiter, cycle, accel, callback, residuals):
        import torch
        if _is_c128(self):
            raise NotImplementedError("device tensors: float64 hierarchies only; pass host arrays to a complex128 one")
        cycle = _cycle_name(cycle)
        if callback is not None or accel not in (None, "cg"):
            raise NotImplementedError("device tensors: plain cycling and accel='cg' (no callback); pass host arrays otherwise")
        if accel == "cg" and cycle == "AMLI":
            raise ValueError("AMLI cycles require acceleration (accel) to be fgmres, or no acceleration")
        n = self.levels[0].A.shape[0]
        dev = self.device_hierarchy()
        for t in (b,) if x0 is None else (b, x0):
            if not _is_device_tensor(t) or t.dtype != torch.float64 or t.numel() != n or not t.is_contiguous() or t.device.index != self.device:
                raise ValueError("device tensors must be contiguous float64 CUDA tensors of %d entries on device %d" % (n, self.device))
        x = torch.zeros_like(b) if x0 is None else x0.clone()
        torch.cuda.current_stream(b.device).synchronize()          # the library works on its own stream
        if accel == "cg":
            if maxiter is None:
                maxiter = int(1.3 * n) + 2
            res, info = dev.pcg(b.data_ptr(), x.data_ptr(), tol, maxiter, cycle, x0_zero=x0 is None, device_vectors=True)
            if info < 0:
                warn("Indefinite matrix or preconditioner detected in CG, aborting")
        else:
            res = dev.solve(b.data_ptr(), x.data_ptr(), tol, 100 if maxiter is None else maxiter, cycle,
                            x0_zero=x0 is None, device_vectors=True)
        if residuals is not None:
            residuals[:] = [float(r) for r in res]
        return x

    def _solve_accel(self, b, x0, tol, maxiter, cycle, accel, callback, residuals):
        """Krylov acceleration (multilevel.py:381-422): the cycle is the preconditioner M;
        the outer Krylov iteration is scipy's (the reference falls back to the same
        scipy.sparse.linalg interface, :404-422)."""
        own = _is_own_krylov(accel)
        if _is_c128(self):
            if own:
                raise NotImplementedError(
                    "the device Krylov methods are float64 only; for a complex128 hierarchy pass a scipy.sparse.linalg "
                    "callable as accel, or use aspreconditioner() as M")
            from . import krylov_c128
            if any(accel is f for f in krylov_c128.METHODS.values()):
                # the complex128 device methods: vectors stay in HBM, the cycle is M
                return accel(self.levels[0].A, b, x0=x0, tol=tol, maxiter=maxiter, M=self.aspreconditioner(cycle=cycle),
                             callback=callback, residuals=residuals)[0]
            _DeviceHierarchyC128.check_levels(self)
        if (accel != "fgmres") and (cycle == "AMLI"):
            raise ValueError("AMLI cycles require acceleration (accel) to be fgmres, or no acceleration")
        if accel == "cg" and callback is None:
            # device-resident PCG (pyamg/krylov/_cg.py semantics, preconditioner-norm history)
            n = self.levels[0].A.shape[0]
            b1 = np.ascontiguousarray(np.ravel(b), dtype=np.float64)
            x1 = np.zeros(n) if x0 is None else np.ascontiguousarray(np.ravel(np.array(x0)), dtype=np.float64)
            if maxiter is None:
                maxiter = int(1.3 * n) + 2
            res, info = self.device_hierarchy().pcg(b1, x1, tol, maxiter, cycle, x0_zero=not np.any(x1))
            if info < 0:
                warn("Indefinite matrix or preconditioner detected in CG, aborting")
            if residuals is not None:
                residuals[:] = [float(r) for r in res]
            return x1.reshape(np.asarray(b).shape)
        if own:
            # pyamg.krylov's own methods (multilevel.py:390-394), device-resident: vectors stay in HBM, the cycle is M
            from . import krylov
            name = accel if isinstance(accel, str) else accel.__name__
            n = self.levels[0].A.shape[0]
            b1 = np.ascontiguousarray(np.ravel(b), dtype=np.float64)
            x1 = np.zeros(n) if x0 is None else np.ascontiguousarray(np.ravel(np.array(x0)), dtype=np.float64)
            dev = self.device_hierarchy()
            aux = None
            if name in ("cgne", "cgnr"):
                dev._set_aux(0, 0, 0, sparse.csc_matrix(self.levels[0].A))
                aux = (0, 0)
            with krylov.DeviceSpace(dev, 0, cycle=cycle, aux=aux) as V:
                bd, xd = V.upload(b1), V.upload(x1)
                info = krylov.run(name, V, bd, xd, tol, maxiter, residuals=residuals, callback=callback)
                x1 = V.download(xd)
            if info < 0 and name == "cg":
                warn("Indefinite matrix or preconditioner detected in CG, aborting")
            return x1.reshape(np.asarray(b).shape)
        # anything else is scipy's (multilevel.py:395-396, 404-422): host vectors, the device cycle as M
        import scipy.sparse.linalg as spla
        if isinstance(accel, str):
            if not hasattr(spla, accel):
                raise ValueError("unknown accel method %r" % accel)
            accel = getattr(spla, accel)
        A = self.levels[0].A
        M = self.aspreconditioner(cycle=cycle)
        cb = callback
        if residuals is not None:
            residuals[:] = [float(np.linalg.norm(np.ravel(b) - A * np.ravel(np.zeros_like(b) if x0 is None else x0)))]

            def callback(x):
                if np.isscalar(x):
                    residuals.append(float(x))
                else:
                    residuals.append(float(np.linalg.norm(np.ravel(b) - A * np.ravel(x))))
                if cb is not None:
                    cb(x)
        try:
            return accel(A, b, x0=x0, rtol=tol, maxiter=maxiter, M=M, callback=callback)[0]
        except TypeError:
            return accel(A, b, x0=x0, tol=tol, maxiter=maxiter, M=M, callback=callback)[0]


def _is_device_tensor(v):
    return hasattr(v, "data_ptr") and hasattr(v, "is_cuda") and bool(v.is_cuda)


def coarse_grid_solver(solver):
    """Return a coarse grid solver suitable for multilevel_solver
    (multilevel.py:554-720).

    Dense methods ('pinv', 'pinv2', 'lu', 'cholesky', 'splu') are turned into
    one dense operator at setup and applied on the device; relaxation names run
    the corresponding device smoother from a zero guess (default 10
    iterations); None gives a zero correction.  ('dense', {'M': array}) supplies
    the operator directly.  Krylov names ('cg', 'gmres', 'bicgstab', ... and
    scipy's 'cgs', 'qmr', 'minres', 'bicg') and arbitrary callables act on the
    coarsest level's few hundred unknowns from a callback inside the cycle.
    """
    if isinstance(solver, _CoarseSolver):
        return solver
    return _CoarseSolver(solver)


class _CoarseSolver(object):
    _DENSE = ("pinv", "pinv2", "lu", "cholesky", "splu", "dense")
    _RELAX = ("gauss_seidel", "jacobi", "block_gauss_seidel", "block_jacobi", "richardson", "sor",
              "chebyshev")

    def __init__(self, solver):
        self.spec = solver
        if isinstance(solver, tuple):
            self.solver, self.kwargs = solver[0], dict(solver[1])
        else:
            self.solver, self.kwargs = solver, {}
        ok = self.solver is None or callable(self.solver) or self.solver in self._DENSE + self._RELAX + (
            "schwarz", "jacobi_ne", "gauss_seidel_ne", "gauss_seidel_nr", "bicg", "bicgstab", "cg", "cgs",
            "gmres", "qmr", "minres")
        if not ok:
            raise ValueError("unknown solver: %s" % self.solver)

    def device_form(self, A):
        """-> ('dense', M) | ('smoother', closure) | ('none', None)"""
        s = self.solver
        if s is None:
            return "none", None
        if s in self._DENSE:
            if not hasattr(self, "P"):
                if s == "dense":
                    self.P = np.asarray(self.kwargs["M"], dtype=np.complex128 if A.dtype == np.complex128 else np.float64)
                elif A.nnz == 0:
                    self.P = np.zeros(A.shape)
                elif s in ("pinv", "pinv2"):
                    self.P = scipy.linalg.pinv(A.toarray(), **self.kwargs)      # multilevel.py:608-612
                else:
                    # lu / cholesky / splu: exact inverse of the (nonsingular part of the) operator
                    self.P = scipy.linalg.pinv(A.toarray())
            return "dense", self.P
        if s in self._RELAX:
            from . import smoothing
            kw = dict(self.kwargs)
            if "iterations" not in kw:
                kw["iterations"] = 10                                           # multilevel.py:665-666
            lvl = multilevel_solver.level()
            lvl.A = A
            return "smoother", getattr(smoothing, "setup_" + str(s))(lvl, **kw)
        # Krylov names and callables (multilevel.py:642-660, 687-689): host code on the coarsest level, called from
        # inside the device cycle with the restricted right-hand side
        kw = dict(self.kwargs)
        if callable(s):
            return "callback", (lambda A_, b_: s(A_, b_, **kw))
        from . import krylov
        if "tol" not in kw:
            kw["tol"] = float(np.finfo(np.float64).eps * 1e6)                  # multilevel.py:649-657
        if s in krylov.METHODS:
            return "callback", (lambda A_, b_: krylov.solve_host(A_, b_, method=s, **kw))
        import scipy.sparse.linalg as spla

        def scipy_solve(A_, b_):
            k2 = dict(kw)
            k2["rtol"] = k2.pop("tol")
            return getattr(spla, s)(A_, b_, **k2)[0]
        return "callback", scipy_solve

    def __call__(self, A, b):
        """generic_solver.__call__ (multilevel.py:694-712): solve on the device."""
        b = np.asanyarray(b)
        if A.nnz == 0:
            return np.zeros(b.shape)
        lvl = multilevel_solver.level()
        lvl.A = sparse.csr_matrix(A) if not (sparse.isspmatrix_csr(A) or sparse.isspmatrix_bsr(A)) else A
        kind, payload = self.device_form(lvl.A)
        if kind == "callback":
            return np.asarray(payload(lvl.A, np.ravel(b))).reshape(b.shape)
        ml = multilevel_solver([lvl], coarse_solver=self)
        dt = np.complex128 if lvl.A.dtype == np.complex128 else np.float64
        x = np.zeros(A.shape[0], dtype=dt)
        ml.device_hierarchy().cycle(np.ascontiguousarray(np.ravel(b), dtype=dt), x, "V", x0_zero=True)
        ml._invalidate_device()
        return x.reshape(b.shape)

    def __repr__(self):
        return "coarse_grid_solver(" + repr(self.solver) + ")"

    def name(self):
        return repr(getattr(self, "solver_name", None) or self.solver)
