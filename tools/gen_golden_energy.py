#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the energy-minimisation prolongation smoothing fixtures.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on its own native module oracle/_ref/_amg_core.so, as
tools/gen_golden_evolution.py does -- and records, under tests/golden/energy/ (a directory of its own:
golden_io._all_cases() lists the hier_*.npz files of tests/golden/ itself):

  <problem>.npz   the inputs of energy_prolongation_smoother as the reference's own level-0 steps produced them (A, the
                  strength matrix Atilde, the tentative prolongator T, the coarse candidates B_c, the fine candidates B)
                  and, per option set s<q>: the options, the sparsity pattern, BtBinv, the returned P, <R, Z> / alpha /
                  beta of every iteration (read from the frame of cg_prolongation_smoothing while it runs) and the calls
                  into the native module (pyamg.amg_core wrapped): arguments before, the output array after.  Arrays a
                  call shares with an earlier call or with the inputs are stored once.  calc_BtB is kept for every
                  option set; the calls of the CG iteration are kept where CALLS says so (the small problems: on the
                  40 x 40 grids they would exceed the size of the largest file of tests/golden/evolution/).
  hier_*.npz      two SA hierarchies with their solves in the hier_*.npz layout of oracle/gen_golden.py

ref_env fakes scipy.linalg.calc_lwork as an empty module; the reference's pinv_array needs calc_lwork.gelss for more
than one candidate, so this tool installs that alias onto scipy's own <prefix>gelss_lwork.

Asserted, with the margins printed: the break decision (<R, Z> against tol) sits a relative 1e-3 from tol; no stored
block of a reference P has its largest magnitude below 1e-10 of P's largest; for the hierarchy fixtures, rebuilding
with every P perturbed by a relative 1e-10 changes neither level sizes nor aggregates.
Usage:  make -C oracle ref && python tools/gen_golden_energy.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_env  # noqa: E402
import gen_golden  # noqa: E402
import golden_io  # noqa: E402
import gen_golden_evolution as gge  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "energy")
LIMIT = 422266                  # the largest file of tests/golden/evolution/
BREAK_GAP = 1e-3
BLOCK_FLOOR = 1e-10
np.mat = np.asmatrix

ARGS = {"incomplete_mat_mult_bsr": ("Ap", "Aj", "Ax", "Bp", "Bj", "Bx", "Sp", "Sj", "Sx", "n_brow", "n_bcol", "brow_A", "bcol_A",
                                    "bcol_B"),
        "satisfy_constraints_helper": ("RowsPerBlock", "ColsPerBlock", "num_block_rows", "NullDim", "x", "y", "z", "Sp", "Sj", "Sx"),
        "calc_BtB": ("NullDim", "Nnodes", "ColsPerBlock", "b", "BsqCols", "x", "Sp", "Sj")}
OUTPUT = {"incomplete_mat_mult_bsr": "Sx", "satisfy_constraints_helper": "Sx", "calc_BtB": "x"}


def install_lwork_alias():
    import scipy.linalg
    import scipy.linalg.lapack as lapack

    def gelss(prefix, m, n, nrhs):
        dtype = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}[prefix]
        routine, = lapack.get_lapack_funcs(("gelss_lwork",), (np.ones((1,), dtype=dtype),))
        return None, lapack._compute_lwork(routine, m, n, nrhs)
    scipy.linalg.calc_lwork.gelss = gelss


class Recorder(object):
    """stands in for pyamg.amg_core: forwards everything, keeps the arguments and results of the three helpers"""

    def __init__(self, core):
        self._core = core
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._core, name)
        if name not in ARGS:
            return fn

        def wrapped(*args):
            before = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
            fn(*args)
            out_at = ARGS[name].index(OUTPUT[name])
            self.calls.append((name, before, np.array(args[out_at], copy=True)))
        return wrapped


class Store(object):
    """arrays by key, equal arrays once: a later key holds the name of the earlier one"""

    def __init__(self):
        self.out = {}
        self.seen = {}

    def put(self, key, v):
        v = np.asarray(v)
        if v.ndim == 0 or v.size < 8:
            self.out[key] = v
            return
        h = (hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest(), str(v.dtype), v.shape)
        if h in self.seen:
            self.out[key] = np.array("=" + self.seen[h])
        else:
            self.seen[h] = key
            self.out[key] = v


def trace_cg(fn):
    """run fn(); -> (result, [(newsum, alpha, beta)] per started iteration) read from cg_prolongation_smoothing's frame"""
    snaps = []

    def local(frame, event, arg):
        if event == "line":
            loc = frame.f_locals
            if "i" in loc and "newsum" in loc:
                s = (int(loc["i"]), float(loc["newsum"]), float(loc.get("alpha", np.nan)), float(loc.get("beta", np.nan)))
                if not snaps or snaps[-1] != s:
                    snaps.append(s)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code.co_name == "cg_prolongation_smoothing" else None
    sys.settrace(tracer)
    try:
        result = fn()
    finally:
        sys.settrace(None)
    rows = []
    started = sorted(set(s[0] for s in snaps))
    for q in started:
        mine = [s for s in snaps if s[0] == q]
        newsum = mine[-1][1]
        after = [s for s in snaps if s[0] == q + 1]
        finished = bool(after)
        # alpha of iteration q is what the frame holds when i has become q + 1; beta of iteration q >= 1 is set within it
        alpha = after[0][2] if finished else np.nan
        beta = mine[-1][3] if q >= 1 and finished else np.nan
        if not finished and len(mine) and q == started[-1] and len(rows) and mine[-1][1] == rows[-1][0]:
            continue                                        # the loop ended on maxiter: no new <R, Z>
        rows.append((newsum, alpha, beta))
    return result, np.array(rows, dtype=np.float64).reshape(-1, 3)


def level0_inputs(pyamg, A, B, strength):
    """the reference's own steps ahead of the smoother (aggregation.py:322-376) -> Atilde, T, B_c"""
    from pyamg.strength import symmetric_strength_of_connection, evolution_strength_of_connection
    from pyamg.aggregation.aggregate import standard_aggregation
    from pyamg.aggregation.tentative import fit_candidates
    np.random.seed(0)
    if isinstance(strength, str) and strength == "symmetric":
        C = symmetric_strength_of_connection(A.copy())
    elif isinstance(strength, str) and strength == "evolution":
        C = evolution_strength_of_connection(A.copy(), np.array(B, copy=True), k=2, epsilon=4.0)
    else:
        C = strength
    C = sps.csr_matrix(C)
    AggOp = standard_aggregation(C)[0]
    T, Bc = fit_candidates(AggOp, np.array(B, copy=True))
    return C, sps.bsr_matrix(T), np.asarray(Bc, dtype=np.float64)


def put_matrix(st, key, M):
    st.put(key + "_indptr", M.indptr.astype(np.intc))
    st.put(key + "_indices", M.indices.astype(np.intc))
    st.put(key + "_data", np.asarray(M.data, dtype=np.float64).ravel())
    st.out[key + "_shape"] = np.array(M.shape, dtype=np.int64)
    st.out[key + "_blocksize"] = np.array(getattr(M, "blocksize", (1, 1)), dtype=np.int64)


def gen_problem(pyamg, name, A, B, strength, option_sets, calls):
    import pyamg.aggregation.smooth as rsm
    import pyamg.util.utils as rut
    import pyamg
    C, T, Bc = level0_inputs(pyamg, A, B, strength)
    st = Store()
    put_matrix(st, "A", A)
    put_matrix(st, "Atilde", C)
    put_matrix(st, "T", T)
    st.put("Bc", Bc)
    st.put("B", np.asarray(B, dtype=np.float64))
    margins = []
    sets = []
    for q, opt in enumerate(option_sets):
        rec = Recorder(pyamg.amg_core)
        keep = pyamg.amg_core
        pyamg.amg_core = rec
        rsm.pyamg.amg_core = rec
        rut.pyamg.amg_core = rec
        try:
            Tin = T.copy()                                  # the reference sorts T and drops its zero blocks in place
            P, trace = trace_cg(lambda: rsm.energy_prolongation_smoother(A.copy(), Tin, C.copy(), Bc.copy(), None, (False, {}),
                                                                         krylov="cg", **opt))
        finally:
            pyamg.amg_core = keep
            rsm.pyamg.amg_core = keep
            rut.pyamg.amg_core = keep
        P = sps.bsr_matrix(P)
        pre = "s%d_" % q
        put_matrix(st, pre + "P", P)
        st.put(pre + "trace", trace)
        btb = [c for c in rec.calls if c[0] == "calc_BtB"]
        assert len(btb) == 1
        nd = Bc.shape[1]
        # BtBinv as compute_BtBinv returns it, rebuilt by the reference's own function on the recorded pattern
        Sp, Sj = btb[0][1][6], btb[0][1][7]
        pat = sps.bsr_matrix((np.ones((len(Sj),) + T.blocksize), Sj, Sp), shape=T.shape)
        st.put(pre + "pattern_indptr", Sp)
        st.put(pre + "pattern_indices", Sj)
        st.put(pre + "BtBinv", np.asarray(rut.compute_BtBinv(Bc.copy(), pat), dtype=np.float64).ravel())
        names = []
        for ci, (cname, before, after) in enumerate(c for c in rec.calls if calls or c[0] == "calc_BtB"):
            for arg, v in zip(ARGS[cname], before):
                st.put("%scall%d__%s" % (pre, ci, arg), v)
            st.put("%scall%d__out" % (pre, ci), after)
            names.append(cname)
        st.out[pre + "calls"] = np.array(names, dtype="U40")
        sets.append(opt)
        # margins: the break decision and the smallest block
        tol = opt.get("tol", 1e-8)
        gap = np.min(np.abs(trace[:, 0] - tol) / tol) if len(trace) else np.inf
        assert gap >= BREAK_GAP, "%s %r: <R, Z> within %g of tol: %r" % (name, opt, BREAK_GAP, trace[:, 0])
        blockmax = np.abs(P.data).reshape(P.data.shape[0], -1).max(axis=1)
        floor = blockmax.min() / np.abs(P.data).max()
        assert floor >= BLOCK_FLOOR, "%s %r: a stored block of P at %g of the largest" % (name, opt, floor)
        cons = np.abs(P * Bc - np.asarray(B)).max()
        margins.append((gap, floor))
        print("%-28s %-58s its=%d blocks=%d break gap %.2e smallest block %.2e |P Bc - B| %.1e <R,Z> %s"
              % (name, json.dumps(opt, sort_keys=True), int(np.sum(~np.isnan(trace[:, 1]))), len(P.indices), gap, floor, cons,
                 " ".join("%.3e" % v for v in trace[:, 0])))
    st.out["options_json"] = np.array(json.dumps(sets))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **st.out)
    size = os.path.getsize(path)
    assert size <= LIMIT, "%s: %d bytes" % (path, size)
    print("%-28s %6.0f KB" % (name, size / 1024))


def elasticity_2d(pyamg):
    from pyamg.gallery import linear_elasticity
    A, B = linear_elasticity((12, 12))
    A = sps.bsr_matrix(A, blocksize=(2, 2)); A.sort_indices()
    return A, np.asarray(B, dtype=np.float64)


def c5_elasticity():
    """the 3 x 3-block operator and its 6 candidates of the hier_c5_elas_p1_cube_* fixtures"""
    g = golden_io.load_hier("c5_elas_p1_cube_bgs")
    A = sps.bsr_matrix(g["levels"][0]["A"], blocksize=(3, 3)); A.sort_indices()
    z = np.load(os.path.join(golden_io.GOLDEN, "hier_c5_elas_p1_cube_bgs.npz"), allow_pickle=False)
    return A, np.asarray(z["B0"], dtype=np.float64)


def random_spd(seed=7, n=150):
    """random sparse SPD operator; its strength matrix gets an empty row (row 9) and the candidate zero entries on a
    whole aggregate, so that a 1 x 1 BtB of 0 meets the zero rule of pinv_array"""
    rng = np.random.RandomState(seed)
    M = sps.random(n, n, density=0.03, random_state=rng, format="csr", data_rvs=lambda s: rng.uniform(-1.0, -0.1, s))
    M = sps.csr_matrix(M + M.T)
    M.setdiag(0.0); M.eliminate_zeros()
    A = sps.csr_matrix(M + sps.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 0.5))
    A.sort_indices()
    A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
    return A


def perturbed_rebuild_is_stable(pyamg, A, build, B=None):
    """level sizes and aggregates of a rebuild in which every smoothed P is perturbed by a relative 1e-10"""
    import pyamg.aggregation.aggregation as ragg
    real = ragg.energy_prolongation_smoother
    sizes = []
    for perturb in (False, True):
        rng = np.random.RandomState(11)

        def smoother(*a, **k):
            P = real(*a, **k)
            if perturb:
                P = P.copy()
                P.data = P.data * (1.0 + 1e-10 * rng.uniform(-1.0, 1.0, P.data.shape))
            return P
        ragg.energy_prolongation_smoother = smoother
        try:
            np.random.seed(0)
            kw = {} if B is None else {"B": B}
            ml = build(A, keep=True, **kw)
        finally:
            ragg.energy_prolongation_smoother = real
        sizes.append([(lvl.A.shape[0], None if not hasattr(lvl, "AggOp") else sps.csr_matrix(lvl.AggOp).indices.tobytes())
                      for lvl in ml.levels])
    return sizes[0] == sizes[1], [s[0] for s in sizes[0]]


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    install_lwork_alias()
    std = [dict(maxiter=4, degree=1, weighting="local"), dict(maxiter=8, degree=1, weighting="diagonal"),
           dict(maxiter=4, degree=2, weighting="local"), dict(maxiter=4, degree=0, weighting="local")]
    A40 = gge.anisotropic(pyamg, 40, 40, 0.01, np.pi / 6)
    ones = lambda A: np.ones((A.shape[0], 1))
    # tol = 0.5 lies between the <R, Z> of iterations 1 and 2 of both 40 x 40 runs (printed): the break fires at iteration 2
    gen_problem(pyamg, "aniso_40x40_symmetric", A40, ones(A40), "symmetric", std + [dict(maxiter=6, degree=1, weighting="local", tol=0.5)],
                calls=False)
    gen_problem(pyamg, "aniso_40x40_evolution", A40, ones(A40), "evolution", std + [dict(maxiter=6, degree=1, weighting="local", tol=0.5)],
                calls=False)
    A17 = gge.anisotropic(pyamg, 17, 23, 0.001, np.pi / 4)
    gen_problem(pyamg, "aniso_17x23", A17, ones(A17), "symmetric", std[:1] + std[2:3], calls=True)
    Ae, Be = elasticity_2d(pyamg)
    gen_problem(pyamg, "elasticity_12x12", Ae, Be, "symmetric", std[:1], calls=True)
    Ac, Bc = c5_elasticity()
    gen_problem(pyamg, "c5_elasticity", Ac, Bc, "symmetric", [dict(maxiter=1, degree=1, weighting="local")], calls=True)
    Ar = random_spd()
    Cr = sps.lil_matrix(sps.csr_matrix(abs(Ar)))
    Cr[9, :] = 0.0
    Cr = sps.csr_matrix(Cr); Cr.eliminate_zeros()
    assert Cr.indptr[10] == Cr.indptr[9]
    Br = np.ones((Ar.shape[0], 1))
    from pyamg.aggregation.aggregate import standard_aggregation
    agg = sps.csr_matrix(standard_aggregation(Cr)[0])
    aggc = agg.tocsc()
    Br[aggc.indices[aggc.indptr[2]:aggc.indptr[3]]] = 0.0    # one whole aggregate: its column of T and its B_c are zero
    gen_problem(pyamg, "random_spd_150", Ar, Br, Cr, [dict(maxiter=4, degree=0, weighting="local"), dict(maxiter=4, degree=1, weighting="diagonal")],
                calls=True)

    # two hierarchies with their solves
    gen_golden.OUT = OUT
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    energy = ("energy", {"krylov": "cg", "maxiter": 4, "degree": 1, "weighting": "local"})
    build_a = lambda A, **kw: pyamg.smoothed_aggregation_solver(A, strength=("evolution", {"k": 2, "epsilon": 4.0}), smooth=energy,
                                                                max_coarse=20, **kw)
    ok, sizes = perturbed_rebuild_is_stable(pyamg, A40, build_a)
    print("hier_sa_evolution_energy_2d: levels %r, stable under a 1e-10 perturbation of every P: %r" % (sizes, ok))
    assert ok
    gen_golden.gen_hier(pyamg, "sa_evolution_energy_2d", A40, build_a, gs, gs, dict(tol=1e-8))
    build_e = lambda A, **kw: pyamg.smoothed_aggregation_solver(A, smooth=energy, max_coarse=10, **kw)
    ok, sizes = perturbed_rebuild_is_stable(pyamg, Ae, build_e, B=Be)
    print("hier_elas_energy_2d: levels %r, stable under a 1e-10 perturbation of every P: %r" % (sizes, ok))
    assert ok
    gen_golden.gen_hier(pyamg, "elas_energy_2d", Ae, build_e, gs, gs, dict(tol=1e-8), B=Be)


if __name__ == "__main__":
    main()
