#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the root-node energy smoothing fixtures.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on its own native module oracle/_ref/_amg_core.so, with the
calc_lwork.gelss alias of tools/gen_golden_energy.py -- and records under tests/golden/rootnode/:

  <problem>.npz       the inputs of the root-node smoother as the reference's own level-0 steps produce them (A, Atilde,
                      AggOp, Cnodes, T before and after scale_T, B_c, B_f, the five members of Cpt_params) and per option
                      set s<q>: the options, the pattern and BtBinv of every pass (a post-filter makes two), T after the
                      initial fit where one runs, the returned P, the CG trace of every pass and the calls into the native
                      module that the filters and compute_BtBinv make (truncate_rows_csr, classical_strength_of_connection,
                      calc_BtB): arguments before, outputs after.  The calls of the CG iteration itself are not kept: the
                      fixtures of tests/golden/energy/ hold those kernels.
  truncate_rows.npz   crafted inputs of truncate_rows_csr (ties, sorted rows, lengths 0, 1, k, k + 1, 65, 300) with the
                      reference's output
  hier_*.npz          three root-node hierarchies with their solves in the hier_*.npz layout of oracle/gen_golden.py,
                      plus the root dofs of every level (Cpts<l>)

Asserted, with the margins printed: <R, Z> a relative 1e-3 from tol in every pass; no stored block of a P below 1e-10 of
its largest; every post-filter decision (k-th against (k+1)-th magnitude, every magnitude against theta * max) at least
1e-6 of the row maximum wide; the hierarchies keep level sizes and aggregates when every P is perturbed by 1e-10.
Usage:  make -C oracle ref && python tools/gen_golden_rootnode.py
"""
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
import gen_golden_evolution as gge  # noqa: E402
import gen_golden_energy as gen  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rootnode")
LIMIT = gen.LIMIT
FILTER_GAP = 1e-6
np.mat = np.asmatrix

ARGS = {"truncate_rows_csr": ("n_row", "k", "Sp", "Sj", "Sx"),
        "classical_strength_of_connection": ("n_row", "theta", "Ap", "Aj", "Ax", "Sp", "Sj", "Sx"),
        "calc_BtB": ("NullDim", "Nnodes", "ColsPerBlock", "b", "BsqCols", "x", "Sp", "Sj")}
OUTPUTS = {"truncate_rows_csr": ("Sj", "Sx"), "classical_strength_of_connection": ("Sp", "Sj", "Sx"), "calc_BtB": ("x",)}


class Recorder(object):
    """stands in for pyamg.amg_core: forwards everything, keeps arguments and outputs of the entries of ARGS"""

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
            after = {o: np.array(args[ARGS[name].index(o)], copy=True) for o in OUTPUTS[name]}
            self.calls.append((name, before, after))
        return wrapped


def filter_margin(M, key, value):
    """the narrowest decision of a scalar-row filter of M, relative to the row maximum"""
    M = sps.csr_matrix(M.tocsr())
    worst = np.inf
    for i in range(M.shape[0]):
        m = np.sort(np.abs(M.data[M.indptr[i]:M.indptr[i + 1]]))[::-1]
        if len(m) == 0 or m[0] == 0.0:
            continue
        if key == "k":
            if len(m) > value and not (m[value - 1] == 0.0 and m[value] == 0.0):
                worst = min(worst, (m[value - 1] - m[value]) / m[0])
        else:
            worst = min(worst, np.abs(m - value * m[0]).min() / m[0])
    return worst


def level0_inputs(A, B, strength):
    from pyamg.strength import symmetric_strength_of_connection
    from pyamg.aggregation.aggregate import standard_aggregation
    from pyamg.aggregation.tentative import fit_candidates
    from pyamg.util.utils import get_Cpt_params, scale_T
    bs = A.blocksize[0] if sps.isspmatrix_bsr(A) else 1
    C = symmetric_strength_of_connection(A.copy()) if isinstance(strength, str) else strength
    C = sps.csr_matrix(C)
    AggOp, Cnodes = standard_aggregation(C)
    AggOp = sps.csr_matrix(AggOp)
    T0, _ = fit_candidates(AggOp, np.array(B[:, :bs], copy=True))
    T0 = sps.bsr_matrix(T0)
    params = get_Cpt_params(A, Cnodes, AggOp, T0)
    T = sps.bsr_matrix(scale_T(T0.copy(), params["P_I"], params["I_F"]))
    Bc = np.asarray(params["P_I"].T * B, dtype=np.float64)
    return C, AggOp, np.asarray(Cnodes), T0, T, params, Bc


def gen_problem(pyamg, name, A, B, strength, option_sets):
    import pyamg.aggregation.smooth as rsm
    import pyamg.util.utils as rut
    C, AggOp, Cnodes, T0, T, params, Bc = level0_inputs(A, B, strength)
    st = gen.Store()
    for key, M in (("A", A), ("Atilde", C), ("T0", T0), ("T", T), ("P_I", params["P_I"]), ("I_F", params["I_F"]),
                   ("I_C", params["I_C"])):
        gen.put_matrix(st, key, M)
    st.put("AggOp_indptr", AggOp.indptr.astype(np.intc)); st.put("AggOp_indices", AggOp.indices.astype(np.intc))
    st.out["AggOp_shape"] = np.array(AggOp.shape, dtype=np.int64)
    st.put("Cnodes", Cnodes.astype(np.int64)); st.put("Cpts", params["Cpts"].astype(np.int64)); st.put("Fpts", params["Fpts"].astype(np.int64))
    st.put("Bc", Bc); st.put("B", np.asarray(B, dtype=np.float64))
    sets = []
    for q, opt in enumerate(option_sets):
        rec = Recorder(pyamg.amg_core)
        keep_core = pyamg.amg_core
        real_cg, real_fit, real_tr, real_fm = rsm.cg_prolongation_smoothing, rsm.filter_operator, rsm.truncate_rows, rsm.filter_matrix_rows
        traces, fits, post = [], [], []

        def cg(*a, **k):
            out, tr = gen.trace_cg(lambda: real_cg(*a, **k))
            traces.append(tr)
            return out

        def fit(*a, **k):
            out = real_fit(*a, **k)
            fits.append(sps.bsr_matrix(params["I_F"] * out + params["P_I"]))
            return out

        def tr_rows(M, k):
            if traces:
                post.append(("k", k, M.copy()))
            return real_tr(M, k)

        def fm_rows(M, theta):
            if traces:
                post.append(("theta", theta, M.copy()))
            return real_fm(M, theta)
        pyamg.amg_core = rec; rsm.pyamg.amg_core = rec; rut.pyamg.amg_core = rec
        rsm.cg_prolongation_smoothing, rsm.filter_operator, rsm.truncate_rows, rsm.filter_matrix_rows = cg, fit, tr_rows, fm_rows
        try:
            P = rsm.energy_prolongation_smoother(A.copy(), T.copy(), C.copy(), Bc.copy(), np.array(B, copy=True), (True, params),
                                                 krylov="cg", **opt)
        finally:
            pyamg.amg_core = keep_core; rsm.pyamg.amg_core = keep_core; rut.pyamg.amg_core = keep_core
            rsm.cg_prolongation_smoothing, rsm.filter_operator, rsm.truncate_rows, rsm.filter_matrix_rows = real_cg, real_fit, real_tr, real_fm
        P = sps.bsr_matrix(P)
        pre = "s%d_" % q
        gen.put_matrix(st, pre + "P", P)
        st.put(pre + "trace", np.concatenate(traces) if traces else np.zeros((0, 3)))
        st.out[pre + "trace_lengths"] = np.array([len(t) for t in traces], dtype=np.int64)
        btb = [c for c in rec.calls if c[0] == "calc_BtB"]
        assert len(btb) == len(traces) == (2 if opt.get("postfilter") else 1)
        for pi, call in enumerate(btb):
            Sp, Sj = call[1][6], call[1][7]
            pat = sps.bsr_matrix((np.ones((len(Sj),) + T.blocksize), Sj, Sp), shape=T.shape)
            st.put("%spass%d_pattern_indptr" % (pre, pi), Sp)
            st.put("%spass%d_pattern_indices" % (pre, pi), Sj)
            st.put("%spass%d_BtBinv" % (pre, pi), np.asarray(rut.compute_BtBinv(Bc.copy(), pat), dtype=np.float64).ravel())
        st.out[pre + "n_fits"] = np.array(len(fits))
        for fi, F in enumerate(fits):
            gen.put_matrix(st, "%sfit%d" % (pre, fi), F)
        names = []
        for ci, (cname, before, after) in enumerate(rec.calls):
            for arg, v in zip(ARGS[cname], before):
                st.put("%scall%d__%s" % (pre, ci, arg), v)
            for o, v in after.items():
                st.put("%scall%d__out_%s" % (pre, ci, o), v)
            names.append(cname)
        st.out[pre + "calls"] = np.array(names, dtype="U40")
        sets.append(opt)
        gaps = []
        for pi, tr in enumerate(traces):
            tol = opt.get("tol", 1e-8) if pi == 0 else 1e-8
            gaps.append(np.min(np.abs(tr[:, 0] - tol) / tol) if len(tr) else np.inf)
        assert min(gaps) >= gen.BREAK_GAP, "%s %r: <R, Z> within %g of tol" % (name, opt, gen.BREAK_GAP)
        blockmax = np.abs(P.data).reshape(P.data.shape[0], -1).max(axis=1)
        floor = blockmax.min() / np.abs(P.data).max()
        assert floor >= gen.BLOCK_FLOOR, "%s %r: a stored block of P at %g of the largest" % (name, opt, floor)
        fgap = min([filter_margin(M, key, v) for key, v, M in post] + [np.inf])
        assert fgap >= FILTER_GAP, "%s %r: a post-filter decision only %g of the row maximum wide" % (name, opt, fgap)
        Cp = params["Cpts"]
        Pc = sps.csr_matrix(P)[Cp]
        assert (Pc != sps.eye(len(Cp), format="csr")).nnz == 0, "rows at Cpts are not the identity"
        print("%-18s %-92s passes=%d fits=%d blocks=%d break gap %.2e smallest block %.2e filter gap %.2e |P Bc - B| %.1e"
              % (name, json.dumps(opt, sort_keys=True), len(traces), len(fits), len(P.indices), min(gaps), floor, fgap,
                 np.abs(P * Bc - np.asarray(B)).max()))
    st.out["options_json"] = np.array(json.dumps(sets))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **st.out)
    size = os.path.getsize(path)
    assert size <= LIMIT, "%s: %d bytes" % (path, size)
    print("%-18s %6.0f KB" % (name, size / 1024))


def gen_truncate(core, k=4):
    rng = np.random.RandomState(3)
    rows = [np.zeros(0), np.array([2.0]), rng.uniform(-1, 1, k), rng.uniform(-1, 1, k + 1), np.full(9, 3.0), np.full(k + 1, -1.0),
            np.arange(1.0, 12.0), np.arange(12.0, 1.0, -1.0), rng.randint(1, 4, 65).astype(float), rng.uniform(-1, 1, 65),
            rng.randint(1, 6, 300).astype(float) * rng.choice([-1.0, 1.0], 300), rng.uniform(-1, 1, 300),
            np.array([1.0, 2.0, 2.0, 1.0, 2.0, 1.0, 2.0]), np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0])]
    Sp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.intc)
    Sj = np.concatenate([rng.permutation(len(r)) for r in rows]).astype(np.intc)
    Sx = np.concatenate(rows)
    out = {"Sp": Sp, "Sj": Sj, "Sx": Sx, "ks": np.array([0, 1, 2, k, 64, 400], dtype=np.int64)}
    for kk in out["ks"]:
        j, x = Sj.copy(), Sx.copy()
        core.truncate_rows_csr(len(rows), int(kk), Sp, j, x)
        out["k%d_Sj" % kk], out["k%d_Sx" % kk] = j, x
    np.savez_compressed(os.path.join(OUT, "truncate_rows.npz"), **out)
    print("truncate_rows      %d rows, k in %r" % (len(rows), list(out["ks"])))


def stable_rebuild(build, A, **kw):
    """level sizes and aggregates of a rebuild in which every smoothed P is perturbed by a relative 1e-10"""
    import pyamg.aggregation.rootnode as rrn
    real = rrn.energy_prolongation_smoother
    seen = []
    for perturb in (False, True):
        rng = np.random.RandomState(11)

        def smoother(*a, **k):
            P = real(*a, **k)
            if perturb:
                P = P.copy()
                P.data = P.data * (1.0 + 1e-10 * rng.uniform(-1.0, 1.0, P.data.shape))
            return P
        rrn.energy_prolongation_smoother = smoother
        try:
            np.random.seed(0)
            ml = build(A, keep=True, **kw)
        finally:
            rrn.energy_prolongation_smoother = real
        seen.append([(lvl.A.shape[0], None if not hasattr(lvl, "AggOp") else sps.csr_matrix(lvl.AggOp).indices.tobytes())
                     for lvl in ml.levels])
    return seen[0] == seen[1], [s[0] for s in seen[0]]


def gen_hierarchy(pyamg, name, A, build, sizes, cycles, B=None):
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    kw = {} if B is None else {"B": B}
    ok, got = stable_rebuild(build, A, **kw)
    print("hier_%s: levels %r, stable under a 1e-10 perturbation of every P: %r" % (name, got, ok))
    assert ok and got == sizes, (got, sizes)
    kept = {}

    def build_and_keep(A, **k):
        kept["ml"] = build(A, **k)
        return kept["ml"]
    gen_golden.gen_hier(pyamg, name, A, build_and_keep, gs, gs, dict(tol=1e-8), B=B)
    path = os.path.join(OUT, "hier_%s.npz" % name)
    z = dict(np.load(path, allow_pickle=False))
    assert len(z["residuals"]) - 1 == cycles, (len(z["residuals"]) - 1, cycles)
    for li, lvl in enumerate(kept["ml"].levels[:-1]):
        z["Cpts%d" % li] = np.asarray(lvl.Cpts, dtype=np.int64)
        Pc = sps.csr_matrix(lvl.P)[lvl.Cpts]
        assert (Pc != sps.eye(len(lvl.Cpts), format="csr")).nnz == 0
    np.savez_compressed(path, **z)
    assert os.path.getsize(path) <= LIMIT, path


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    gen.install_lwork_alias()
    from pyamg.aggregation.rootnode import rootnode_solver
    ones = lambda A: np.ones((A.shape[0], 1))
    base = dict(maxiter=4, degree=2, weighting="local")
    A17 = gge.anisotropic(pyamg, 17, 23, 0.001, np.pi / 4)
    gen_problem(pyamg, "aniso_17x23", A17, ones(A17), "symmetric",
                [dict(maxiter=4, degree=1, weighting="local"), dict(base), dict(base, prefilter={"k": 3}),
                 dict(base, postfilter={"theta": 0.1}), dict(base, postfilter={"k": 4, "theta": 0.2})])
    Ae, Be = gen.elasticity_2d(pyamg)
    gen_problem(pyamg, "elasticity_12x12", Ae, Be, "symmetric",
                [dict(maxiter=4, degree=1, weighting="local"), dict(maxiter=4, degree=1, weighting="local", postfilter={"k": 6})])
    Ac, Bc = gen.c5_elasticity()
    gen_problem(pyamg, "c5_elasticity", Ac, Bc, "symmetric", [dict(maxiter=1, degree=1, weighting="local")])
    Ar = gen.random_spd()
    Cr = sps.lil_matrix(sps.csr_matrix(abs(Ar)))
    Cr[9, :] = 0.0
    Cr = sps.csr_matrix(Cr); Cr.eliminate_zeros()
    gen_problem(pyamg, "random_spd_150", Ar, ones(Ar), Cr,
                [dict(maxiter=4, degree=0, weighting="local"), dict(maxiter=4, degree=1, weighting="diagonal")])
    gen_truncate(pyamg.amg_core)

    gen_golden.OUT = OUT
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    A40 = gge.anisotropic(pyamg, 40, 40, 0.01, np.pi / 6)
    ev = ("evolution", {"k": 2, "epsilon": 4.0})
    energy = ("energy", {"krylov": "cg", "maxiter": 4, "degree": 2, "weighting": "local", "postfilter": {"theta": 0.1}})
    gen_hierarchy(pyamg, "rootnode_ev_d2_post", A40, lambda A, **kw: rootnode_solver(A, strength=ev, smooth=energy, max_coarse=20, **kw),
                  [1600, 280, 90, 24, 4], 17)
    gen_hierarchy(pyamg, "rootnode_default", A40, lambda A, **kw: rootnode_solver(A, max_coarse=20, **kw), [1600, 196, 25, 4], 43)
    gen_hierarchy(pyamg, "rootnode_elas", Ae, lambda A, **kw: rootnode_solver(A, max_coarse=10, **kw), [288, 32, 6], 12, B=Be)


if __name__ == "__main__":
    main()
