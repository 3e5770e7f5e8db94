"""Fixtures of the row-parallel classical setup stages -- tests/golden/classical/ (tools/gen_golden_classical.py) and
the classical_strength_* / rs_direct_interpolation_* cases of tests/golden/setup_kernels.npz -- with numpy models of the
two kernels written from the reference's text (amg_core/ruge_stuben.h:46-130, :497-595), and the replay of every
recorded call through an implementation: an object with strength, maximum, pass1 and pass2."""
import os

import numpy as np

import golden_io

DIR = os.path.join(golden_io.GOLDEN, "classical")
CASES = ("wide_257", "wide_257c", "branches", "unsorted")
CANONICAL = ("wide_257c",)              # operators the device routes of classical.py take
DBL_MIN = np.finfo(np.float64).tiny
_cache = {}


def same_bits(a, b):
    """array_equal on the raw bytes: NaN payloads and the sign of zero count"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def crafted(case):
    """-> (A = dict(Ap, Aj, Ax), calls = [(entry, inputs, outputs)]) with the operator and the S of an interpolation
    pass filled in, so that every call reads like the native one"""
    if case in _cache:
        return _cache[case]
    z = np.load(os.path.join(DIR, "%s.npz" % case), allow_pickle=False)
    A = _frozen({k: z[k] for k in ("Ap", "Aj", "Ax")})
    n = len(A["Ap"]) - 1
    calls = []
    for k, entry in enumerate(str(e) for e in z["calls"]):
        pre = "c%d__" % k
        outs = _frozen({f[len(pre):-4]: z[f] for f in z.files if f.startswith(pre) and f.endswith("_out")})
        if entry == "classical_strength_of_connection":
            ins = dict(n_row=n, theta=float(z[pre + "theta"]), **A)
        elif entry == "maximum_row_value":
            ins = dict(n_row=n, **A)
        else:
            S = calls[int(z[pre + "S"])][2]
            ins = dict(n_nodes=n, Sp=S["Sp"], Sj=S["Sj"])
            if entry == "rs_direct_interpolation_pass1":
                ins["splitting"] = z[pre + "splitting"]
            else:
                first = calls[int(z[pre + "pass1"])]
                ins.update(A, Sx=S["Sx"], splitting=first[1]["splitting"], Bp=first[2]["Bp"])
        calls.append((entry, _frozen(ins), outs))
    _cache[case] = (A, calls)
    return _cache[case]


def setup_cases(prefix):
    """the cases of setup_kernels.npz whose name starts with prefix: [(name, dict of arrays)]"""
    key = "setup:" + prefix
    if key not in _cache:
        z = np.load(os.path.join(golden_io.GOLDEN, "setup_kernels.npz"), allow_pickle=False)
        names = sorted({f.split("__")[0] for f in z.files if f.startswith(prefix)})
        _cache[key] = [(name, _frozen({f.split("__")[1]: z[f] for f in z.files if f.startswith(name + "__")})) for name in names]
    return _cache[key]


def strength_of(A, theta, impl):
    """impl.strength on a scipy CSR matrix"""
    return impl.strength(A.shape[0], theta, np.ascontiguousarray(A.indptr, np.intc), np.ascontiguousarray(A.indices, np.intc),
                         np.ascontiguousarray(A.data, np.float64))


# ------------------------------------------------------------------------------------------------ numpy models
class Model(object):
    """the two kernels and their small companions in numpy"""

    @staticmethod
    def maximum(n, Ap, Aj, Ax, skip_diagonal=False):
        rows = np.repeat(np.arange(n), np.diff(Ap[:n + 1]))
        use = (Aj[:len(rows)] != rows) if skip_diagonal else np.ones(len(rows), dtype=bool)
        m = np.full(n, DBL_MIN)
        np.fmax.at(m, rows[use], np.abs(Ax[:len(rows)][use]))           # like std::max(m, |a|): a NaN never replaces m
        return m

    @staticmethod
    def strength(n, theta, Ap, Aj, Ax):
        rows = np.repeat(np.arange(n), np.diff(Ap[:n + 1]))
        Aj, Ax = Aj[:len(rows)], Ax[:len(rows)]
        threshold = theta * Model.maximum(n, Ap, Aj, Ax, skip_diagonal=True)
        with np.errstate(invalid="ignore"):
            keep = (Aj == rows) | (np.abs(Ax) >= threshold[rows])
        Sp = np.zeros(n + 1, dtype=np.intc)
        np.cumsum(np.bincount(rows[keep], minlength=n), out=Sp[1:])
        return Sp, Aj[keep].astype(np.intc), Ax[keep].astype(np.float64)

    @staticmethod
    def pass1(n, Sp, Sj, splitting):
        rows = np.repeat(np.arange(n), np.diff(Sp[:n + 1]))
        Sj = Sj[:len(rows)]
        strong = (splitting[Sj] == 1) & (Sj != rows) & (splitting[rows] != 1)
        Bp = np.zeros(n + 1, dtype=np.intc)
        np.cumsum(np.where(splitting[:n] == 1, 1, np.bincount(rows[strong], minlength=n)), out=Bp[1:])
        return Bp

    @staticmethod
    def pass2(n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp):
        coarse = np.cumsum(splitting[:n]) - splitting[:n]
        Bj, Bx = np.zeros(Bp[n], dtype=np.intc), np.zeros(Bp[n], dtype=np.float64)
        zero = np.float64(0.0)
        with np.errstate(all="ignore"):
            for i in range(n):
                at = Bp[i]
                if splitting[i] == 1:
                    Bj[at], Bx[at] = coarse[i], 1.0
                    continue
                strong = [jj for jj in range(Sp[i], Sp[i + 1]) if splitting[Sj[jj]] == 1 and Sj[jj] != i]
                sp = sn = ap = an = diag = zero
                for jj in strong:
                    if Sx[jj] < 0: sn = sn + Sx[jj]
                    else: sp = sp + Sx[jj]
                for jj in range(Ap[i], Ap[i + 1]):
                    if Aj[jj] == i: diag = diag + Ax[jj]
                    elif Ax[jj] < 0: an = an + Ax[jj]
                    else: ap = ap + Ax[jj]
                alpha, beta = an / sn, ap / sp
                if sp == 0:
                    diag, beta = diag + ap, zero
                neg, pos = -alpha / diag, -beta / diag
                for jj in strong:
                    Bj[at], Bx[at] = coarse[Sj[jj]], (neg if Sx[jj] < 0 else pos) * Sx[jj]
                    at += 1
        return Bj, Bx


# ------------------------------------------------------------------------------------------------ replay
def replay(entry, ins, impl):
    """one recorded call through impl -> dict of outputs, named as the fixture names them"""
    a = ins
    if entry == "classical_strength_of_connection":
        return dict(zip(("Sp", "Sj", "Sx"), impl.strength(a["n_row"], a["theta"], a["Ap"], a["Aj"], a["Ax"])))
    if entry == "maximum_row_value":
        return {"x": impl.maximum(a["n_row"], a["Ap"], a["Aj"], a["Ax"])}
    if entry == "rs_direct_interpolation_pass1":
        return {"Bp": impl.pass1(a["n_nodes"], a["Sp"], a["Sj"], a["splitting"])}
    assert entry == "rs_direct_interpolation_pass2"
    return dict(zip(("Bj", "Bx"), impl.pass2(a["n_nodes"], a["Ap"], a["Aj"], a["Ax"], a["Sp"], a["Sj"], a["Sx"], a["splitting"],
                                             a["Bp"])))


def check_crafted(case, impl):
    """every recorded call of a crafted case, bit for bit; returns the entries seen"""
    seen = set()
    for k, (entry, ins, outs) in enumerate(crafted(case)[1]):
        got = replay(entry, ins, impl)
        for name, want in outs.items():
            assert same_bits(got[name], want), (case, k, entry, name)
        seen.add(entry)
    return seen


def check_setup_strength(impl, also_maximum=None):
    """the 15 classical_strength_* cases of setup_kernels.npz; also_maximum: a second implementation whose
    maximum_row_value is compared on the same operators"""
    cases = setup_cases("classical_strength_")
    assert len(cases) == 15
    for name, c in cases:
        Ap, Aj, Ax = c["Ap"].astype(np.intc), c["Aj"].astype(np.intc), c["Ax"].astype(np.float64)
        n = len(Ap) - 1
        Sp, Sj, Sx = impl.strength(n, float(c["theta"][0]), Ap, Aj, Ax)
        assert same_bits(Sp, c["Sp"].astype(np.intc)) and same_bits(Sj, c["Sj"].astype(np.intc)), name
        assert same_bits(Sx, c["Sx"].astype(np.float64)), name
        if also_maximum is not None:
            assert same_bits(impl.maximum(n, Ap, Aj, Ax), also_maximum.maximum(n, Ap, Aj, Ax)), name


def check_setup_interpolation(impl):
    """the 5 rs_direct_interpolation_* cases of setup_kernels.npz"""
    cases = setup_cases("rs_direct_interpolation_")
    assert len(cases) == 5
    for name, c in cases:
        Ap, Aj, Cp, Cj, spl = (c[k].astype(np.intc) for k in ("Ap", "Aj", "Cp", "Cj", "splitting"))
        Ax, Cx = c["Ax"].astype(np.float64), c["Cx"].astype(np.float64)
        n = len(Ap) - 1
        Pp = impl.pass1(n, Cp, Cj, spl)
        assert same_bits(Pp, c["Pp"].astype(np.intc)), name
        Pj, Px = impl.pass2(n, Ap, Aj, Ax, Cp, Cj, Cx, spl, Pp)
        assert same_bits(Pj, c["Pj"].astype(np.intc)) and same_bits(Px, c["Px"].astype(np.float64)), name


# ------------------------------------------------------------------------------------------------ operators
def operator(name):
    """the canonical operators of the route comparisons: 'poisson_17x23', 'aniso_40x40' (whose recorded strength
    matrices are splitting_io.problem(name)['S']) and the crafted 'wide_257c'"""
    import scipy.sparse as sps

    import evolution_io
    import splitting_io
    if name == "poisson_17x23":
        return splitting_io.poisson2d(17, 23)
    if name == "aniso_40x40":
        A = sps.csr_matrix(evolution_io.problem(name)["A"], copy=True)
    else:
        c = crafted(name)[0]
        A = sps.csr_matrix((c["Ax"].copy(), c["Aj"].copy(), c["Ap"].copy()), shape=(len(c["Ap"]) - 1,) * 2)
    A.indices, A.indptr = A.indices.astype(np.intc), A.indptr.astype(np.intc)
    assert A.has_canonical_format and np.all(A.data != 0)
    return A


def same_csr(M, G):
    return M.shape == G.shape and same_bits(M.indptr, G.indptr.astype(M.indptr.dtype)) and \
        same_bits(M.indices, G.indices.astype(M.indices.dtype)) and same_bits(M.data, G.data)


def same_hierarchy(ml, ref, keys=("A", "P", "R", "C", "splitting")):
    """level sizes and the named members of every level, bit for bit"""
    assert [l.A.shape for l in ml.levels] == [l.A.shape for l in ref.levels]
    for k, (a, b) in enumerate(zip(ml.levels, ref.levels)):
        for key in keys:
            assert hasattr(a, key) == hasattr(b, key), (k, key)
            if not hasattr(b, key):
                continue
            if key == "splitting":
                assert same_bits(a.splitting, b.splitting), (k, key)
            else:
                assert same_csr(getattr(a, key), getattr(b, key)), (k, key)
