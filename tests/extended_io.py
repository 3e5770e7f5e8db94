"""Extended+i interpolation: a pure-Python model of the definition -- dicts and Python floats, the
operations in the stated order, so that its results are compared bit for bit -- and the designed cases that the host
tests and the GPU tests share.  A case is (A, S, splitting) as scipy CSR matrices and an int32 array, together with a
check that the branch it was designed for is taken."""
import math

import numpy as np
import scipy.sparse as sps

import classical_io as cio
import splitting_io as sio

_cache = {}


# ------------------------------------------------------------------------------------------------ the model
def _rows(M):
    """-> per row the stored entries [(column, value)] in stored order"""
    p, j, x = M.indptr, M.indices, M.data
    return [[(int(j[e]), float(x[e])) for e in range(p[i], p[i + 1])] for i in range(M.shape[0])]


def _bar(akk, v):
    return v if ((akk >= 0 and v < 0) or (akk < 0 and v > 0)) else 0.0


def _div(a, b):
    """IEEE division of Python floats, with 0 denominators"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def sets(S_rows, splitting, i):
    """-> (Cs_i, Fs_i, C_hat) of F row i"""
    Si = [j for j, _ in S_rows[i] if j != i]
    Cs = [j for j in Si if splitting[j] == 1]
    Fs = [j for j in Si if splitting[j] == 0]
    chat = set(Cs)
    for k in Fs:
        chat.update(l for l, _ in S_rows[k] if l != k and splitting[l] == 1)
    return Cs, Fs, sorted(chat)


def model(A, S, splitting, max_per_row=None, trace=None):
    """-> (Pp, Pj, Px) as numpy arrays.  trace: a dict that receives, per F row, what the branches were: 'lumped'
    (strong F neighbours with d_k == 0), 'filtered' (entries the sign filter dropped), 'truncated'."""
    n = A.shape[0]
    A_rows, S_rows = _rows(A), _rows(S)
    for rows in (A_rows, S_rows):
        for r in rows:
            assert len({j for j, _ in r}) == len(r), "duplicate columns"
    a = [dict(r) for r in A_rows]
    cidx = np.cumsum(splitting) - splitting
    Pp, Pj, Px = [0], [], []
    for i in range(n):
        if splitting[i] == 1:
            cols, vals = [int(cidx[i])], [1.0]
        else:
            Cs, Fs, chat = sets(S_rows, splitting, i)
            inhat, fs = set(chat), set(Fs)
            info = {"lumped": [], "filtered": 0, "chat": chat, "Cs": Cs, "Fs": Fs}
            D = a[i].get(i, 0.0)
            for j, v in A_rows[i]:
                if j != i and j not in inhat and j not in fs:
                    D = D + v
            w = [a[i].get(c, 0.0) for c in chat]
            at = {c: t for t, c in enumerate(chat)}
            for k in Fs:
                akk = a[k].get(k, 0.0)
                d = 0.0
                for l, v in A_rows[k]:
                    if l == i or l in inhat:
                        d = d + _bar(akk, v)
                aik = a[i].get(k, 0.0)
                if d == 0.0:
                    D = D + aik
                    info["lumped"].append(k)
                    continue
                for l, v in A_rows[k]:
                    if _bar(akk, v) != 0.0:
                        c = _div(aik * v, d)
                        if l == i:
                            D = D + c
                        elif l in inhat:
                            w[at[l]] = w[at[l]] + c
                    elif l == i or l in inhat:
                        info["filtered"] += 1
            cols, vals = [int(cidx[c]) for c in chat], [_div(-wt, D) for wt in w]
            q = max_per_row
            info["truncated"] = False
            if q is not None and len(vals) > q and all(math.isfinite(v) for v in vals):
                info["truncated"] = True
                order = sorted(range(len(vals)), key=lambda t: (-abs(vals[t]), t))[:q]
                kept = sorted(order)
                s_all = s_kept = 0.0
                for v in vals:
                    s_all = s_all + v
                for t in kept:
                    s_kept = s_kept + vals[t]
                info["s_kept"] = s_kept
                scale = _div(s_all, s_kept) if s_kept != 0.0 else None
                cols = [cols[t] for t in kept]
                vals = [vals[t] * scale if scale is not None else vals[t] for t in kept]
            if trace is not None:
                trace[i] = info
        Pj.extend(cols); Px.extend(vals)
        Pp.append(len(Pj))
    return np.array(Pp, dtype=np.intc), np.array(Pj, dtype=np.intc), np.array(Px, dtype=np.float64)


def same_arrays(got, want):
    """(Pp, Pj, Px) against (Pp, Pj, Px) on the raw bytes: NaN payloads and the sign of zero count"""
    return all(cio.same_bits(np.asarray(g), w) for g, w in zip(got, want))


def arrays_of(P):
    return P.indptr.astype(np.intc), P.indices.astype(np.intc), P.data.astype(np.float64)


# ------------------------------------------------------------------------------------------------ operators
def _csr(n, entries):
    """{row: [(column, value), ...]} in the stored order given -> CSR with int32 arrays, nothing sorted or summed"""
    p, j, x = [0], [], []
    for i in range(n):
        for c, v in entries.get(i, []):
            j.append(c); x.append(v)
        p.append(len(j))
    M = sps.csr_matrix((np.array(x, dtype=np.float64), np.array(j, dtype=np.intc), np.array(p, dtype=np.intc)), shape=(n, n))
    return M


def poisson3d(m):
    I, T = sps.identity(m), sps.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    A = (sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T)).tocsr()
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.intc), A.indptr.astype(np.intc)
    return A


def aniso():
    return sps.csr_matrix(cio.operator("aniso_40x40"), copy=True)


def shuffled(M, seed):
    """the same matrix with the entries of every row in a random stored order"""
    rng = np.random.RandomState(seed)
    j, x = M.indices.copy(), M.data.copy()
    for i in range(M.shape[0]):
        lo, hi = M.indptr[i], M.indptr[i + 1]
        perm = lo + rng.permutation(hi - lo)
        j[lo:hi], x[lo:hi] = M.indices[perm], M.data[perm]
    return sps.csr_matrix((x, j, M.indptr.copy()), shape=M.shape)


def strength(A, theta=0.25):
    from pyamg_amd import classical
    return classical.classical_strength_of_connection(A, theta, device=False)


def _crafted(name):
    c = cio.crafted(name)[0]
    n = len(c["Ap"]) - 1
    return sps.csr_matrix((c["Ax"].copy(), c["Aj"].copy(), c["Ap"].copy()), shape=(n, n))


# ------------------------------------------------------------------------------------------------ cycling on the host
def right_hand_side(n):
    return np.random.RandomState(7).rand(n)


def host_cycles(ml, b, tol=1e-8, maxiter=200):
    """V(1,1) cycles with symmetric Gauss-Seidel and a pseudo-inverse on the coarsest level, from x = 0, on the host:
    the number of cycles until ||b - A x|| <= tol ||b|| (the solver's own cycling needs a GPU)"""
    from pyamg_amd._host import dp, host_lib, i32, ip
    L = host_lib()
    ops = []
    for lvl in ml.levels:
        A = lvl.A
        ops.append((A, i32(A.indptr), i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)))
    coarse = np.linalg.pinv(ml.levels[-1].A.toarray())

    def smooth(k, x, rhs):
        A, Ap, Aj, Ax = ops[k]
        n = A.shape[0]
        L.amgsetup_gauss_seidel(ip(Ap), ip(Aj), dp(Ax), dp(x), dp(rhs), 0, n, 1)
        L.amgsetup_gauss_seidel(ip(Ap), ip(Aj), dp(Ax), dp(x), dp(rhs), n - 1, -1, -1)

    def cycle(k, x, rhs):
        if k == len(ops) - 1:
            x[:] = coarse.dot(rhs)
            return
        smooth(k, x, rhs)
        rc = np.ascontiguousarray(ml.levels[k].R.dot(rhs - ops[k][0].dot(x)))
        xc = np.zeros_like(rc)
        cycle(k + 1, xc, rc)
        x += ml.levels[k].P.dot(xc)
        smooth(k, x, rhs)

    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    A = ops[0][0]
    stop = tol * np.linalg.norm(b)
    for it in range(1, maxiter + 1):
        cycle(0, x, b)
        if np.linalg.norm(b - A.dot(x)) <= stop:
            return it
    return maxiter + 1


# ------------------------------------------------------------------------------------------------ designed cases
def _chain():
    """0 (C) - 1 (F) - 2 (F) - 3 (C), everything strong: row 2 has the strong C neighbour 3 and, through 1, the
    distance-two C point 0; row 1 likewise.  Row 4 (F) depends on the F point 5 alone, which depends on C point 0:
    no strong C neighbour, but a distance-two one.  Row 6 (F) is strongly connected to the F point 7 alone, which has
    no C neighbour: an empty C_hat."""
    A = _csr(8, {0: [(0, 4.0), (1, -1.0), (5, -1.5)],
                 1: [(0, -1.0), (1, 4.0), (2, -1.25)],
                 2: [(1, -1.25), (2, 4.0), (3, -0.75)],
                 3: [(2, -0.75), (3, 4.0)],
                 4: [(4, 3.0), (5, -2.0), (3, -0.001)],
                 5: [(5, 3.5), (4, -2.0), (0, -1.5)],
                 6: [(6, 2.0), (7, -1.0)],
                 7: [(7, 2.0), (6, -1.0)]})
    S = _csr(8, {0: [(1, 1.0), (5, 1.0)], 1: [(0, 1.0), (2, 1.0)], 2: [(1, 1.0), (3, 1.0)], 3: [(2, 1.0)],
                 4: [(5, 1.0)], 5: [(4, 1.0), (0, 1.0)], 6: [(7, 1.0)], 7: [(6, 1.0)]})
    spl = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=np.intc)

    def check(trace):
        assert trace[4]["Cs"] == [] and trace[4]["chat"] == [0]             # distance two only
        assert trace[6]["chat"] == [] and trace[7]["chat"] == []            # empty rows
        assert trace[2]["chat"] == [0, 3] and 0 not in {c for c, _ in _rows(A)[2]}      # a member that is no neighbour
    return A, S, spl, check


def _lumped():
    """row 1 (F) depends strongly on the F point 2, whose row holds neither 1's C_hat nor a negative entry at 1: d_2 == 0,
    so a_12 joins D"""
    A = _csr(4, {0: [(0, 2.0), (1, -1.0)],
                 1: [(1, 3.0), (0, -1.0), (2, -1.0)],
                 2: [(2, 2.0), (1, 0.5), (3, -1.0)],
                 3: [(3, 2.0), (2, -1.0)]})
    S = _csr(4, {0: [(1, 1.0)], 1: [(0, 1.0), (2, 1.0)], 2: [(1, 1.0)], 3: [(2, 1.0)]})
    spl = np.array([1, 0, 0, 0], dtype=np.intc)

    def check(trace):
        assert trace[1]["lumped"] == [2] and trace[1]["chat"] == [0]
    return A, S, spl, check


def _signs():
    """positive off-diagonals that the filter drops, and row 3 with a negative diagonal, where the filter keeps the
    positive entries instead"""
    A = _csr(5, {0: [(0, 4.0), (1, -1.0), (2, 0.5)],
                 1: [(1, 4.0), (0, -1.0), (2, 0.75), (3, -1.0)],
                 2: [(2, 4.0), (0, 0.5), (1, 0.75), (4, -2.0)],
                 3: [(3, -4.0), (1, 1.0), (4, 1.5), (0, -0.25)],
                 4: [(4, 4.0), (2, -2.0), (3, 1.5)]})
    S = _csr(5, {0: [(1, 1.0), (2, 1.0)], 1: [(0, 1.0), (2, 1.0), (3, 1.0)], 2: [(0, 1.0), (1, 1.0), (4, 1.0)],
                 3: [(1, 1.0), (4, 1.0), (0, 1.0)], 4: [(2, 1.0), (3, 1.0)]})
    spl = np.array([1, 0, 0, 0, 1], dtype=np.intc)

    def check(trace):
        assert trace[1]["filtered"] > 0 and trace[2]["filtered"] > 0
        assert A[3, 3] < 0 and 3 in trace[1]["Fs"] and 3 not in trace[1]["lumped"]
    return A, S, spl, check


def _weak_in_chat():
    """row 1 (F): its neighbour 3 (C) is weak (not in S_1) but belongs to C_hat through the strong F neighbour 2, so
    a_13 is interpolatory; its neighbour 4 (C) is weak and in nobody's strong set, so a_14 is lumped.  S stores its
    diagonal."""
    A = _csr(5, {0: [(0, 4.0), (1, -2.0)],
                 1: [(1, 5.0), (0, -2.0), (2, -2.0), (3, -0.125), (4, -0.0625)],
                 2: [(2, 4.0), (1, -2.0), (3, -1.5)],
                 3: [(3, 4.0), (2, -1.5), (1, -0.125)],
                 4: [(4, 1.0), (1, -0.0625)]})
    S = _csr(5, {0: [(0, 1.0), (1, 1.0)], 1: [(1, 1.0), (0, 1.0), (2, 1.0)], 2: [(2, 1.0), (1, 1.0), (3, 1.0)],
                 3: [(3, 1.0), (2, 1.0)], 4: [(4, 1.0), (1, 1.0)]})
    spl = np.array([1, 0, 0, 1, 1], dtype=np.intc)

    def check(trace):
        assert trace[1]["Cs"] == [0] and trace[1]["chat"] == [0, 3] and A[1, 3] != 0 and A[1, 4] != 0
        assert all((i, i) in {(r, c) for r in range(5) for c, _ in _rows(S)[r]} for i in range(5))
    return A, S, spl, check


def _zero_D():
    """F rows whose D is zero: row 1 (a stored zero diagonal, nothing lumped) has the weights +inf, +inf and, at the
    stored zero a_13, NaN; row 4 stores no diagonal at all.  Rows with a non-finite weight are never truncated."""
    A = _csr(6, {0: [(0, 2.0), (1, -1.0)],
                 1: [(0, -1.0), (1, 0.0), (2, -1.0), (3, 0.0)],
                 2: [(2, 2.0), (1, -1.0)],
                 3: [(3, 2.0), (1, 0.0)],
                 4: [(5, -1.0), (0, -0.5)],
                 5: [(5, 1.0), (4, -1.0)]})
    S = _csr(6, {0: [(1, 1.0)], 1: [(0, 1.0), (2, 1.0), (3, 1.0)], 2: [(1, 1.0)], 3: [(1, 1.0)], 4: [(0, 1.0), (5, 1.0)],
                 5: [(4, 1.0)]})
    spl = np.array([1, 0, 1, 1, 0, 1], dtype=np.intc)

    def check(trace):
        Pp, Pj, Px = model(A, S, spl)
        row = Px[Pp[1]:Pp[2]]
        assert len(row) == 3 and np.isinf(row[0]) and np.isinf(row[1]) and np.isnan(row[2])
        assert model(A, S, spl, max_per_row=1)[0][2] - model(A, S, spl, max_per_row=1)[0][1] == 3
    return A, S, spl, check


def _truncation():
    """rows made for the truncation rule: row 0 (F) has four weights of equal magnitude (a tie: the smaller columns
    stay); row 5 (F) has weights +x, -x, so that the two kept entries sum to zero (s_kept == 0: no rescaling) beside
    a smaller third one; row 6 (F) has two entries (m <= q for q = 2, 4)"""
    A = _csr(7, {0: [(0, 4.0), (1, -1.0), (2, -1.0), (3, -1.0), (4, -1.0)],
                 1: [(1, 1.0)], 2: [(2, 1.0)], 3: [(3, 1.0)], 4: [(4, 1.0)],
                 5: [(5, 2.0), (1, -1.0), (2, 1.0), (3, -0.25)],
                 6: [(6, 2.0), (3, -1.0), (4, -0.5)]})
    S = _csr(7, {0: [(1, 1.0), (2, 1.0), (3, 1.0), (4, 1.0)], 5: [(1, 1.0), (2, 1.0), (3, 1.0)], 6: [(3, 1.0), (4, 1.0)]})
    spl = np.array([0, 1, 1, 1, 1, 0, 0], dtype=np.intc)

    def check(trace):
        Pp, Pj, Px = model(A, S, spl)
        assert len(set(np.abs(Px[Pp[0]:Pp[1]]))) == 1 and Pp[1] == 4
        Tp, Tj, Tx = model(A, S, spl, max_per_row=2)
        assert list(Tj[Tp[0]:Tp[1]]) == [0, 1]                              # the tie keeps the smaller columns
        info = {}
        model(A, S, spl, max_per_row=2, trace=info)
        assert info[5]["truncated"] and info[5]["s_kept"] == 0.0 and not info[6]["truncated"]
        assert cio.same_bits(Tx[Tp[5]:Tp[6]], Px[Pp[5]:Pp[6]][:2])         # kept as they were
    return A, S, spl, check


def _pmis_problem(A, seed, theta=0.25):
    from pyamg_amd import classical
    S = strength(A, theta)
    np.random.seed(seed)
    return A, S, classical.PMIS(S, device=False)


def _grid(shuffle):
    """Poisson 17 x 23 (391 rows, more than a workgroup) under its PMIS splitting; shuffle: every row of A and S in a
    random stored order"""
    A, S, spl = _pmis_problem(sio.poisson2d(17, 23), 3)
    if shuffle:
        A, S = shuffled(A, 11), shuffled(S, 12)

    def check(trace):
        assert A.shape[0] > 256 and any(len(t["chat"]) > len(t["Cs"]) for t in trace.values())     # distance two is used
        if shuffle:
            from pyamg_amd import classical
            assert not classical._sorted_unique_rows(A) and not classical._sorted_unique_rows(S)
    return A, S, spl, check


def _recorded(name):
    """-> A and [(S, splitting)] of the recorded interpolation calls of a crafted fixture (S: the pattern with ones)"""
    A = _crafted(name)
    n = A.shape[0]
    out = []
    for entry, ins, _ in cio.crafted(name)[1]:
        if entry == "rs_direct_interpolation_pass1":
            Sp, Sj = ins["Sp"].astype(np.intc), ins["Sj"][:ins["Sp"][n]].astype(np.intc)
            out.append((sps.csr_matrix((np.ones(len(Sj)), Sj, Sp), shape=(n, n)), ins["splitting"].astype(np.intc)))
    return A, out


def slots(S, splitting, i):
    """the candidate slots of F row i: row i of S and the rows of S of its strong F neighbours;
    more than 256 leave the LDS path of the device kernels"""
    row = S.indices[S.indptr[i]:S.indptr[i + 1]]
    return len(row) + sum(S.indptr[k + 1] - S.indptr[k] for k in row if k != i and splitting[k] == 0)


def _branches(which):
    """branches.npz under its three recorded splittings: mixed (its F row 3 has a zero diagonal: non-finite weights;
    its row 0 is empty), all C and all F"""
    A, calls = _recorded("branches")
    S, spl = calls[which]

    def check(trace):
        if which == 0:
            assert spl[3] == 0 and A[3, 3] == 0 and trace[3]["chat"] and A.indptr[1] == 0
        else:
            assert np.all(spl == (1 if which == 1 else 0))
            assert model(A, S, spl)[0][-1] == (A.shape[0] if which == 1 else 0)
    return A, S, spl.copy(), check


def _wide(full):
    """wide_257c (257 rows, one past a workgroup).  full: S is A's pattern and row 128 the only F point, so that its
    C_hat holds all 256 other points, the most 257 rows allow, on 257 slots.  Otherwise the recorded S (202 entries in
    row 128) with row 128 and twenty of its strong neighbours as F points: row 128 has more than 256 slots, and F rows
    beside it reach through it more than 64 members on fewer than 256 slots."""
    A, calls = _recorded("wide_257c")
    n = A.shape[0]
    spl = np.ones(n, dtype=np.intc)
    spl[128] = 0
    if full:
        S = sps.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    else:
        S = calls[0][0]
        row = [k for k in S.indices[S.indptr[128]:S.indptr[129]] if k != 128]
        for k in row[:18] + [127, 129]:
            spl[k] = 0

    def check(trace):
        assert n == 257 and slots(S, spl, 128) > 256
        if full:
            assert len(trace[128]["chat"]) == 256
        else:
            assert len(trace[128]["chat"]) > 64
            assert any(64 < len(t["chat"]) <= 256 and slots(S, spl, i) <= 256 for i, t in trace.items() if i != 128)
    return A, S, spl, check


CASES = {"chain": _chain, "lumped": _lumped, "signs": _signs, "weak_in_chat": _weak_in_chat, "zero_D": _zero_D,
         "truncation": _truncation,
         "grid": lambda: _grid(False), "grid_shuffled": lambda: _grid(True), "zero_diagonal": lambda: _branches(0),
         "all_C": lambda: _branches(1), "all_F": lambda: _branches(2), "wide": lambda: _wide(False),
         "wide_full": lambda: _wide(True)}


def case(name):
    """-> (A, S, splitting, check, want) with want = {q: model arrays} for q in QS and trace = the model's trace;
    built once, read-only"""
    if name not in _cache:
        A, S, spl, check = CASES[name]()
        trace = {}
        want = {None: model(A, S, spl, trace=trace)}
        for q in QS[1:]:
            want[q] = model(A, S, spl, max_per_row=q)
        for arrays in want.values():
            for a in arrays:
                a.setflags(write=False)
        spl.setflags(write=False)
        _cache[name] = (A, S, spl, check, want, trace)
    return _cache[name]


QS = (None, 1, 2, 4)
