"""Operators with DESIGNED dependency levels for the point Gauss-Seidel kernel set (tests/test_gs_cases_host.py pins
them on the host, tests/test_gpu_gs_forms.py sweeps them on the device).  No GPU, no torch.

The layered generator numbers the rows level by level.  A row of level l holds one entry in level l - 1 (which pins its
level), further entries in chosen earlier levels l - d, entries in chosen LATER levels l + d (never the row's own level:
the write-after-read rule of build_levels would move the target) and its diagonal -- all in shuffled stored order.  A
row may instead be pinned by a READER: a row of level l - 1 that holds an entry pointing at it (write after read), which
is how rows without any earlier operand, and diagonal-only rows, are placed in a chosen level.  build_levels() below is
a restatement of csrc/hier.hip build_levels; selection() restates the choices of build_csr_schedule and
build_flow_form, field by field as amg_mat_gs_info reports them.

Values: off-diagonals are random non-dyadic numbers of magnitude 0.1 .. 1, the diagonal dominates its row (nine sweeps
stay finite), and -- unless a case says otherwise -- every fifth row stores its diagonal twice with different values
(the last one wins, relaxation.h:51-52)."""
import numpy as np

INFO_FIELDS = ("levels", "chains", "chained", "chain_long", "chain2", "c2_pf", "cl_codes", "flow", "lpr", "nchunks",
               "flow_auto", "level_copy")
SEQUENCES = ([0], [1], [0, 0], [1, 1], [0, 1], [1, 0], [0, 1, 0, 1], [1, 1, 0, 0, 1], [0, 1, 1, 0, 0, 1, 0, 1, 1])
FLOW_SENTINEL = 0x7FF4A5A55A5A0001
SENSITIVITY = ("reversed_sum", "stale_operand", "first_diagonal", "flavour")


class Case(object):
    def __init__(self, name, family, n, ncols, rows, widths=None, order=None, expect=None, exempt=(), longest=None,
                 short=None):
        self.name, self.family, self.n, self.ncols = name, family, n, ncols
        self.rows = rows                                  # per row: [(column, value)] in stored order
        self.widths = widths                              # designed level widths (None: an index list decides)
        self.order = None if order is None else np.ascontiguousarray(order, dtype=np.intc)
        self.expect = dict(expect or {})                  # amg_mat_gs_info fields stated by hand (built under flow 2)
        self.exempt = frozenset(exempt)                   # sensitivity checks that cannot change a bit here
        self.longest = longest                            # designed longest off-diagonal row (None: not stated)
        self.short = short                                # designed nnz <= 10 n (None: not stated)
        self.Ap = np.zeros(n + 1, dtype=np.intc)
        self.Ap[1:] = np.cumsum([len(r) for r in rows])
        self.Aj = np.array([c for r in rows for c, v in r], dtype=np.intc)
        self.Ax = np.array([v for r in rows for c, v in r], dtype=np.float64)
        self.nnz = int(self.Ap[-1])
        rng = np.random.RandomState(len(name) * 7919 + n)
        self.b = rng.uniform(-1.0, 1.0, n) * 3.1
        self.x = rng.uniform(-1.0, 1.0, ncols) * 1.7
        self.halo = ncols > n
        self._levels = None
        self._sel = {}

    def __repr__(self):
        return self.name

    def tasks(self):
        return list(range(self.n)) if self.order is None else [int(i) for i in self.order]

    def levels(self):
        """(level_ptr, order) of the restated build_levels, computed once"""
        if self._levels is None:
            self._levels = build_levels(self.n, self.rows, self.tasks())
        return self._levels

    def info(self, flow_mode=2):
        if flow_mode not in self._sel:
            self._sel[flow_mode] = selection(self, flow_mode)
        return self._sel[flow_mode]

    def longest_offdiag(self):
        return max([sum(1 for c, v in self.rows[i] if c != i) for i in set(self.tasks())] or [0])


# ---------------------------------------------------------------------------------------------- restated host rules
def build_levels(n, rows, tasks):
    """csrc/hier.hip build_levels: level of a task = 1 + the latest earlier task that wrote what it reads or writes, or
    read what it writes.  Returns (level_ptr, order): order[k] = index into tasks of the k-th task in level order."""
    lastW, lastR, lvl = [0] * n, [0] * n, []
    for i in tasks:
        l = max(lastW[i], lastR[i])
        for c, v in rows[i]:
            if c != i and 0 <= c < n and lastW[c] > l:
                l = lastW[c]
        l += 1
        lvl.append(l)
        lastW[i] = l
        for c, v in rows[i]:
            if c != i and 0 <= c < n and lastR[c] < l:
                lastR[c] = l
    nl = max(lvl) if lvl else 0
    level_ptr = [0] * (nl + 1)
    for l in lvl:
        level_ptr[l] += 1
    for l in range(nl):
        level_ptr[l + 1] += level_ptr[l]
    cur = list(level_ptr[:-1])
    order = [0] * len(tasks)
    for t, l in enumerate(lvl):
        order[cur[l - 1]] = t
        cur[l - 1] += 1
    return level_ptr, order


def _pieces(classes, first, last, minlen, closer_from_above):
    """runs of one class in [first, last); a run shorter than minlen joins a neighbour (build_csr_schedule)"""
    pc = []
    for q in range(first, last):
        c = classes[q]
        if pc and pc[-1][2] == c:
            pc[-1][1] = q + 1
        else:
            pc.append([q, q + 1, c])
    merged = True
    while merged and len(pc) > 1:
        merged = False
        for k in range(len(pc)):
            if pc[k][1] - pc[k][0] >= minlen:
                continue
            if k == 0:
                j = 1
            elif k + 1 == len(pc):
                j = k - 1
            elif closer_from_above:
                j = k - 1 if (pc[k - 1][2] >= pc[k][2] and (pc[k + 1][2] < pc[k][2] or pc[k - 1][2] <= pc[k + 1][2])) else k + 1
            else:
                j = k - 1 if pc[k - 1][2] <= pc[k + 1][2] else k + 1
            a0, a1 = min(j, k), max(j, k)
            pc[a0] = [pc[a0][0], pc[a1][1], max(pc[a0][2], pc[a1][2])]
            del pc[a1]
            merged = True
            break
        k = 0
        while k + 1 < len(pc):
            if pc[k][2] == pc[k + 1][2]:
                pc[k][1] = pc[k + 1][1]
                del pc[k + 1]
                merged = True
            else:
                k += 1
    return pc


def selection(case, flow_mode=2):
    """What build_csr_schedule (csrc/hier.hip) and build_flow_form (csrc/gsflow.hip) decide for this case when the
    schedule is built under amg_set_gs_flow(flow_mode), as the twelve fields of amg_mat_gs_info."""
    n, rows, tasks = case.n, case.rows, case.tasks()
    level_ptr, order = case.levels()
    ntasks, nl = len(tasks), len(level_ptr) - 1
    rowmap = [tasks[t] for t in order]
    width = [level_ptr[l + 1] - level_ptr[l] for l in range(nl)]
    def stored(i):                                          # entries of the level-ordered copy: overridden diagonals are left out
        return len(rows[i]) - max(0, sum(1 for c, v in rows[i] if c == i) - 1)
    entries = [sum(stored(rowmap[k]) for k in range(level_ptr[l], level_ptr[l + 1])) for l in range(nl)]
    nnz = sum(entries)
    short_rows = ntasks > 0 and nnz <= 10.0 * ntasks
    once = ntasks == n and len(set(rowmap)) == n
    inside = all(0 <= c < n for i in set(rowmap) for c, v in rows[i])

    def diag(i):
        d = [v for c, v in rows[i] if c == i]
        return d[-1] if d else 0.0

    def offdiag(i):
        return sum(1 for c, v in rows[i] if c != i)

    def cls(w):
        return 64 if w <= 64 else (128 if w <= 128 else (256 if w <= 256 else 512))

    chains, chain_long = [], False
    if short_rows:
        l = 0
        while l < nl:
            if width[l] > 512:
                l += 1
                continue
            e = l
            while e < nl and width[e] <= 512:
                e += 1
            if e - l >= 4:
                for q in _pieces([cls(w) for w in width], l, e, 16, True):
                    for p in range(q[0], q[1], 4096):
                        chains.append((p, min(q[1], p + 4096), q[2]))
            l = e
    elif ntasks > 0:
        def need(q):
            if entries[q] < 4:
                return 513
            w = max(width[q], (entries[q] + 7) // 8)
            return cls(w) if w <= 512 else 513
        nd = [need(q) for q in range(nl)]
        l = 0
        while l < nl:
            if nd[l] > 512:
                l += 1
                continue
            e = l
            while e < nl and nd[e] <= 512:
                e += 1
            if e - l >= 4:
                for q in _pieces(nd, l, e, 8, False):
                    for p in range(q[0], q[1], 1024):
                        chains.append((p, min(q[1], p + 1024), q[2]))
                chain_long = True
            l = e
    in_chain = [False] * nl
    for c in chains:
        for l in range(c[0], c[1]):
            in_chain[l] = True
    chained_rows = [rowmap[k] for l in range(nl) if in_chain[l] for k in range(level_ptr[l], level_ptr[l + 1])]
    cl_codes = chain_long and once and all(diag(i) != 0.0 and all(0 <= c < n for c, v in rows[i]) for i in chained_rows)
    chain2, c2_pf = False, 0
    if chains and not chain_long and once and inside:
        longest = max(offdiag(i) for i in chained_rows)
        c2_pf = 4 if longest <= 4 else (8 if longest <= 8 else 12)
        chain2 = longest <= 12 and all(diag(i) != 0.0 for i in chained_rows)
    flow, lpr, nchunks, flow_auto = False, 1, 0, False
    allow_flow = True                                    # halo cases run with AMG_DIST_FLOW=1
    chained = sum(c[1] - c[0] for c in chains)
    if allow_flow and flow_mode != 0 and ntasks == n:
        wanted = (chain_long or chained * 10 < nl * 9) and ntasks < nl * 200000
        if wanted or flow_mode == 2:
            ok = n > 0 and nl > 0 and once and all(0 <= c < case.ncols for i in range(n) for c, v in rows[i])
            ok = ok and all(any(c == i for c, v in rows[i]) and diag(i) != 0.0 for i in range(n))
            longest = max(offdiag(i) for i in range(n)) if ok else 0
            if ok and longest <= 512:
                while lpr * 8 < longest:
                    lpr *= 2
                R = 64 // lpr
                nchunks = sum((w + R - 1) // R for w in width)
                flow = True
            flow_auto = wanted and flow
    dropped = flow_auto and flow_mode == 1
    out = dict(levels=nl, chains=len(chains), chained=chained, chain_long=int(chain_long), chain2=int(chain2), c2_pf=c2_pf,
               cl_codes=int(cl_codes), flow=int(flow), lpr=lpr, nchunks=nchunks, flow_auto=int(flow_auto), level_copy=1)
    if dropped:
        out.update(chains=0, chained=0, chain_long=0, chain2=0, cl_codes=0, level_copy=0)
    out["chain_widths"] = [] if dropped else [c[2] for c in chains]       # not an info field: the launches' workgroup sizes
    return out


# ---------------------------------------------------------------------------------------------- the layered generator
def _value(rng):
    v = rng.uniform(0.1, 1.0) * (1.0 if rng.rand() < 0.5 else -1.0)
    return float(v) * 1.0000001192092896               # never a short dyadic fraction


def layered(name, family, widths, spec, seed, double_diag=5, ncols_extra=0, sort=None, **kw):
    """spec(l, p) -> dict with optional keys
         lower: level distances d (an entry into level l - d each; 1 is added unless pin == 'reader')
         upper: level distances d (an entry into level l + d each, where that level exists)
         fill:  that many more entries into earlier rows (all distinct while enough earlier rows exist)
         pin:   'reader' -- no entry of its own fixes the level; a row of level l - 1 gets an entry pointing here
         dup:   store the first off-diagonal column a second time (another value)
         zero:  one more entry, an explicit 0.0, at a column of level l - 1
         halo:  that many entries into the halo columns n .. n + ncols_extra - 1
         diag:  'twice' | 'once' | 'zero' | 'missing' (default: twice on every double_diag-th row)"""
    rng = np.random.RandomState(seed)
    start = np.concatenate(([0], np.cumsum(widths))).astype(int)
    n, nl = int(start[-1]), len(widths)
    cols = [[] for _ in range(n)]
    specs, zero_at = {}, {}
    for l in range(nl):
        for p in range(widths[l]):
            i = int(start[l]) + p
            s = dict(spec(l, p) or {})
            specs[i] = s
            lower = list(s.get("lower", ()))
            if l >= 1 and s.get("pin") != "reader" and 1 not in lower:
                lower.insert(0, 1)
            for d in lower:
                if 1 <= d <= l:
                    cols[i].append(int(start[l - d]) + (p * 3 + d) % widths[l - d])
            for d in s.get("upper", ()):
                if l + d < nl:
                    cols[i].append(int(start[l + d]) + (p * 5 + d) % widths[l + d])
            k = int(s.get("fill", 0))
            if k and start[l] > 0:
                off = int(rng.randint(0, start[l]))
                have = set(cols[i])
                q = 0
                while k > 0:
                    c = (off + q) % int(start[l])
                    q += 1
                    if c in have and q <= start[l]:
                        continue
                    cols[i].append(c)
                    have.add(c)
                    k -= 1
            if s.get("zero") and l >= 1:                    # at a column of the level before: a dependency like any entry
                zero_at[i] = int(start[l - 1]) + (p * 7 + 2) % widths[l - 1]
            for h in range(int(s.get("halo", 0))):
                cols[i].append(n + (i * 3 + h * 7) % ncols_extra)
    for l in range(1, nl):                                  # readers, after every row's own entries
        for p in range(widths[l]):
            i = int(start[l]) + p
            if specs[i].get("pin") == "reader":
                cols[int(start[l - 1]) + p % widths[l - 1]].append(i)
    rows = []
    for i in range(n):
        s = specs[i]
        ent = [(c, _value(rng)) for c in cols[i]]
        if s.get("dup") and ent:
            ent.append((ent[0][0], _value(rng)))
        if i in zero_at:
            ent.append((zero_at[i], 0.0))
        mag = sum(abs(v) for c, v in ent) + 1.0
        d = s.get("diag", "twice" if (double_diag and i % double_diag == 2) else "once")
        dv = float(mag * rng.uniform(1.5, 2.5)) * 1.0000001192092896
        if d == "twice":
            ent.append((i, dv * 0.37))
            order = rng.permutation(len(ent))
            ent = [ent[k] for k in order]
            ent.insert(int(rng.randint(ent.index((i, dv * 0.37)) + 1, len(ent) + 1)), (i, dv))    # the dominating one last
        else:
            if d == "once":
                ent.append((i, dv))
            elif d == "zero":
                ent.append((i, 0.0))
            ent = [ent[k] for k in rng.permutation(len(ent))]
        if sort == "descending":
            ent.sort(key=lambda cv: -cv[0])
        rows.append(ent)
    return Case(name, family, n, n + ncols_extra, rows, widths=list(widths), **kw)


def generic(l, p):
    """operands one, two and three levels back and ahead on some rows; at most 6 off-diagonal entries"""
    k = p % 4
    if k == 0:
        return dict(lower=[1, 2, 3], upper=[1, 2, 3])
    if k == 1:
        return dict(lower=[1, 2], upper=[1])
    if k == 2:
        return dict(lower=[1], upper=[2, 3])
    return dict(lower=[1, 3])


# ---------------------------------------------------------------------------------------------- the families
def flow_lpr_cases():
    out = []
    for L, lpr in ((0, 1), (1, 1), (8, 1), (9, 2), (16, 2), (17, 4), (32, 4), (33, 8), (64, 8), (65, 16), (128, 16),
                   (129, 32), (256, 32), (257, 64), (512, 64), (513, 0)):
        if L == 0:
            c = layered("flow_lpr_0", "flow_lpr", [640], lambda l, p: {}, 100, longest=0, short=True,
                        exempt=("reversed_sum", "stale_operand", "flavour"), expect=dict(levels=1, flow=1, lpr=1, nchunks=10, chains=0))
            out.append(c)
            continue
        R = 64 // lpr if lpr else 1
        widths = [560] + [w for w in (R - 1, R, R + 1) if w >= 1] + [5, 3]
        nl = len(widths)

        def spec(l, p, L=L, nl=nl):
            if p == 0 and l >= 1:
                return dict(pin="reader")                   # a chain of rows with one later entry each; the last one is diagonal-only
            if p == 1 and l in (2, nl - 2):
                return dict(fill=L - 1)                     # the long rows: one where the level width sits on the chunk size, one near the end
            if L == 1 or l == 0:
                return {}
            return dict(lower=[1, 2] if p % 2 else [1], upper=[1] if (p % 3 == 0 and L >= 3) else [])
        R1 = 64 // lpr if lpr else 64
        nch = sum((w + R1 - 1) // R1 for w in widths)
        exp = dict(levels=nl, flow=int(lpr != 0), lpr=max(lpr, 1), nchunks=nch if lpr else 0, chain_long=0)
        out.append(layered("flow_lpr_%d" % L, "flow_lpr", widths, spec, 100 + L, longest=L, short=True, expect=exp,
                           exempt=("reversed_sum", "flavour") if L == 1 else ()))     # one product per row: no order, one rounding
    return out


def _grid_widths(nchunks):
    pat, w, k = (65, 20, 64, 7, 130), [], 0
    left = nchunks
    while left > 0:
        c = pat[k % len(pat)]
        if (c + 63) // 64 > left:
            c = 33
        w.append(c)
        left -= (c + 63) // 64
        k += 1
    return w


def flow_grid_cases():
    out = []
    for n in (1, 64, 65, 130):
        out.append(layered("flow_grid_diag_%d" % n, "flow_grid", [n], lambda l, p: {}, 200 + n, double_diag=3, longest=0, short=True,
                           exempt=("reversed_sum", "stale_operand", "flavour") + (("first_diagonal",) if n == 1 else ()),
                           expect=dict(levels=1, flow=1, lpr=1, nchunks=(n + 63) // 64, chains=0)))
    # one level, one chunk, rows that are not diagonal-only: every operand is a frozen halo column
    out.append(layered("flow_grid_1", "flow_grid", [40], lambda l, p: dict(halo=3), 260, ncols_extra=8, longest=3, short=True,
                       exempt=("stale_operand",), expect=dict(levels=1, flow=1, lpr=1, nchunks=1, chains=0, chain2=0)))
    for k in (15, 16, 17, 23, 31, 32, 33):
        w = _grid_widths(k)
        out.append(layered("flow_grid_%d" % k, "flow_grid", w, generic, 270 + k, longest=6, short=True,
                           expect=dict(levels=len(w), flow=1, lpr=1, nchunks=k)))
    return out


def flow_gate_cases():
    def spec(l, p):
        k = p % 6
        if k == 0:
            return dict(lower=[1])                          # operands exactly one level back
        if k == 1:
            return dict(pin="reader", lower=[2])           # exactly two back: that operand is the gate
        if k == 2:
            return dict(pin="reader", lower=[5, 7, 9])     # many levels back
        if k == 3:
            return dict(pin="reader", upper=[1, 2])        # later levels only: the gate is the permanent zero
        if k == 4:
            return dict(lower=[1, 2, 3], upper=[1, 2, 3])
        return dict(lower=[1], upper=[3])
    return [layered("flow_gate_narrow", "flow_gate", [30] * 12, spec, 300, short=True,
                    expect=dict(levels=12, flow=1, lpr=1, nchunks=12, chains=1, chained=12, chain2=1, c2_pf=8)),
            layered("flow_gate_wide", "flow_gate", [100, 70, 130] * 4, spec, 301, short=True,
                    expect=dict(levels=12, flow=1, lpr=1, nchunks=28, chains=1, chained=12, chain2=1, c2_pf=8))]


def chain_short_cases():
    out = []

    def add(name, widths, spec=generic, **exp):
        longest = exp.pop("longest", None)
        out.append(layered("chain_short_" + name, "chain_short", widths, spec, 400 + len(out), longest=longest, short=True,
                           expect=dict(exp, levels=len(widths), chain_long=0)))
    add("run3", [600, 10, 10, 10, 600], chains=0, chained=0, chain2=0)
    add("run4", [600, 10, 10, 10, 10, 600], chains=1, chained=4, chain2=1, c2_pf=8)
    def three(l, p):                                        # at most three off-diagonal entries: 4 slots per row
        return dict(lower=[1, 2], upper=[1] if p % 2 else [])

    def nine(l, p):                                         # one row of nine in every chain: 12 slots per row
        return dict(fill=8) if (p == 5 and l % 8 == 4) else generic(l, p)
    add("w64_65", [64] * 16 + [65] * 16, nine, chains=2, chained=32, chain2=1, c2_pf=12)
    add("join15", [64] * 15 + [65] * 16, chains=1, chained=31, chain2=1)
    add("w128_129", [128] * 16 + [129] * 16, three, chains=2, chained=32, chain2=1, c2_pf=4)
    add("w256_513_257", [256] * 5 + [513] + [257] * 5, nine, chains=2, chained=10, chain2=1, c2_pf=12)
    add("w512_513_40", [512] * 4 + [513] + [40] * 4, chains=2, chained=8, chain2=1, c2_pf=8)
    add("w512_three", [512] * 4, three, chains=1, chained=4, chain2=1, c2_pf=4)
    for L, pf in ((4, 4), (5, 8), (8, 8), (9, 12), (12, 12), (13, 12), (40, 12)):
        def spec(l, p, L=L):
            if l == 4 and p == 7:
                return dict(fill=L - 1)
            return dict(lower=[1, 2], upper=[1] if p % 2 else [])
        add("longest_%d" % L, [50] * 6, spec, longest=L, chains=1, chained=6, chain2=int(L <= 12), c2_pf=pf)
    add("tridiagonal_4200", [1] * 4200, lambda l, p: dict(lower=[1], upper=[1]), longest=2, chains=2, chained=4200, chain2=1, c2_pf=4)
    return out


def _long_levels(pieces, first=520):
    """pieces: (levels, rows per level, off-diagonal entries per row); a first level of `first` short rows supplies the
    distinct earlier columns the long rows need"""
    widths, per = [first], [0]
    for nlev, r, e in pieces:
        widths += [r] * nlev
        per += [e] * nlev
    return widths, per


def chain_long_cases():
    out = []

    def add(name, pieces, first=520, **exp):
        widths, per = _long_levels(pieces, first)

        def spec(l, p):
            if l == 0:
                return dict(upper=[1, 2])
            return dict(fill=per[l] - 1)
        out.append(layered("chain_long_" + name, "chain_long", widths, spec, 500 + len(out), short=False,
                           longest=max(per), expect=dict(exp, levels=len(widths), chain_long=1, chain2=0, cl_codes=1)))
    # threads by ROWS: 60 / 100 / 200 / 300 rows of 7 stored entries; levels of 30 or 40 rows x 501 entries keep nnz above
    # 10 n (they need 1879 and more threads: level launches, like the 520-row first level)
    add("by_rows_64_128", [(8, 60, 6), (8, 100, 6), (2, 30, 500), (4, 60, 6)], chains=3, chained=20)
    add("by_rows_256_512", [(8, 200, 6), (8, 300, 6), (1, 40, 500)], chains=2, chained=16)
    # threads by ENTRIES, (entries + 7) / 8: 4 x 101 -> 51, 8 x 111 -> 111, 8 x 231 -> 231, 7 x 501 -> 439; then 10 x 501 -> 627 (a
    # level launch), a run of five levels, a one-row level of 2 entries (never chained: the e < 4 rule), and four more
    add("by_entries", [(8, 4, 100), (8, 8, 110), (8, 8, 230), (8, 7, 500), (1, 10, 500), (5, 4, 100), (1, 1, 1), (4, 4, 100)],
        chains=6, chained=41)
    add("pieces_7_8", [(7, 4, 40), (8, 8, 120)], chains=1, chained=15)
    add("pieces_8_8", [(8, 4, 40), (8, 8, 120)], chains=2, chained=16)
    w = [1] * 1100
    out.append(layered("chain_long_band_1100", "chain_long", w, lambda l, p: dict(lower=list(range(1, 13)), upper=list(range(1, 13))),
                       560, short=False, longest=24, expect=dict(levels=1100, chains=2, chained=1100, chain_long=1, cl_codes=1, chain2=0)))
    return out


def level_launch_cases():
    def tiles(l, p):
        if l == 2 and p in (3, 200, 599):
            return dict(fill=4500)                          # 4500 entries: three LDS tiles of 2048 in one workgroup
        return generic(l, p)
    return [layered("level_launch_short", "level_launch", [1500, 1400, 1300], generic, 600, short=True,
                    expect=dict(levels=3, chains=0, flow=1, lpr=1)),
            layered("level_launch_tiles", "level_launch", [2300, 2000, 600], tiles, 601, longest=4501, short=True,
                    expect=dict(levels=3, chains=0, flow=0))]


SHORT_BASE = [50] * 6 + [600] + [50] * 5
LONG_BASE = [(8, 6, 80), (1, 530, 3), (8, 10, 90)]


def _short(name, spec, **kw):
    exp = kw.pop("expect", {})
    return layered("odd_short_" + name, "oddities", SHORT_BASE, spec, 700 + len(name), short=True,
                   expect=dict(dict(levels=12, chains=2, chained=11, chain_long=0), **exp), **kw)


def _long(name, mod, **kw):
    widths, per = _long_levels(LONG_BASE)
    exp = kw.pop("expect", {})

    def spec(l, p):
        s = dict(upper=[1, 2]) if l == 0 else dict(fill=per[l] - 1)
        s.update(mod(l, p) or {})
        return s
    return layered("odd_long_" + name, "oddities", widths, spec, 800 + len(name), short=False,
                   expect=dict(dict(levels=len(widths), chains=2, chained=16, chain_long=1), **exp), **kw)


def oddity_cases():
    out = []

    def both(name, mod, short_exp, long_exp, **kw):
        out.append(_short(name, lambda l, p: dict(generic(l, p), **(mod(l, p) or {})), expect=short_exp, **kw))
        out.append(_long(name, mod, expect=long_exp, **kw))
    std_s, std_l = dict(chain2=1, flow=1), dict(cl_codes=1, flow=1)
    both("diag_twice", lambda l, p: dict(diag="twice"), std_s, std_l)
    both("duplicates", lambda l, p: dict(dup=True), std_s, std_l)
    both("zeros", lambda l, p: dict(zero=True), std_s, std_l)
    both("descending", lambda l, p: {}, std_s, std_l, sort="descending")
    # a zero / a missing diagonal in chained levels and in the wide one: the row keeps its value; the LDS hand-off copies and
    # the dataflow form decline
    both("zero_diag", lambda l, p: dict(diag="zero") if p == 2 and l in (3, 6, 9) else {}, dict(chain2=0, flow=0), dict(cl_codes=0, flow=0))
    both("missing_diag", lambda l, p: dict(diag="missing") if p == 2 and l in (3, 6, 9) else {}, dict(chain2=0, flow=0), dict(cl_codes=0, flow=0))
    both("halo", lambda l, p: dict(halo=2) if p % 3 == 0 else {}, dict(chain2=0, flow=1), dict(cl_codes=0, flow=1), ncols_extra=37)
    # index lists over the plain operators: a random permutation of all rows, a subset, a list with repeats
    for base, tag in ((_short, "short"), (_long, "long")):
        c0 = base("plain", (lambda l, p: generic(l, p)) if base is _short else (lambda l, p: {}))
        rng = np.random.RandomState(900 + len(tag))
        n = c0.n
        lists = (("permutation", rng.permutation(n)), ("subset", rng.permutation(n)[:n // 2]),
                 ("repeats", np.concatenate((rng.permutation(n), rng.randint(0, n, n // 3)))))
        for lname, order in lists:
            c = Case("odd_%s_%s" % (tag, lname), "oddities", n, c0.ncols, c0.rows, widths=None, order=order,
                     expect=dict(flow=int(lname == "permutation"), chain2=0) if lname != "permutation" else dict(flow=1))
            out.append(c)
    return out


def sentinel_case():
    """x carries the dataflow sentinel's bits at one owned and one halo position, each read by earlier rows"""
    def spec(l, p):
        s = generic(l, p)
        if p % 3 == 0:
            s["halo"] = 2
        return s
    c = layered("sentinel", "sentinel", [40] * 8, spec, 950, ncols_extra=11, short=True)
    owned = sum(c.widths[:5]) + 3                          # a row of level 5: rows of levels 2 .. 4 hold entries ahead into it
    halo = c.n + 4
    assert any(cc == owned for i in range(owned) for cc, v in c.rows[i]) and any(cc == halo for r in c.rows for cc, v in r)
    bits = c.x.view(np.uint64)
    bits[owned] = FLOW_SENTINEL
    bits[halo] = FLOW_SENTINEL
    c.sentinel_positions = (owned, halo)
    return c


_ALL = []


def all_cases():
    if not _ALL:
        for f in (flow_lpr_cases, flow_grid_cases, flow_gate_cases, chain_short_cases, chain_long_cases, level_launch_cases,
                  oddity_cases):
            _ALL.extend(f())
        names = [c.name for c in _ALL]
        assert len(set(names)) == len(names)
        for c in _ALL:
            assert c.n <= 5000 and c.nnz <= 70000, (c.name, c.n, c.nnz)
    return _ALL


# ---------------------------------------------------------------------------------------------- model and oracle
def model(case, seq, bsr1, x, b, mutate=None):
    """the sequential sweeps in plain Python floats: relaxation.h:34-62 (bsr1 false) and :90-173 with 1 x 1 blocks (true).
    mutate: one of SENSITIVITY[:3] -- a deliberately wrong variant for the sensitivity checks"""
    x = [float(v) for v in x]
    b = [float(v) for v in b]
    tasks = case.tasks()
    lev = None
    if mutate == "stale_operand":
        level_ptr, order = case.levels()
        lev = {}
        for l in range(len(level_ptr) - 1):
            for k in range(level_ptr[l], level_ptr[l + 1]):
                lev.setdefault(tasks[order[k]], l)
    for d in seq:
        x0 = list(x)
        for i in (reversed(tasks) if d else tasks):
            row = case.rows[i]
            if mutate == "reversed_sum":
                row = row[::-1]
            rsum = b[i] if bsr1 else 0.0
            diag, have = 0.0, False
            for c, v in row:
                if c == i:
                    if mutate == "first_diagonal" and have:
                        continue
                    if mutate == "reversed_sum" and have:
                        continue                            # (the reversed walk meets the LAST diagonal first)
                    diag, have = v, True
                else:
                    xc = x[c]
                    if lev is not None and c in lev and lev[c] == lev[i] + (1 if d else -1):
                        xc = x0[c]
                    rsum = (rsum - v * xc) if bsr1 else (rsum + v * xc)
            if have and diag != 0.0:
                x[i] = (rsum / diag) if bsr1 else ((b[i] - rsum) / diag)
    return np.array(x, dtype=np.float64)


def oracle(case, seq, bsr1, x, b):
    """the same sweeps through the C oracle (tests/oracle_lib.py)"""
    import oracle_lib
    lib = oracle_lib.load()
    x = np.array(x, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    bb = b
    if case.ncols > case.n and bsr1:                       # the block routine indexes b like x
        bb = np.concatenate((b, np.zeros(case.ncols - case.n)))
    ip, dp = oracle_lib.ip, oracle_lib.dp
    n = case.n
    for d in seq:
        if case.order is None:
            lo, hi, st = (n - 1, -1, -1) if d else (0, n, 1)
            if bsr1:
                lib.oracle_bsr_gauss_seidel(ip(case.Ap), ip(case.Aj), dp(case.Ax), dp(x), dp(bb), lo, hi, st, 1)
            else:
                lib.oracle_gauss_seidel(ip(case.Ap), ip(case.Aj), dp(case.Ax), dp(x), dp(bb), lo, hi, st)
        elif not bsr1:
            m = len(case.order)
            lo, hi, st = (m - 1, -1, -1) if d else (0, m, 1)
            lib.oracle_gauss_seidel_indexed(ip(case.Ap), ip(case.Aj), dp(case.Ax), dp(x), dp(bb), ip(case.order), lo, hi, st)
        else:
            for i in (case.order[::-1] if d else case.order):      # the block routine, one listed row at a time
                i = int(i)
                lib.oracle_bsr_gauss_seidel(ip(case.Ap), ip(case.Aj), dp(case.Ax), dp(x), dp(bb), i, i + 1, 1, 1)
    return x


def bit_mismatches(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))
