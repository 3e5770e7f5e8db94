"""BSR operators with DESIGNED dependency levels for the block smoother kernel set (tests/test_block_cases_host.py pins
them on the host, tests/test_gpu_block_forms.py sweeps them on the device).  No GPU, no torch.

The block analogue of gs_cases.layered: the block rows are numbered level by level, a block row of level l holds one
block into level l - 1, further blocks into chosen earlier and later levels (never its own), or is pinned by a READER of
level l - 1; stored order is shuffled.  The block PATTERN is the scalar pattern gs_cases.layered builds; every entry of
it becomes a bs x bs block here.  build_levels is gs_cases.build_levels on block rows; selection() restates the choices
of build_block_schedule (csrc/hier.hip), build_block_flow_form (csrc/gsflow.hip) and build_bsell / build_bsell_levels
(csrc/sell.hip), field by field as amg_hier_block_info reports them.

Values: every block entry is a random non-dyadic number of magnitude 0.1 .. 1; the diagonal block's diagonal dominates
its scalar row (nine sweeps of every kind stay finite); every fifth block row stores its diagonal block twice (the last
one counts for the point flavours, relaxation.h:127-129; the block flavours leave out both, :785).  Dinv is given
explicitly: the float64 inverse of the last stored diagonal block unless a case says otherwise."""
import numpy as np

import gs_cases as gc

INFO_FIELDS = ("levels", "bs", "flow", "seg", "lpr", "rows_per_chunk", "nchunks", "slot_rows", "level_copy", "slices",
               "scheduled", "longest")
KINDS = ("block_gauss_seidel", "block_jacobi", "bsr_gauss_seidel", "bsr_jacobi")
SEQS = {"block_gauss_seidel": ([0], [1], [0, 1]), "bsr_gauss_seidel": ([0], [1], [0, 1]),
        "block_jacobi": ([0], [1], [0, 1]), "bsr_jacobi": ([0], [0, 0])}       # (bsr_jacobi has no backward form: relaxation.h:303)
NINE = [0, 1, 1, 0, 0, 1, 0, 1, 1]
OMEGA = 0.7300000190734863
NONDYADIC = 1.0000001192092896
SENSITIVITY = ("reversed_sum", "running_sum", "stale_operand", "dinv_transposed", "diag_in_sum", "intra_ascending",
               "first_diagonal")
# the kinds a deliberately wrong variant can show in
MUTATION_KINDS = {"reversed_sum": KINDS, "running_sum": KINDS, "stale_operand": ("block_gauss_seidel", "bsr_gauss_seidel"),
                  "dinv_transposed": ("block_gauss_seidel", "block_jacobi"), "diag_in_sum": KINDS,
                  "intra_ascending": ("bsr_gauss_seidel",), "first_diagonal": ("bsr_gauss_seidel", "bsr_jacobi")}
FLOW_FORMS = {1: (8, 1), 2: (8, 2), 3: (5, 3), 4: (8, 4), 8: (8, 8), 16: (8, 16)}       # lanes per scalar row -> (seg, lpr)
BSL_WIN, BSL_PASS, TILE = 32, 8, 2048


class BlockCase(object):
    def __init__(self, name, family, bs, nb, Ap, Aj, Ax, Dinv, widths=None, expect=None, exempt=(), longest=None, props=None,
                 vectorised=False):
        self.name, self.family, self.bs, self.nb = name, family, int(bs), int(nb)
        self.Ap = np.ascontiguousarray(Ap, dtype=np.intc)
        self.Aj = np.ascontiguousarray(Aj, dtype=np.intc)
        self.Ax = np.ascontiguousarray(Ax, dtype=np.float64).ravel()
        self.Dinv = np.ascontiguousarray(Dinv, dtype=np.float64).ravel()
        self.widths = None if widths is None else [int(w) for w in widths]
        self.expect = dict(expect or {})                  # amg_hier_block_info fields stated by hand (block_gauss_seidel, flow 2)
        self.exempt = frozenset(exempt)                   # sensitivity checks that cannot change a bit here
        self.longest = longest                            # designed longest off-diagonal block count (None: not stated)
        self.props = dict(props or {})
        self.vectorised = vectorised                      # too large for Python loops: the model runs level by level in numpy
        self.nblocks = int(self.Ap[-1])
        assert len(self.Aj) == self.nblocks and len(self.Ax) == self.nblocks * bs * bs and len(self.Dinv) == nb * bs * bs
        rng = np.random.RandomState(len(name) * 7919 + nb)
        self.b = rng.uniform(-1.0, 1.0, nb * bs) * 3.1
        self.x = rng.uniform(-1.0, 1.0, nb * bs) * 1.7
        self._levels = self._lists = self._level_of = None
        self._sel = {}

    def __repr__(self):
        return self.name

    def pattern(self):
        """per block row [(block column, None)] in stored order: what gs_cases.build_levels walks"""
        Ap, Aj = self.Ap.tolist(), self.Aj.tolist()
        return [[(c, None) for c in Aj[Ap[i]:Ap[i + 1]]] for i in range(self.nb)]

    def levels(self, tasks=None):
        """(level_ptr, order) of the restated build_levels on block rows; the full range is computed once"""
        if tasks is not None:
            return gc.build_levels(self.nb, self.pattern(), list(tasks))
        if self._levels is None:
            self._levels = gc.build_levels(self.nb, self.pattern(), list(range(self.nb)))
        return self._levels

    def level_of(self):
        if self._level_of is None:
            level_ptr, order = self.levels()
            lev = np.zeros(self.nb, dtype=np.int64)
            for l in range(len(level_ptr) - 1):
                lev[np.asarray(order[level_ptr[l]:level_ptr[l + 1]], dtype=np.int64)] = l
            self._level_of = lev
        return self._level_of

    def lists(self):
        if self._lists is None:
            self._lists = (self.Ap.tolist(), self.Aj.tolist(), self.Ax.tolist(), self.Dinv.tolist())
        return self._lists

    def offdiag_counts(self):
        rows = np.repeat(np.arange(self.nb), np.diff(self.Ap))
        return np.bincount(rows[self.Aj != rows], minlength=self.nb)

    def longest_offdiag(self):
        return int(self.offdiag_counts().max()) if self.nb else 0

    def info(self, smoother="block_gauss_seidel", flow_mode=2, sell_levels=False):
        key = (smoother, flow_mode, sell_levels)
        if key not in self._sel:
            self._sel[key] = selection(self, smoother, flow_mode, sell_levels)
        return self._sel[key]


# ---------------------------------------------------------------------------------------------- restated host rules
def _sliced(lengths, nblocks, bs, windows, factor):
    """csrc/sell.hip build_bsell_bs: every window of 32 slices sorts its block rows by block count, descending; a slice
    stores as many blocks per row as its first row holds; the form is dropped when the padding exceeds `factor`"""
    nbr = 64 // bs
    cols = 0
    for w0, wl in windows:
        seg = np.sort(lengths[w0:w0 + wl])[::-1]
        cols += int(seg[::nbr].sum())
    if cols * nbr > factor * nblocks or (len(lengths) and int(lengths.max()) > 60000):
        return 0
    return len(windows) * BSL_WIN


def _sliceable(case):
    return case.bs in (2, 3) and case.nb >= (1 << 15) and 4 * case.nb <= case.nblocks <= 48 * case.nb


def operator_slices(case):
    """build_bsell: the whole operator in its own row order (block Jacobi passes, operator applications)"""
    if not _sliceable(case):
        return 0
    win = BSL_WIN * (64 // case.bs)
    windows = [(w0, min(win, case.nb - w0)) for w0 in range(0, case.nb, win)]
    return _sliced(np.diff(case.Ap), case.nblocks, case.bs, windows, 1.15)


def level_slices(case, level_ptr, order, forced):
    """build_bsell_levels: the level-ordered copy, windows cut at the level boundaries"""
    nl = len(level_ptr) - 1
    if not _sliceable(case) or (not forced and nl * 8192 > case.nb):
        return 0
    win = BSL_WIN * (64 // case.bs)
    windows = [(w0, min(win, level_ptr[l + 1] - w0)) for l in range(nl) for w0 in range(level_ptr[l], level_ptr[l + 1], win)]
    return _sliced(np.diff(case.Ap)[np.asarray(order, dtype=np.int64)], case.nblocks, case.bs, windows, 1.3)


def flow_form(bs, level_ptr, cnt, ntasks, nb):
    """csrc/gsflow.hip build_block_flow_form.  cnt: off-diagonal block count by level-order position.  Returns the form's
    fields (flow 0 with the counted longest row when it declines after counting; None when it declines before)"""
    nl = len(level_ptr) - 1
    if nb <= 0 or ntasks != nb or nl <= 0 or bs not in (2, 3):
        return None
    longest = max(cnt) if len(cnt) else 0
    if longest > 128:
        return dict(flow=0, longest=longest)
    lpr = 1
    while 8 * lpr < longest:
        lpr *= 2
    seg = 8
    if 9 <= longest <= 15:
        seg, lpr = 5, 3
    R = 64 // (bs * lpr)
    nchunks = slot_rows = 0
    chunk_slots = []
    for l in range(nl):
        lo, hi = level_ptr[l], level_ptr[l + 1]
        ordl = sorted(range(lo, hi), key=lambda k: -((cnt[k] + lpr - 1) // lpr))           # stable
        for r0 in range(lo, hi, R):
            ns = (cnt[ordl[r0 - lo]] + lpr - 1) // lpr
            chunk_slots.append(ns)
            nchunks += 1
            slot_rows += ns
    return dict(flow=1, seg=seg, lpr=lpr, rows_per_chunk=R, nchunks=nchunks, slot_rows=slot_rows, longest=longest,
                chunk_slots=chunk_slots)


def selection(case, smoother="block_gauss_seidel", flow_mode=2, sell_levels=False, tasks=None):
    """The twelve fields of amg_hier_block_info for `smoother` as the coarse smoother of a one-level hierarchy over the
    case, built under amg_set_gs_flow(flow_mode) (sell_levels: AMG_SELL_LEVELS=1).  tasks: a flat entry's row list
    instead of the whole range -- what its block schedule would hold."""
    out = dict.fromkeys(INFO_FIELDS, 0)
    out["bs"] = case.bs
    if smoother in ("block_jacobi", "jacobi"):
        out.update(slices=operator_slices(case), scheduled=case.nb)
        return out
    level_ptr, order = case.levels(tasks)
    ntasks = case.nb if tasks is None else len(tasks)
    rows = order if tasks is None else [tasks[t] for t in order]
    out.update(levels=len(level_ptr) - 1, scheduled=ntasks, level_copy=1)
    form = None
    if smoother == "block_gauss_seidel" and flow_mode != 0 and case.bs in (2, 3):
        once = ntasks == case.nb and len(set(rows)) == case.nb
        if once:                                            # (every block column of the cases is in range)
            cnt = case.offdiag_counts()[np.asarray(rows, dtype=np.int64)].tolist()
            form = flow_form(case.bs, level_ptr, cnt, ntasks, case.nb)
    if form:
        out.update({k: v for k, v in form.items() if k in out})
        out["chunk_slots"] = form.get("chunk_slots", [])    # not an info field
    if out["flow"]:
        out["level_copy"] = 0                               # the form serves the schedule alone
    else:
        out["slices"] = level_slices(case, level_ptr, rows, sell_levels)
    return out


# ---------------------------------------------------------------------------------------------- the layered generator
def _blocks(rng, count, bs):
    v = rng.uniform(0.1, 1.0, (count, bs, bs)) * np.where(rng.rand(count, bs, bs) < 0.5, 1.0, -1.0)
    return v * NONDYADIC


def assemble(name, family, bs, pattern, seed, dinv="inverse", **kw):
    """pattern: per block row [(block column, kind)] in stored order, kind one of 'off', 'zero' (an explicit zero block),
    'diag' (the last one stored dominates; an earlier one is overridden), 'diag_zero' (a dominating diagonal block with
    one zero on its own diagonal).  dinv: 'inverse' | 'random' (blocks that are no inverse of anything)"""
    rng = np.random.RandomState(seed)
    nb = len(pattern)
    Ap = np.zeros(nb + 1, dtype=np.int64)
    Ap[1:] = np.cumsum([len(r) for r in pattern])
    Aj = np.array([c for r in pattern for c, k in r], dtype=np.int64)
    kinds = [k for r in pattern for c, k in r]
    A = _blocks(rng, len(kinds), bs)
    rows = np.repeat(np.arange(nb), np.diff(Ap))
    isdiag = Aj == rows
    for q, k in enumerate(kinds):
        assert (k in ("diag", "diag_zero")) == bool(isdiag[q]), (name, q, k)
        if k == "zero":
            A[q] = 0.0
    # scalar row sums of everything off the diagonal blocks
    rowabs = np.zeros((nb, bs))
    np.add.at(rowabs, rows[~isdiag], np.abs(A[~isdiag]).sum(axis=2))
    eye = np.eye(bs, dtype=bool)
    last = {}
    for q in np.nonzero(isdiag)[0]:
        last[int(rows[q])] = int(q)
    Dinv = _blocks(rng, nb, bs)                             # rows without a diagonal block keep a random block
    scale = 1.0 / (2.0 * rowabs.sum(axis=1) + 2.0 * bs)
    Dinv *= scale[:, None, None]
    for q in np.nonzero(isdiag)[0]:
        i = int(rows[q])
        D = A[q] * 0.3
        inner = np.abs(np.where(eye, 0.0, D)).sum(axis=1)
        dom = (rowabs[i] + inner + 1.0) * rng.uniform(1.5, 2.5, bs) * NONDYADIC
        D[eye] = dom * (1.0 if last[i] == q else 0.37)
        if kinds[q] == "diag_zero":
            D[i % bs, i % bs] = 0.0
        A[q] = D
        if last[i] == q and dinv == "inverse":
            Dinv[i] = np.linalg.inv(D)
    return BlockCase(name, family, bs, nb, Ap, Aj, A, Dinv, **kw)


def layered(name, family, bs, widths, spec, seed, double_diag=5, sort=None, dinv="inverse", **kw):
    """spec(l, p) as for gs_cases.layered (lower, upper, fill, pin, dup, zero, diag), plus
         diag_at: stored position of the (single) diagonal block in this block row"""
    base = gc.layered(name, family, widths, spec, seed, double_diag=double_diag, sort=sort)
    start = np.concatenate(([0], np.cumsum(widths))).astype(int)
    pattern = []
    for l in range(len(widths)):
        for p in range(widths[l]):
            i = int(start[l]) + p
            s = spec(l, p) or {}
            row = []
            for c, v in base.rows[i]:
                if c == i:
                    row.append((c, "diag_zero" if v == 0.0 else "diag"))
                else:
                    row.append((c, "zero" if v == 0.0 else "off"))
            if "diag_at" in s:
                d = [e for e in row if e[0] == i]
                assert len(d) == 1, (name, i)
                row = [e for e in row if e[0] != i]
                row.insert(min(int(s["diag_at"]), len(row)), d[0])
            pattern.append(row)
    return assemble(name, family, bs, pattern, seed + 1, dinv=dinv, widths=list(widths), **kw)


generic = gc.generic


def form_for(L):
    """(seg, lpr) build_block_flow_form picks for a longest off-diagonal block count L, None when it declines"""
    if L > 128:
        return None
    if 9 <= L <= 15:
        return 5, 3
    lpr = 1
    while 8 * lpr < L:
        lpr *= 2
    return 8, lpr


# ---------------------------------------------------------------------------------------------- the families
LPR_LONGEST = (0, 1, 8, 9, 15, 16, 17, 32, 33, 64, 65, 128, 129)
LPR_FORMS = ((8, 1),) * 3 + ((5, 3),) * 2 + ((8, 2),) + ((8, 4),) * 2 + ((8, 8),) * 2 + ((8, 16),) * 2 + (None,)


def bflow_lpr_cases():
    out = []
    for bs in (2, 3):
        for L, want in zip(LPR_LONGEST, LPR_FORMS):
            form = form_for(L) or (8, 16)
            R = 64 // (bs * form[1])
            name = "bflow_lpr_bs%d_%d" % (bs, L)
            if L == 0:
                # no off-diagonal block at all: one level of 2 R + 1 diagonal-only block rows, three chunks without slots
                out.append(layered(name, "bflow_lpr", bs, [2 * R + 1], lambda l, p: {}, 1000 + bs, longest=0,
                                   exempt=("reversed_sum", "running_sum", "stale_operand"),
                                   expect=dict(levels=1, flow=1, seg=8, lpr=1, rows_per_chunk=R, nchunks=3, slot_rows=0),
                                   props=dict(R=R, long_rows=[])))
                continue
            wide = max(R + 2, 5)
            widths = [L + 2 * R + 5] + [w for w in (R - 1, R, R + 1) if w >= 1] + [wide, 3]
            nl = len(widths)
            at_R = widths.index(R, 1)
            long_rows = [(at_R, min(1, R - 1)), (nl - 2, 3)]     # where the width equals R, and near the end

            def spec(l, p, L=L, nl=nl, long_rows=long_rows):
                if l == nl - 1:
                    return dict(pin="reader")               # the last level: diagonal-only rows, placed by readers
                if L == 1:
                    if p < 3:                               # three chains of rows with one later block each
                        return dict(pin="reader") if l >= 1 else {}
                    return dict(upper=[1]) if (l == 0 and p % 2) else {}
                if l == 0:
                    return dict(upper=[1, 2]) if p % 3 == 0 else {}
                if (l, p) in long_rows:
                    return dict(fill=L - 1)
                k = p % 4
                if k == 0:
                    return dict(lower=[1, 2])
                if k == 1:
                    return dict(upper=[1])
                if k == 2:
                    return dict(fill=L // 2 - 1)            # half as long: another slot count inside the level
                return {}
            exp = dict(levels=nl, flow=int(want is not None), longest=L)
            if want:
                exp.update(seg=want[0], lpr=want[1], rows_per_chunk=R, nchunks=sum((w + R - 1) // R for w in widths))
            else:
                exp.update(level_copy=1, nchunks=0)
            out.append(layered(name, "bflow_lpr", bs, widths, spec, 1000 + 10 * L + bs, longest=L, expect=exp,
                               exempt=("reversed_sum", "running_sum") if L == 1 else (),
                               props=dict(R=R, long_rows=long_rows)))
    return out


def _grid_widths(nchunks, R):
    pat, w, k = (R + 1, R // 3 + 1, R, 2, 2 * R + 2), [], 0
    left = nchunks
    while left > 0:
        c = pat[k % len(pat)]
        if (c + R - 1) // R > left:
            c = R // 2 + 1
        w.append(c)
        left -= (c + R - 1) // R
        k += 1
    return w


def bflow_grid_cases():
    out = []
    R = {2: 32, 3: 21}
    # one block row in all; one chunk in all (a single level cannot hold an off-diagonal block)
    out.append(layered("bflow_grid_bs3_one", "bflow_grid", 3, [1], lambda l, p: {}, 2001, longest=0,
                       exempt=("reversed_sum", "running_sum", "stale_operand", "first_diagonal"),
                       expect=dict(levels=1, flow=1, seg=8, lpr=1, nchunks=1, slot_rows=0, scheduled=1)))
    out.append(layered("bflow_grid_bs2_one_chunk", "bflow_grid", 2, [R[2] - 2], lambda l, p: {}, 2002, double_diag=3, longest=0,
                       exempt=("reversed_sum", "running_sum", "stale_operand"),
                       expect=dict(levels=1, flow=1, seg=8, lpr=1, nchunks=1, slot_rows=0)))
    for bs in (2, 3):
        # three chunks: with any sequence of at most four sweeps the launch stays below the 32-wave floor
        out.append(layered("bflow_grid_bs%d_3" % bs, "bflow_grid", bs, [R[bs], R[bs] - 1, 5], generic, 2010 + bs,
                           expect=dict(levels=3, flow=1, seg=8, lpr=1, rows_per_chunk=R[bs], nchunks=3)))
        for k in (31, 32, 33):
            w = _grid_widths(k, R[bs])
            out.append(layered("bflow_grid_bs%d_%d" % (bs, k), "bflow_grid", bs, w, generic, 2020 + 3 * k + bs,
                               expect=dict(levels=len(w), flow=1, seg=8, lpr=1, rows_per_chunk=R[bs], nchunks=k)))
        # twelve levels of twelve chunks: look-ahead 50 and four sweeps ask for 576 waves, cut to 512 -- flow_slot deals them
        out.append(layered("bflow_grid_bs%d_wide" % bs, "bflow_grid", bs, [12 * R[bs]] * 12, generic, 2200 + bs,
                           expect=dict(levels=12, flow=1, seg=8, lpr=1, rows_per_chunk=R[bs], nchunks=144)))
    return out


def bflow_gate_cases():
    def spec(l, p):
        k = p % 6
        if k == 0:
            return dict(lower=[1])                          # operands exactly one level back
        if k == 1:
            return dict(pin="reader", lower=[2])           # exactly two back: that operand is the gate
        if k == 2:
            return dict(pin="reader", lower=[5, 7, 9])     # many levels back
        if k == 3:
            return dict(pin="reader", upper=[1, 2])        # later levels only: the gate is the zero position
        if k == 4:
            return dict(lower=[1, 2, 3], upper=[1, 2, 3])
        return dict(lower=[1], upper=[3])
    out = []
    for bs, R in ((2, 32), (3, 21)):
        out.append(layered("bflow_gate_bs%d_narrow" % bs, "bflow_gate", bs, [R // 2] * 12, spec, 3000 + bs,
                           expect=dict(levels=12, flow=1, seg=8, lpr=1, rows_per_chunk=R, nchunks=12)))
        out.append(layered("bflow_gate_bs%d_wide" % bs, "bflow_gate", bs, [2 * R + 5, R + 3, 3 * R + 1] * 4, spec, 3010 + bs,
                           expect=dict(levels=12, flow=1, seg=8, lpr=1, rows_per_chunk=R, nchunks=36)))
    return out


STREAM_BS = (2, 3, 4, 5, 6, 7, 16)


def stream_cases():
    out = []
    for bs in STREAM_BS:
        w = 256 // bs
        T = (TILE - 1) // (bs * bs)                         # whole blocks of one LDS tile
        long = T + 2                                        # a block row of two tiles
        widths = [max(long + 8, 30), w - 1, w, w + 1, 1, 7]
        # the long block rows are the first of their level -- the first of a workgroup, whose tiles start with them: the
        # diagonal block first in the first tile, last in it, first in the second tile, last of the row
        place = {1: 0, 2: T - 1, 3: T, 4: T + 1}

        def spec(l, p, place=place, long=long):
            if l in place and p == 0:
                return dict(fill=long - 2, diag="once", diag_at=place[l])
            if l == 0 and p == 5:
                return dict(diag="missing")                 # an empty block row
            if l == 0:
                return dict(upper=[1, 2]) if p % 2 else {}
            return generic(l, p)
        exp = dict(levels=len(widths), flow=0, level_copy=1)
        if bs in (2, 3):
            exp.update(longest=long - 1)                    # counted, then declined: more than 128 blocks
        out.append(layered("stream_bs%d" % bs, "stream", bs, widths, spec, 4000 + bs, longest=long - 1, expect=exp,
                           props=dict(long_rows=[(l, 0) for l in place], diag_at=place, tile_blocks=T, empty_row=5)))
    return out


def sliced_case(bs, drop_last=False):
    """2^15 block rows (one fewer with drop_last) of 4 to 12 blocks in five wide levels, built with numpy"""
    nb = (1 << 15) - (1 if drop_last else 0)
    win = BSL_WIN * (64 // bs)
    widths = [15000, win - 172, 9000, 7000]
    widths.append(nb - sum(widths))
    rng = np.random.RandomState(5000 + bs)
    start = np.concatenate(([0], np.cumsum(widths)))
    lev = np.repeat(np.arange(len(widths)), widths)
    i = np.arange(nb)
    k = rng.randint(3, 12, nb)                              # off-diagonal blocks: 4 .. 12 blocks with the diagonal one
    k[:16] = (7, 8) * 8                                     # rows of 8 and 9 blocks: one and two passes of BSL_PASS
    cnt = k + 1
    Ap = np.concatenate(([0], np.cumsum(cnt)))
    rows = np.repeat(i, cnt)
    slot = np.arange(Ap[-1]) - Ap[rows]                    # 0: the diagonal block, 1: the block into the level before, ...
    wl, sl = np.asarray(widths)[lev], start[lev]
    other = rng.randint(0, 1 << 30, Ap[-1]) % (nb - wl[rows])
    other = np.where(other >= sl[rows], other + wl[rows], other)          # any block row outside the row's own level
    prev = np.maximum(lev - 1, 0)
    before = start[prev][rows] + rng.randint(0, 1 << 30, Ap[-1]) % np.asarray(widths)[prev][rows]
    Aj = np.where(slot == 0, rows, np.where((slot == 1) & (lev[rows] > 0), before, other))
    perm = np.lexsort((rng.rand(Ap[-1]), rows))             # stored order shuffled inside every block row
    Aj = Aj[perm]
    isdiag = Aj == rows
    A = _blocks(rng, Ap[-1], bs)
    rowabs = np.zeros((nb, bs))
    np.add.at(rowabs, rows[~isdiag], np.abs(A[~isdiag]).sum(axis=2))
    eye = np.eye(bs, dtype=bool)
    D = A[isdiag] * 0.3
    inner = np.abs(np.where(eye, 0.0, D)).sum(axis=2)
    D[:, eye] = (rowabs + inner + 1.0) * rng.uniform(1.5, 2.5, (nb, bs)) * NONDYADIC
    A[isdiag] = D
    name = "sliced_bs%d%s" % (bs, "_minus_one" if drop_last else "")
    return BlockCase(name, "sliced", bs, nb, Ap, Aj, A, np.linalg.inv(D), widths=widths, vectorised=True,
                     exempt=("first_diagonal",), expect=dict(levels=5, flow=1, seg=5, lpr=3),
                     props=dict(window=win))


_SLICED = {}


def sliced_cases():
    for bs in (3, 2):
        if bs not in _SLICED:
            _SLICED[bs] = sliced_case(bs)
    return [_SLICED[3], _SLICED[2]]


def sliced_minus_one():
    if "m1" not in _SLICED:
        _SLICED["m1"] = sliced_case(3, drop_last=True)
    return _SLICED["m1"]


SHORT_WIDTHS = [30] * 5 + [100] + [30] * 4
LONG_WIDTHS = [60, 12, 12, 12, 30, 12, 12]


def _short(name, mod=None, **kw):
    exp = kw.pop("expect", {})
    return layered("odd_short_" + name, "oddities", 3, SHORT_WIDTHS, lambda l, p: dict(generic(l, p), **((mod(l, p) if mod else None) or {})),
                   6000 + len(name), expect=dict(dict(levels=10, flow=1, seg=8, lpr=1, rows_per_chunk=21), **exp), **kw)


def _long(name, mod=None, **kw):
    exp = kw.pop("expect", {})

    def spec(l, p):
        if l == 0:
            s = dict(upper=[1, 2])
        elif p % 3 == 0:
            s = dict(fill=23)
        else:
            s = generic(l, p)
        s.update((mod(l, p) if mod else None) or {})
        return s
    return layered("odd_long_" + name, "oddities", 2, LONG_WIDTHS, spec, 7000 + len(name),
                   expect=dict(dict(levels=7, flow=1, seg=8, lpr=4, rows_per_chunk=8), **exp), **kw)


def oddity_cases():
    out = []

    def both(name, mod=None, **kw):
        out.append(_short(name, mod, **kw))
        out.append(_long(name, mod, **kw))
    both("plain")                                           # the flat entries sweep these over sub-ranges, strides, backward
    both("descending", sort="descending")
    both("duplicates", lambda l, p: dict(dup=True))
    both("zeros", lambda l, p: dict(zero=True))
    both("diag_twice", lambda l, p: dict(diag="twice"))
    # block flavours apply Dinv all the same; the point flavours leave the block row / the scalar row as it is
    both("missing_diag", lambda l, p: dict(diag="missing") if p == 2 and l in (1, 3, 5) else {})
    both("zero_in_diag", lambda l, p: dict(diag="zero") if p == 2 and l in (1, 3, 5) else {})
    both("dinv_not_inverse", dinv="random")
    return out


_ALL = []


def all_cases():
    if not _ALL:
        for f in (bflow_lpr_cases, bflow_grid_cases, bflow_gate_cases, stream_cases, sliced_cases, oddity_cases):
            _ALL.extend(f())
        names = [c.name for c in _ALL]
        assert len(set(names)) == len(names)
        for c in _ALL:
            assert c.family == "sliced" or (c.nb <= 5000 and len(c.Ax) <= 200000), (c.name, c.nb, len(c.Ax))
    return _ALL


def flat_ranges(nb):
    """(start, stop, step) over block rows for the flat entries: the whole range both ways, a sub-range, a stride, a
    backward sub-range.  All but the first two make ntasks != nb: the dataflow form must decline."""
    return {"all_fwd": (0, nb, 1), "all_bwd": (nb - 1, -1, -1), "sub_fwd": (5, nb - 7, 1),
            "stride2_fwd": (3, 3 + 2 * ((nb - 7) // 2), 2), "sub_bwd": (nb - 8, 4, -1)}


def flat_calls(case, rng3):
    """(fn, args) for the four block entries of the amg_core table over one range, as flat_ranges.call_table takes them"""
    rng = np.random.RandomState(case.nb + 17)
    temp = rng.uniform(-1.0, 1.0, case.nb * case.bs)
    omega = np.array([OMEGA])
    B = [("Ap", case.Ap), ("Aj", case.Aj), ("Ax", case.Ax), ("x", case.x), ("b", case.b)]
    r3 = [("rs", rng3[0]), ("re", rng3[1]), ("rt", rng3[2])]
    yield "bsr_gauss_seidel", B + r3 + [("bs", case.bs)]
    yield "block_gauss_seidel", B + [("Dinv", case.Dinv)] + r3 + [("bs", case.bs)]
    yield "block_jacobi", B + [("Dinv", case.Dinv), ("temp", temp)] + r3 + [("omega", omega), ("bs", case.bs)]
    if rng3[2] > 0:
        yield "bsr_jacobi", B + [("temp", temp)] + r3 + [("bs", case.bs), ("omega", omega)]


# ---------------------------------------------------------------------------------------------- model and oracle
def _range(case, d):
    if isinstance(d, tuple):
        return d
    return (case.nb - 1, -1, -1) if d else (0, case.nb, 1)


def model(case, kind, seq, x, b, mutate=None):
    """the sequential sweeps in plain Python floats: block_gauss_seidel (relaxation.h:756-810), block_jacobi (:661-728),
    bsr_gauss_seidel (:90-173), bsr_jacobi (:267-360).  seq: one entry per sweep, 0 forward / 1 backward over all block
    rows or a (start, stop, step) triple.  mutate: one of SENSITIVITY -- a deliberately wrong variant"""
    assert kind in KINDS and (mutate is None or mutate in SENSITIVITY)
    if case.vectorised:
        return model_by_levels(case, kind, seq, x, b, mutate)
    bs = case.bs
    B2 = bs * bs
    Ap, Aj, Ax, Dinv = case.lists()
    x = [float(v) for v in x]
    b = [float(v) for v in b]
    point = kind.startswith("bsr_")
    jacobi = kind.endswith("jacobi")
    lev = case.level_of().tolist() if mutate == "stale_operand" else None
    R = range(bs)
    for d in seq:
        start, stop, step = _range(case, d)
        back = step < 0
        x0 = list(x)
        src = x0 if jacobi else x                           # Jacobi reads the copy (temp), Gauss-Seidel the live iterate
        intra = list(reversed(R)) if (back and mutate != "intra_ascending") else list(R)
        for i in range(start, stop, step):
            ib = i * bs
            blocks = range(Ap[i], Ap[i + 1])
            dptr = -1
            for jj in blocks:
                if Aj[jj] == i and not (mutate == "first_diagonal" and dptr != -1):
                    dptr = jj * B2
            if mutate == "reversed_sum":
                blocks = reversed(blocks)
            rs = [b[ib + k] for k in R] if point else [0.0] * bs
            for jj in blocks:
                j = Aj[jj]
                if j == i and mutate != "diag_in_sum":
                    continue
                op = src
                if lev is not None and lev[j] == lev[i] + (1 if back else -1):
                    op = x0
                o, xo = jj * B2, j * bs
                xs = [op[xo + c] for c in R]
                for r in R:
                    if mutate == "running_sum":
                        s = rs[r]
                        for c in R:
                            p = Ax[o + r * bs + c] * xs[c]
                            s = (s - p) if point else (s + p)
                        rs[r] = s
                    else:
                        v = 0.0
                        for c in R:
                            v = v + Ax[o + r * bs + c] * xs[c]
                        rs[r] = (rs[r] - v) if point else (rs[r] + v)
            if not point:
                t = [b[ib + k] - rs[k] for k in R]
                D = i * B2
                for r in R:
                    v = 0.0
                    for c in R:
                        v = v + (Dinv[D + c * bs + r] if mutate == "dinv_transposed" else Dinv[D + r * bs + c]) * t[c]
                    rs[r] = v
                for k in R:
                    x[ib + k] = ((1.0 - OMEGA) * x0[ib + k] + OMEGA * rs[k]) if jacobi else rs[k]
            elif dptr != -1:
                for k in intra:
                    diag = 1.0
                    for kk in intra:
                        if k == kk:
                            diag = Ax[dptr + k * bs + kk]
                        else:
                            rs[k] = rs[k] - Ax[dptr + k * bs + kk] * src[ib + kk]
                    if diag != 0.0:
                        x[ib + k] = ((1.0 - OMEGA) * x0[ib + k] + OMEGA * rs[k] / diag) if jacobi else rs[k] / diag
    return np.array(x, dtype=np.float64)


def model_by_levels(case, kind, seq, x, b, mutate=None):
    """the same arithmetic, one dependency level at a time in numpy (elementwise products and sums in the sequential
    order; block rows of a level do not read each other).  Whole-range sweeps only."""
    bs, nb = case.bs, case.nb
    point = kind.startswith("bsr_")
    jacobi = kind.endswith("jacobi")
    A = case.Ax.reshape(-1, bs, bs)
    Dv = case.Dinv.reshape(nb, bs, bs)
    Ap, Aj = case.Ap.astype(np.int64), case.Aj.astype(np.int64)
    X = np.array(x, dtype=np.float64).reshape(nb, bs)
    B = np.asarray(b, dtype=np.float64).reshape(nb, bs)
    lev = case.level_of()
    if jacobi:
        groups = [np.arange(nb)]
    else:
        level_ptr, order = case.levels()
        order = np.asarray(order, dtype=np.int64)
        groups = [order[level_ptr[l]:level_ptr[l + 1]] for l in range(len(level_ptr) - 1)]
    for d in seq:
        assert not isinstance(d, tuple)
        back = bool(d) and not jacobi
        X0 = X.copy()
        intra = list(range(bs))[::-1] if (back and mutate != "intra_ascending") else list(range(bs))
        for idx in (groups[::-1] if back else groups):
            src = X0 if jacobi else X
            cnt = Ap[idx + 1] - Ap[idx]
            K = int(cnt.max()) if len(idx) else 0
            dptr = np.full(len(idx), -1, dtype=np.int64)
            for k in range(K):
                jj = np.minimum(Ap[idx] + k, len(Aj) - 1)
                hit = (k < cnt) & (Aj[jj] == idx)
                if mutate == "first_diagonal":
                    hit &= dptr < 0
                dptr = np.where(hit, jj, dptr)
            rs = B[idx].copy() if point else np.zeros((len(idx), bs))
            for k in range(K):
                off = (cnt - 1 - k) if mutate == "reversed_sum" else np.full(len(idx), k)
                m = k < cnt
                jj = np.clip(Ap[idx] + off, 0, len(Aj) - 1)
                j = Aj[jj]
                take = m & ((j != idx) | (mutate == "diag_in_sum"))
                xs = src[j]
                if mutate == "stale_operand":
                    stale = lev[j] == lev[idx] + (1 if back else -1)
                    xs = np.where(stale[:, None], X0[j], xs)
                Ab = A[jj]
                if mutate == "running_sum":
                    s = rs
                    for c in range(bs):
                        p = Ab[:, :, c] * xs[:, c][:, None]
                        s = (s - p) if point else (s + p)
                else:
                    v = np.zeros((len(idx), bs))
                    for c in range(bs):
                        v = v + Ab[:, :, c] * xs[:, c][:, None]
                    s = (rs - v) if point else (rs + v)
                rs = np.where(take[:, None], s, rs)
            if not point:
                t = B[idx] - rs
                Db = Dv[idx]
                y = np.zeros((len(idx), bs))
                for c in range(bs):
                    y = y + (Db[:, c, :] if mutate == "dinv_transposed" else Db[:, :, c]) * t[:, c][:, None]
                X[idx] = ((1.0 - OMEGA) * X0[idx] + OMEGA * y) if jacobi else y
            else:
                has = dptr >= 0
                Dg = A[np.maximum(dptr, 0)]
                xi = src[idx].copy()
                new = X[idx].copy()
                for k in intra:
                    r = rs[:, k]
                    for kk in intra:
                        if kk != k:
                            r = r - Dg[:, k, kk] * xi[:, kk]
                    diag = Dg[:, k, k]
                    ok = has & (diag != 0.0)
                    q = r / np.where(diag != 0.0, diag, 1.0)
                    if jacobi:
                        val = (1.0 - OMEGA) * X0[idx][:, k] + OMEGA * r / np.where(diag != 0.0, diag, 1.0)
                    else:
                        val = q
                        xi[:, k] = np.where(ok, val, xi[:, k])       # Gauss-Seidel inside the block: later rows read it
                    new[:, k] = np.where(ok, val, new[:, k])
                X[idx] = new
    return X.reshape(-1).copy()


def oracle(case, kind, seq, x, b):
    """the same sweeps through the C oracle (tests/oracle_lib.py)"""
    import oracle_lib
    lib = oracle_lib.load()
    ip, dp = oracle_lib.ip, oracle_lib.dp
    x = np.array(x, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    temp = np.zeros_like(x)
    omega = np.array([OMEGA])
    A = (ip(case.Ap), ip(case.Aj), dp(case.Ax))
    for d in seq:
        lo, hi, st = _range(case, d)
        if kind == "block_gauss_seidel":
            lib.oracle_block_gauss_seidel(A[0], A[1], A[2], dp(x), dp(b), dp(case.Dinv), lo, hi, st, case.bs)
        elif kind == "block_jacobi":
            lib.oracle_block_jacobi(A[0], A[1], A[2], dp(x), dp(b), dp(case.Dinv), dp(temp), lo, hi, st, dp(omega), case.bs)
        elif kind == "bsr_gauss_seidel":
            lib.oracle_bsr_gauss_seidel(A[0], A[1], A[2], dp(x), dp(b), lo, hi, st, case.bs)
        else:
            assert st > 0
            lib.oracle_bsr_jacobi(A[0], A[1], A[2], dp(x), dp(b), dp(temp), lo, hi, st, case.bs, dp(omega))
    return x


bit_mismatches = gc.bit_mismatches
