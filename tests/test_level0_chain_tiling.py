"""CPU restatement of the fused level-0 chains' tiling (kernels.hip level0_chain_kernel): the tile and halo index
arithmetic, the z march with its register windows and operand queues, and the LDS neighbour reads, replayed lane by
lane (vectorised over a workgroup's 32 x 16 lanes) on small odd grids, against the separate passes applied row by row.
Same slot order and the same separately rounded products in both, so the results must be the same bits."""
import numpy as np
import pytest

TX, TY = 32, 16        # the tile's extent in lanes (L0C_TX, L0C_TY)
ABSENT = 255


def box_codes(nx, ny, nz, ndict, rng):
    """Random codes of a 7-point stencil on the box, slot order (-P, -L, -1, 0, 1, L, P); couplings that would leave
    the box are absent."""
    n = nx * ny * nz
    codes = rng.randint(0, ndict, size=(n, 7))
    z, y, x = np.unravel_index(np.arange(n), (nz, ny, nx))
    inside = [z > 0, y > 0, x > 0, np.ones(n, bool), x < nx - 1, y < ny - 1, z < nz - 1]
    for u in range(7):
        codes[~inside[u], u] = ABSENT
    return codes


def row_sum(codes_row, dictv, xv, gscale):
    """coded_row_sum: terms in slot order, v * (gscale * x), absent slots skipped."""
    acc = np.zeros(np.broadcast(codes_row[..., 0], xv[0]).shape)
    for u in range(7):
        c = codes_row[..., u]
        on = c != ABSENT
        v = dictv[np.where(on, c, 0)]
        pr = v * (gscale * xv[u])
        acc = np.where(on, acc + pr, acc)
    return acc


def reference_chain(first_res, last_res, codes, dictv, dims, g0, x, b, c_gs, c_last):
    """The separate passes, each over all rows (stencil_coded_kernel)."""
    nx, ny, nz = dims
    off = [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
    n = nx * ny * nz
    idx = np.arange(n)

    def apply(vec, gscale):
        xv = [vec[np.clip(idx + o, 0, n - 1)] for o in off]
        return row_sum(codes, dictv, xv, gscale)

    r = b - apply(g0, 1.0) if first_res else g0
    xo = x if not first_res else g0
    xn = xo + (c_last * r + apply(r, c_gs))
    rn = b - apply(xn, 1.0) if last_res else None
    return xn, rn


def tiled_chain(first_res, last_res, codes, dictv, dims, g0, x, b, c_gs, c_last, zc):
    """level0_chain_kernel, one workgroup at a time."""
    nx, ny, nz = dims
    S = int(first_res) + 1 + int(last_res)
    SP = int(first_res) + 1
    INX, INY = TX - 2 * S, TY - 2 * S
    P = nx * ny
    tiles_x, tiles_y = -(-nx // INX), -(-ny // INY)
    nzc = -(-nz // zc)
    xout = np.full(nx * ny * nz, np.nan)
    rout = np.full(nx * ny * nz, np.nan)
    absent = np.full(7, ABSENT)
    NL = TX * TY
    ty, tx = np.divmod(np.arange(NL), TX)
    for bid in range(tiles_x * tiles_y * nzc):
        zb, rem = divmod(bid, tiles_x * tiles_y)
        tyi, txi = divmod(rem, tiles_x)
        gx = txi * INX - S + tx
        gy = tyi * INY - S + ty
        inxy = (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny)
        ring1 = inxy & (tx >= 1) & (tx < TX - 1) & (ty >= 1) & (ty < TY - 1)
        inner = inxy & (tx >= S) & (tx < TX - S) & (ty >= S) & (ty < TY - S)
        col = np.where(inxy, gy * nx + gx, 0)
        z0 = zb * zc
        z1 = min(z0 + zc, nz)
        w = np.zeros((S + 1, 3, NL))
        cq = np.full((S, NL, 7), ABSENT)
        bq = np.zeros((S, NL))
        xq = np.zeros(NL)
        k = z0 - S
        g_next = np.where(inxy & (k >= 0), g0[np.clip(k * P + col, 0, None)], 0.0)
        c_next = np.tile(absent, (NL, 1))
        b_next = np.zeros(NL)
        x_next = np.zeros(NL)
        for _ in range((z1 - z0) + 2 * S):
            w[0, 0], w[0, 1], w[0, 2] = w[0, 1].copy(), w[0, 2].copy(), g_next
            for s in range(S - 1, 0, -1):
                cq[s], bq[s] = cq[s - 1].copy(), bq[s - 1].copy()
            cq[0], bq[0], xq = c_next, b_next, x_next
            kn = k + 1
            ok = inxy & (kn >= 0) & (kn < nz)
            g_next = np.where(ok, g0[np.where(ok, kn * P + col, 0)], 0.0)
            rowk = ring1 & (k >= 0) & (k < nz)
            ik = np.where(rowk, k * P + col, 0)
            c_next = np.where(rowk[:, None], codes[ik], absent)
            b_next = np.where(rowk, b[ik], 0.0)
            if not first_res:
                x_next = np.where(rowk, x[ik], 0.0)
            for s in range(1, S + 1):
                plane = np.concatenate([np.zeros(TX), w[s - 1, 1], np.zeros(TX)])    # LDS with its padding
                q = TX + np.arange(NL)
                xv = [w[s - 1, 0], plane[q - TX], plane[q - 1], w[s - 1, 1], plane[q + 1], plane[q + TX], w[s - 1, 2]]
                if s == SP:
                    acc = row_sum(cq[s - 1], dictv, xv, c_gs)
                    val = (w[0, 0] if first_res else xq) + (c_last * w[s - 1, 1] + acc)
                else:
                    acc = row_sum(cq[s - 1], dictv, xv, 1.0)
                    val = bq[s - 1] - acc
                w[s, 0], w[s, 1], w[s, 2] = w[s, 1].copy(), w[s, 2].copy(), val
            p = k - S
            if z0 <= p < z1:
                i = p * P + col[inner]
                assert np.all(np.isnan(xout[i])), "a row written twice"
                if last_res:
                    rout[i] = w[S, 2][inner]
                xout[i] = w[SP, 2 - (S - SP)][inner]
            k += 1
    return xout, (rout if last_res else None)


@pytest.mark.parametrize("dims", [(7, 5, 3), (37, 29, 11), (61, 33, 9), (30, 27, 70)])
@pytest.mark.parametrize("chain", [(False, True), (True, True), (True, False)])
def test_tiled_chain_matches_separate_passes(dims, chain):
    first_res, last_res = chain
    rng = np.random.RandomState(sum(dims) + 7 * first_res + 3 * last_res)
    nx, ny, nz = dims
    n = nx * ny * nz
    dictv = rng.standard_normal(6)
    codes = box_codes(nx, ny, nz, len(dictv), rng)
    g0, x, b = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    if first_res:
        x = g0
    zc = min(64, nz) if nz != 70 else 32          # (a ragged last chunk)
    c_gs, c_last = 0.37, -1.21
    xr, rr = reference_chain(first_res, last_res, codes, dictv, dims, g0, x, b, c_gs, c_last)
    xt, rt = tiled_chain(first_res, last_res, codes, dictv, dims, g0, x, b, c_gs, c_last, zc)
    assert not np.any(np.isnan(xt)), "rows the chain never wrote"
    assert np.array_equal(xt, xr)
    if last_res:
        assert np.array_equal(rt, rr)
