"""Root-node energy smoothing on the device (csrc/energy.hip: amg_energy_smooth_rootnode_device, the identity kernel, the
initial fit) against the host route bit for bit, the flat entry truncate_rows_csr against the reference's recorded
calls and the sequential model of tests/rootnode_io.py, and one hierarchy built through the device route."""
import numpy as np
import pytest
import scipy.sparse as sps

import energy_io as eio
import evolution_io as evo
import golden_io
import rootnode_io as rio
from pyamg_amd import amg_core, smooth, util
from pyamg_amd.aggregation import fit_candidates, poisson, standard_aggregation, symmetric_strength_of_connection
from pyamg_amd.smooth import energy_prolongation_smoother

pytestmark = pytest.mark.gpu


def rootnode_inputs(A, B, AggOp, Cnodes):
    """the level's steps ahead of the smoother (rootnode.py): -> the scaled T, Cpt_params' dictionary, B_c"""
    bs = A.blocksize[0] if sps.isspmatrix_bsr(A) else 1
    T0, _ = fit_candidates(AggOp, B[:, :bs])
    par = util.get_Cpt_params(A, np.asarray(Cnodes), AggOp, T0)
    return util.scale_T(T0, par["P_I"], par["I_F"]), par, par["P_I"].T * B


def both_routes(A, T, Atilde, Bc, B, par, **opt):
    th, td = [], []
    H = energy_prolongation_smoother(A, T, Atilde, Bc, B, (True, par), device=False, _trace=th, **opt)
    D = energy_prolongation_smoother(A, T, Atilde, Bc, B, (True, par), device=True, _trace=td, **opt)
    eio.same_bits(D, H)
    assert td == th, "the two routes took other inner products: %r and %r" % (td, th)
    assert rio.rows_are_identity(D, par["Cpts"])
    return H, th


# ---------------------------------------------------------------------------------------------- device against host
@pytest.mark.parametrize("name,q", rio.all_sets())
def test_device_route_equals_host_route_bit_for_bit(name, q):
    p = rio.problem(name)
    s = p["sets"][q]
    if not s["fits"] and not smooth._scatter(sps.bsr_matrix(p["T"]), s["passes"][0][0], s["passes"][0][1])[1].all():
        # random_spd_150 with degree 1: the empty row of Atilde leaves a block of T outside the pattern and no initial fit
        # drops it
        assert (name, q) == ("random_spd_150", 1)
        with pytest.raises(NotImplementedError, match="outside the restated setup"):
            energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], (True, p["params"]), device=True, **s["options"])
        return
    H, trace = both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], p["params"], **s["options"])
    assert len(trace) == sum(len(t) for t in s["traces"])
    assert np.array_equal(H.indptr, s["P"].indptr) and np.array_equal(H.indices, s["P"].indices)


def test_fixtures_reach_the_initial_fit_at_both_block_shapes():
    shapes = set()
    for name, q in rio.all_sets():
        p = rio.problem(name)
        if p["sets"][q]["fits"]:
            shapes.add((p["A"].blocksize[0] if sps.isspmatrix_bsr(p["A"]) else 1, p["Bc"].shape[1]))
    assert {(2, 3), (3, 6), (1, 1)} <= shapes         # (1, 1): the second pass of a post-filter


def test_scalar_problem_with_two_candidates():
    A = poisson((12, 11), format="csr")
    n = A.shape[0]
    B = np.column_stack([np.ones(n), np.arange(n, dtype=np.float64) % 11])
    C = symmetric_strength_of_connection(A)
    AggOp, Cnodes = standard_aggregation(C)
    T, par, Bc = rootnode_inputs(A, B, AggOp, Cnodes)
    assert Bc.shape[1] == 2
    H, trace = both_routes(A, T, C, Bc, B, par, maxiter=4, degree=1)
    assert len(trace) == 4
    H, trace = both_routes(A, T, C, Bc, B, par, maxiter=3, degree=2, postfilter={"k": 4})
    assert len(trace) == 4


# ---------------------------------------------------------------------------------------------- the identity kernel
def chain(n_agg, per, bs=1):
    """a 1-D Laplacian (bs > 1: its Kronecker product with an SPD block) with n_agg aggregates of per consecutive nodes,
    the root in the middle: exact aggregate counts through a predefined aggregation"""
    n = n_agg * per
    A = poisson((n,), format="csr")
    if bs > 1:
        blk = np.eye(bs) * 2.0 + 0.25 * np.ones((bs, bs))
        A = sps.kron(A, blk).tobsr(blocksize=(bs, bs))
        A.sort_indices()
    AggOp = sps.csr_matrix((np.ones(n, dtype=np.int8), np.repeat(np.arange(n_agg), per), np.arange(n + 1)), shape=(n, n_agg))
    Cnodes = np.arange(n_agg) * per + per // 2
    B = np.kron(np.ones((n, 1)), np.eye(bs))
    return A, B, AggOp, Cnodes


@pytest.mark.parametrize("n_agg,per,bs", [(255, 3, 1), (256, 3, 1), (257, 3, 1), (29, 2, 3), (1, 5, 1)])
def test_identity_kernel_at_workgroup_boundaries(n_agg, per, bs):
    A, B, AggOp, Cnodes = chain(n_agg, per, bs)
    T, par, Bc = rootnode_inputs(A, B, AggOp, Cnodes)
    assert T.shape[1] == n_agg * bs and len(par["Cpts"]) * bs == n_agg * bs * bs
    H, trace = both_routes(A, T, None, Bc, B, par, maxiter=3, degree=1)
    assert len(trace) >= 1
    assert np.count_nonzero(H.data) > np.count_nonzero(T.data) or n_agg == 1


# ---------------------------------------------------------------------------------------------- iteration edge cases
def test_maxiter_zero_returns_the_fitted_prolongator():
    for name in ("aniso_17x23", "elasticity_12x12"):
        p = rio.problem(name)
        H, trace = both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], p["params"], maxiter=0)
        assert trace == []
    G = rio.problem("elasticity_12x12")["sets"][0]["fits"][0].copy(); G.eliminate_zeros()
    assert np.array_equal(H.indices, G.indices)
    p = rio.problem("aniso_17x23")
    T = sps.bsr_matrix(p["T"]); T.sort_indices()
    eio.same_bits(both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], p["params"], maxiter=0)[0], T)


def test_tolerance_break_at_iteration_two():
    p = rio.problem("aniso_17x23")
    ref = p["sets"][0]["traces"][0][:, 0]
    assert ref[2] < 0.5 < ref[1]
    H, trace = both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], p["params"], maxiter=6, degree=1, tol=0.5)
    assert len(trace) == 3 and trace[2][0] < 0.5 and trace[2][1] == 0.0


# ---------------------------------------------------------------------------------------------- argument checks
def captured_plan(monkeypatch):
    p = rio.problem("elasticity_12x12")
    seen = []
    real = smooth._cg_device

    def spy(plan, *a, **k):
        seen.append(plan)
        return real(plan, *a, **k)
    monkeypatch.setattr(smooth, "_cg_device", spy)
    energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], (True, p["params"]), device=True, maxiter=1)
    monkeypatch.setattr(smooth, "_cg_device", real)
    return seen[0]


def test_c_entry_refuses_bad_roots_before_any_launch(monkeypatch):
    plan = captured_plan(monkeypatch)
    assert plan.root_row is not None and plan.Bf is not None and plan.R == plan.Cc
    good_root, good_Sp, good_Sj, good_Tx = plan.root_row, plan.Sp, plan.Sj, plan.Tx
    # two columns share a root
    plan.root_row = good_root.copy(); plan.root_row[1] = plan.root_row[0]
    with pytest.raises(ValueError, match="share a root"):
        smooth._cg_device(plan, 1, 1e-8)
    # a root outside the matrix
    plan.root_row = good_root.copy(); plan.root_row[0] = plan.n_brow
    with pytest.raises(ValueError, match="outside the matrix"):
        smooth._cg_device(plan, 1, 1e-8)
    # a root's pattern row holds two blocks: the row of a non-root node is named as root
    plan.root_row = good_root.copy()
    two = int(np.nonzero(np.diff(good_Sp) >= 2)[0][0])
    assert two not in good_root
    plan.root_row[0] = two
    with pytest.raises(ValueError, match="exactly one block"):
        smooth._cg_device(plan, 1, 1e-8)
    # the one block of a root row is another column
    plan.root_row = good_root.copy()
    plan.Sj = good_Sj.copy(); plan.Sj[good_Sp[good_root[0]]] = (good_Sj[good_Sp[good_root[0]]] + 1) % plan.n_bcol
    with pytest.raises(ValueError, match="exactly one block"):
        smooth._cg_device(plan, 1, 1e-8)
    plan.Sj = good_Sj
    # R != Cc
    plan.Cc = plan.R + 1
    with pytest.raises(ValueError, match="square blocks"):
        smooth._cg_device(plan, 1, 1e-8)
    plan.Cc = plan.R
    Tx, its = smooth._cg_device(plan, 1, 1e-8)          # the untouched plan still runs
    assert its == 1 and Tx.shape == good_Tx.shape


# ---------------------------------------------------------------------------------------------- truncate_rows_csr
def device_truncate(n_row, k, Sp, Sj, Sx):
    j, x = np.ascontiguousarray(Sj).copy(), np.ascontiguousarray(Sx).copy()
    amg_core.truncate_rows_csr(n_row, k, np.ascontiguousarray(Sp), j, x)
    return j, x


def test_truncate_rows_reproduces_recorded_and_crafted_calls():
    cases = [(a["n_row"], a["k"], a["Sp"], a["Sj"], a["Sx"], o["Sj"], o["Sx"]) for a, o in rio.recorded_calls("truncate_rows_csr")]
    cases += [(len(Sp) - 1, k, Sp, Sj, Sx, wj, wx) for k, Sp, Sj, Sx, wj, wx in rio.crafted_truncations()]
    assert len(cases) >= 9
    for n_row, k, Sp, Sj, Sx, wj, wx in cases:
        j, x = device_truncate(n_row, k, Sp, Sj, Sx)
        assert np.array_equal(j, wj) and np.array_equal(x, wx), "k = %d" % k


@pytest.mark.parametrize("n_row", [255, 256, 257])
def test_truncate_rows_at_workgroup_boundaries(n_row):
    rng = np.random.RandomState(n_row)
    counts = rng.randint(0, 71, n_row)
    counts[-1] = 70                                     # the last lane has work
    Sp = np.concatenate([[0], np.cumsum(counts)]).astype(np.intc)
    Sj = np.concatenate([rng.permutation(80)[:c] for c in counts]).astype(np.intc)
    Sx = rng.randint(-4, 5, int(Sp[-1])).astype(np.float64)          # small integers: ties and zeros everywhere
    for k in (0, 1, 7, 70, 71):
        j, x = device_truncate(n_row, k, Sp, Sj, Sx)
        wj, wx = rio.model_truncate_rows_csr(n_row, k, Sp, Sj, Sx)
        assert np.array_equal(j, wj) and np.array_equal(x, wx), "k = %d" % k
        if k == 0:
            assert not x.any()
        if k >= 70:
            assert np.array_equal(j, Sj) and np.array_equal(x, Sx)


def test_truncate_rows_refusals():
    Sp = np.array([0, 2], dtype=np.intc); Sj = np.array([0, 1], dtype=np.intc)
    with pytest.raises(NotImplementedError):
        amg_core.truncate_rows_csr(1, 1, Sp, Sj, np.ones(2, dtype=np.float32))
    with pytest.raises(NotImplementedError):
        amg_core.truncate_rows_csr(1, 1, Sp, Sj, np.ones(2, dtype=np.complex128))
    with pytest.raises(NotImplementedError):
        amg_core.truncate_rows_csr(1, 1, Sp.astype(np.int64), Sj, np.ones(2))
    x = np.array([1.0, 2.0])
    with pytest.raises(ValueError):                     # Sx shorter than the last offset
        amg_core.truncate_rows_csr(1, 1, np.array([0, 3], dtype=np.intc), Sj, x)
    with pytest.raises(ValueError):
        amg_core.truncate_rows_csr(1, -1, Sp, Sj, x)
    assert np.array_equal(x, [1.0, 2.0])


# ---------------------------------------------------------------------------------------------- working size, solver
def test_device_route_at_working_size():
    """the 480 x 481 grid of tests/evolution_io.py (230 880 rows), root-node defaults: the identity kernel and every
    kernel of the iteration span many workgroups; the host route, pinned to the reference at small size, is the oracle"""
    A, _ = evo.large_grid()
    B = np.ones((A.shape[0], 1))
    C = symmetric_strength_of_connection(A)
    AggOp, Cnodes = standard_aggregation(C)
    T, par, Bc = rootnode_inputs(A, B, AggOp, Cnodes)
    H, trace = both_routes(A, T, C, Bc, B, par)
    assert len(trace) == 4 and H.shape[0] == 230880 and len(H.indices) > 256 * 256 and H.shape[1] > 256 * 64


def test_hierarchy_through_the_device_route():
    name = "rootnode_ev_d2_post"
    g, dev = rio.build_hierarchy(name, device=True)
    _, host = rio.build_hierarchy(name, device=False)
    sizes, cycles = rio.HIERARCHIES[name]
    assert [lvl.A.shape[0] for lvl in dev.levels] == sizes
    for a, b in zip(dev.levels, host.levels):
        if hasattr(b, "P"):
            eio.same_bits(a.P, b.P)
            assert rio.rows_are_identity(a.P, a.Cpts)
    res = []
    x = dev.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"], residuals=res)
    assert len(res) - 1 == len(g["residuals"]) - 1 == cycles
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], x, g["b"])
