"""The matrix-free tangent operator on the GPU (fenics_constitutive_amd.TangentOperator, csrc/jit/tangent_operator.hip): the
product, its fused ordered dot, the diagonal blocks and whole conjugate-gradient runs compared ON THE BITS with the NumPy oracle of
tangent_operator_util.py and with the routes the package already has -- ``tangent_action(op(.))`` in both gradient layouts,
``K.diagonal_blocks(K(tangent))`` --, every output between canaries; the statuses, the refusals, and the Newton loop of
examples/cube_tension_matrix_free_solve.py.  The product and the diagonal blocks run at every tiling the template generates
(tangent_operator_util.TILING_SHAPES: W one less than 64 // Q, tiles off the 16-byte grid, dead lanes, A >= 64 with one, two and three
passes over the nodes, every slab size), the grid-stride loops of both element kernels under the cap of one compute unit."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402
from cube_tension_matrix_free_solve import MatrixFreeSolveLoop  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import force as force_module  # noqa: E402
from fenics_constitutive_amd import gradient, jit, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result, tables_of  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, cell_counts  # noqa: E402
from gradient_util import cube_operator_tables  # noqa: E402
from solver_util import SEG, conjugate_gradient, ordered_dot, spd_tangent  # noqa: E402
from tangent_operator_util import (NO_MATRIX, TILING_SHAPES, diagonal_blocks_oracle, distinct_inputs, operator_solve, product_oracle,  # noqa: E402
                                   random_mask, tiling_constants)

TO_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
SHAPES = TILING_SHAPES  # every tiling the template generates (tangent_operator_util.py; test_tangent_operator.py: each branch is reached)
PRODUCT_SHAPES = tuple(name for name in TILING_SHAPES if name != "wide130")
SOLVE_SHAPES = TO_SHAPES + ("q3", "odd33_3d", "wide70")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


def operators(t, layout="nabla_grad"):
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"], layout=layout)
    return op, fc.InternalForce(op, t["weights"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the product
# ---------------------------------------------------------------------------------------------------------------------------------
def check_product(a, t, tangent, v, mask, what, pairs=()):
    """A(tangent, v) between canaries against the oracle and against every (op, force) of ``pairs``; returns the host result"""
    n = a.shape[0]
    a.set_constrained(mask)
    tangent_dev, v_dev = to_device(tangent, "cuda"), to_device(v, "cuda")
    buf, out = guarded(n)
    got = a(tangent_dev, v_dev, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    have = to_host(out)
    assert_same_bits(have, product_oracle(tangent, v, *tables_of(t), mask=mask), f"{what}: oracle")
    assert_same_bits(to_host(v_dev), v, f"{what}: v was written")
    for op, force in pairs:
        vm = v_dev if mask is None else torch.where(to_device(mask, "cuda"), torch.zeros((), dtype=torch.float64, device="cuda"), v_dev)
        y = force.tangent_action(tangent_dev, op(vm))
        if mask is not None:
            y = torch.where(to_device(mask, "cuda"), v_dev, y)
        assert_same_bits(have, to_host(y), f"{what}: tangent_action(op(.)) in layout {op.layout}")
    return have


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", PRODUCT_SHAPES)
def test_product_on_the_bits(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    w = force_module.cells_per_tile(d_, q_)
    assert w == tiling_constants(d_, a_, q_, affine).W
    for n_cells in cell_counts(w, q_):
        integer = n_cells % 2 == 0
        t = distinct_inputs(shape, n_cells, 7 + n_cells, integer, affine)
        pairs = [operators(t, layout) for layout in gradient.LAYOUTS]
        a = fc.TangentOperator(pairs[0][1])
        assert fc.TangentOperator(pairs[1][1])._code is a._code  # the layout is not part of the program
        rng = np.random.default_rng(n_cells)
        v = rng.integers(-8, 9, size=a.shape[0]).astype(np.float64) if integer else rng.normal(size=a.shape[0])
        for mask in (None, random_mask(t, d_, n_cells, whole_cell=n_cells // 2)):
            what = f"{shape} affine={affine} cells={n_cells} integer={integer} mask={'yes' if mask is not None else 'no'}"
            have = check_product(a, t, t["tangent"], v, mask, what, pairs)
            assert (bits(have.reshape(-1, d_)[t["lonely"]]) == 0).all(), what  # the node in no cell: +0.0
            if mask is not None:
                assert mask.any() and np.array_equal(bits(have[mask]), bits(v[mask])), what
                used = np.repeat(np.bincount(t["dofmap"].reshape(-1), minlength=t["n_nodes"]) > 0, d_)
                assert (used & ~mask).any() == (n_cells > 1) or w == 1, what  # (one cell: all of its dofs are constrained)
                assert np.abs(have[~mask]).max() > 0 or not (used & ~mask).any(), what
    assert a(to_device(t["tangent"], "cuda"), to_device(v, "cuda")).shape == (a.shape[0],)  # without out: a new tensor


def test_product_of_a_mesh_without_cells():
    t = distinct_inputs("hex8", 1, 2, False, False)
    op = fc.DisplacementGradient(t["dofmap"][:0], t["ref"], t["jinv"][:0], 300)
    a = fc.TangentOperator(fc.InternalForce(op, t["weights"][:0]))
    buf, out = guarded(900)
    a(torch.zeros(0, dtype=torch.float64, device="cuda"), to_device(np.arange(1.0, 901.0), "cuda"), out=out)
    blocks = a.diagonal_blocks(torch.zeros(0, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    assert_margins_intact(buf, 900)
    assert (bits(to_host(out)) == 0).all() and (bits(to_host(blocks)) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the fused dot
# ---------------------------------------------------------------------------------------------------------------------------------
def interval_mesh(n_nodes):
    """a chain of two-node cells over n_nodes nodes (D = 1: the dofs are the nodes), lengths and tangent random"""
    rng = np.random.default_rng(n_nodes)
    dofmap = np.stack([np.arange(n_nodes - 1), np.arange(1, n_nodes)], axis=1).astype(np.int32)
    h = rng.uniform(0.5, 1.5, size=n_nodes - 1)
    return dict(dofmap=dofmap, ref=np.array([[[-1.0], [1.0]]]), jinv=np.ascontiguousarray((1.0 / h)[:, None, None]), weights=h[:, None].copy(),
                n_nodes=n_nodes, tangent=rng.uniform(1.0, 2.0, size=n_nodes - 1))


def plain_dot(a, tangent, p, what):
    """solver.matvec in _MODE_PLAIN: (the product, the dot it left in the control block)"""
    n = a.shape[0]
    buf, out = guarded(n)
    solver.matvec(a, to_device(tangent, "cuda"), to_device(p, "cuda"), out=out)
    control = solver._operator(a)._control[a.device]
    control.download(a.device, solver._SCALARS)
    assert_margins_intact(buf, n)
    assert int(control.ints[solver._STATUS]) == 0 and int(control.ints[solver._COUNTER]) == 0, what
    return to_host(out), float(control.host[solver._DOT])


def check_dots(sizes):
    for n_nodes in sizes:
        t = interval_mesh(n_nodes)
        a = fc.TangentOperator(operators(t)[1])
        mask = np.zeros(n_nodes, dtype=bool)
        mask[[0, n_nodes // 3]] = True
        a.set_constrained(mask)
        p = np.random.default_rng(1).normal(size=n_nodes)
        for repeat in range(2):  # (the counter is left at zero: the second run finds its last block too)
            y, have = plain_dot(a, t["tangent"], p, f"interval {n_nodes}")
            assert_same_bits(y, product_oracle(t["tangent"], p, *tables_of(t), mask=mask), f"interval {n_nodes}")
            want = ordered_dot(p, y)
            assert bits(np.float64(have)) == bits(np.float64(want)), (n_nodes, have, want)


def test_dot_on_the_bits():
    check_dots((1 + 1, 257, SEG - 1, SEG, SEG + 1, 2 * SEG + 5))
    # D = 3: a 10 x 10 x 9 cube has 3630 dofs, two segments; cubes of 3069, 3072 and 3075 dofs: the nearest to SEG a node count allows
    for cells in ((10, 10, 9), (2, 10, 30), (7, 7, 15), (4, 4, 40)):
        mesh = FE.Cube(*cells)
        op, f = cube_operators(mesh)
        dofmap, ref, jinv = cube_operator_tables(mesh)
        a = fc.TangentOperator(f)
        mask, _ = tension_constraints(mesh)
        a.set_constrained(mask)
        tangent = spd_tangent(mesh.n_points, 6, 1, False)
        p = np.random.default_rng(2).normal(size=mesh.n_dofs)
        y, have = plain_dot(a, tangent, p, f"cube {cells}")
        assert_same_bits(y, product_oracle(tangent, p, dofmap, ref, jinv, f._weights, mesh.n_nodes, mask=mask), f"cube {cells}")
        assert bits(np.float64(have)) == bits(np.float64(ordered_dot(p, y))), cells
    assert mesh.n_dofs == SEG + 3


def test_dot_on_one_compute_unit(one_cu):
    n_nodes = 17 * SEG + 5  # 18 segments: more than the 16 blocks one compute unit is capped at
    check_dots((n_nodes,))
    assert {(name, nb) for name, nb in one_cu} == {(to.ELEMENT_KERNEL, gradient.BLOCKS_PER_CU), (to.NODE_KERNEL, gradient.BLOCKS_PER_CU)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the diagonal blocks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", tuple(TILING_SHAPES))
def test_diagonal_blocks_on_the_bits(shape, affine):
    d_, a_, q_, _ = SHAPES[shape]
    cw = to.diagonal_cells_per_tile(a_)
    assert cw == tiling_constants(d_, a_, q_, affine).CW
    n_cells = 3 * cw + 1
    t = distinct_inputs(shape, n_cells, 13, False, affine)
    op, f = operators(t)
    tangent = to_device(t["tangent"], "cuda")
    tile = cw * a_ * d_ * d_ * 8
    for mask in (None, random_mask(t, d_, 4, whole_cell=1)):
        want = diagonal_blocks_oracle(t["tangent"], *tables_of(t), mask=mask)
        if shape in NO_MATRIX:  # no assembled matrix to stand between: the oracle alone (test_tangent_operator.py ties it to the dense K)
            with pytest.raises(ValueError, match="does not compile without scratch"):
                fc.TangentMatrix(f)
        else:
            k = fc.TangentMatrix(f)
            k.set_constrained(mask)
            have = to_host(k.diagonal_blocks(k(tangent)))
            assert_same_bits(have, want, f"{shape}: the oracle and the matrix")
            want = have
        for scratch in (tile, 2 * tile + 8, None):  # one tile of cells, two, everything
            a = fc.TangentOperator(f, scratch_bytes=scratch)
            a.set_constrained(mask)
            assert len(a.chunks()) == {tile: 4, 2 * tile + 8: 2, None: 1}[scratch]
            buf, out = guarded(d_ * d_ * t["n_nodes"])
            a.diagonal_blocks(tangent, out=out)
            torch.cuda.synchronize()
            assert_margins_intact(buf, d_ * d_ * t["n_nodes"])
            assert_same_bits(to_host(out), want, f"{shape} affine={affine} cells={n_cells} scratch={scratch} mask={'yes' if mask is not None else 'no'}")
        assert a.diagonal_blocks(tangent).shape == (t["n_nodes"], d_, d_)
    assert (bits(want.reshape(-1, d_, d_)[t["lonely"]]) == 0).all() and np.abs(want).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. the grid-stride loops under the cap of one compute unit: more than two trips, the ragged tile last
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_cells", [("q3", 129 * 20 + 7), ("odd33_3d", 130)])
def test_product_on_one_compute_unit(shape, n_cells, one_cu):
    d_, a_, q_, affine = SHAPES[shape]
    k = tiling_constants(d_, a_, q_, affine)
    tiles = -(-n_cells // k.W)
    assert tiles > 2 * gradient.BLOCKS_PER_CU * 4 and (n_cells % k.W != 0) == (k.W > 1)  # (four waves, a tile each, per block)
    t = distinct_inputs(shape, n_cells, 31, False, affine)
    a = fc.TangentOperator(operators(t)[1])
    v = np.random.default_rng(n_cells).normal(size=a.shape[0])
    for mask in (None, random_mask(t, d_, 6, whole_cell=n_cells - 1)):
        del one_cu[:]
        check_product(a, t, t["tangent"], v, mask, f"{shape} affine={affine} cells={n_cells} on one compute unit mask={'yes' if mask is not None else 'no'}")
        assert (to.ELEMENT_KERNEL, gradient.BLOCKS_PER_CU) in one_cu  # the launch really was capped


def test_diagonal_blocks_on_one_compute_unit(one_cu):
    shape, n_cells = "wide70", 129
    d_, a_, q_, affine = SHAPES[shape]
    k = tiling_constants(d_, a_, q_, affine)
    assert k.kPasses == 2 and -(-n_cells // k.CW) > 2 * gradient.BLOCKS_PER_CU * 4
    t = distinct_inputs(shape, n_cells, 33, False, affine)
    a = fc.TangentOperator(operators(t)[1])
    tangent = to_device(t["tangent"], "cuda")
    for mask in (None, random_mask(t, d_, 8, whole_cell=n_cells - 1)):
        a.set_constrained(mask)
        assert len(a.chunks()) == 1
        del one_cu[:]
        buf, out = guarded(d_ * d_ * t["n_nodes"])
        a.diagonal_blocks(tangent, out=out)
        torch.cuda.synchronize()
        assert_margins_intact(buf, d_ * d_ * t["n_nodes"])
        assert_same_bits(to_host(out), diagonal_blocks_oracle(t["tangent"], *tables_of(t), mask=mask),
                         f"{shape} cells={n_cells} on one compute unit mask={'yes' if mask is not None else 'no'}")
        assert (to.DIAGONAL_ELEMENT_KERNEL, gradient.BLOCKS_PER_CU) in one_cu and (to.DIAGONAL_NODE_KERNEL, gradient.BLOCKS_PER_CU) in one_cu


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. solves
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SOLVE_SHAPES)
def test_exactly_k_iterations(shape):
    d_, a_, q_, affine = SHAPES[shape]
    n_cells = -(-257 // q_)
    if shape == "wide70":  # the fewest cells with two tiles of the product (W = 32) and two of the diagonal blocks (CW = 1)
        n_cells = force_module.cells_per_tile(d_, q_) + 1
    t = distinct_inputs(shape, n_cells, 21, False, affine, every_node=True)
    a = fc.TangentOperator(operators(t)[1])
    mask = random_mask(t, d_, 26)
    a.set_constrained(mask)
    tangent = spd_tangent(n_cells * q_, MANDEL_DIM[d_], 21, False)
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=a.shape[0]))
    start = rng.normal(size=a.shape[0])
    for pc in ("block_jacobi", None):
        for its in (1, 2, 7):
            cg = fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{shape} {pc} k={its} x0={'yes' if x0 is not None else 'no'}"
                want = operator_solve(tangent, b, *tables_of(t), mask=mask, x0=x0, preconditioner=pc, rtol=0.0, maxiter=its)
                res, x = solve_guarded(cg, tangent, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, x, want, what)
        x0_dev = to_device(start, "cuda")
        res = cg(to_device(tangent, "cuda"), to_device(b, "cuda"), x0=x0_dev)  # without out: a new tensor, x0 untouched
        assert res.x.data_ptr() != x0_dev.data_ptr() and np.array_equal(to_host(x0_dev), start)
        assert_same_bits(to_host(res.x), want.x, f"{shape} {pc}: without out")


@pytest.fixture(scope="module")
def cube_system():
    """the tension-test system of a 10 x 10 x 9 cube (3630 dofs: two segments) on a random positive definite tangent, its right-hand
    side and the oracle's solves"""
    mesh = FE.Cube(10, 10, 9)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, f._weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    tangent = spd_tangent(mesh.n_points, 6, 1, False)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    a = fc.TangentOperator(f)
    a.set_constrained(mask)
    oracle = {(pc, kw): operator_solve(tangent, b, *tables, mask=mask, preconditioner=pc, **dict(kw))
              for pc in ("block_jacobi", None) for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))}
    return mesh, f, tables, mask, tangent, b, a, oracle


@pytest.mark.parametrize("pc", ["block_jacobi", None])
def test_check_every_changes_nothing(pc, cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),)):
        want = oracle[(pc, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16)
            res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, check_every=every, **dict(kw)), tangent, b)
            assert_same_result(res, x, want, f"{pc} {dict(kw)} check_every={every}")
            assert res.looks == 1 + -(-want.iterations // every)
    assert oracle[("block_jacobi", kw)].iterations < oracle[(None, kw)].iterations


def test_statuses(cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    for pc in ("block_jacobi", None):
        cg = fc.ConjugateGradient(a, preconditioner=pc, rtol=1e-6)
        # a negated tangent: indefinite at the first product, x is x0 on the bits
        res, x = solve_guarded(cg, -tangent, b, start)
        assert (res.status, res.iterations, res.converged) == ("indefinite", 0, False)
        assert_same_bits(x, start, f"{pc}: indefinite")
        assert_same_result(res, x, operator_solve(-tangent, b, *tables, mask=mask, x0=start, preconditioner=pc, rtol=1e-6), f"{pc}: indefinite")
        # b = 0: converged at once
        res, x = solve_guarded(cg, tangent, np.zeros(n))
        assert (res.status, res.iterations, res.converged, res.residual_norm, res.rhs_norm, res.looks) == ("converged", 0, True, 0.0, 0.0, 1)
        assert (bits(x) == 0).all()
        res, x = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, maxiter=0), tangent, b, start)
        assert (res.status, res.iterations, res.looks) == ("maxiter", 0, 1)
        assert_same_bits(x, start, f"{pc}: maxiter 0")
    # an all-zero tangent: every free node's own block is zero -- no iteration, x is x0
    res, x = solve_guarded(fc.ConjugateGradient(a), np.zeros_like(tangent), b, start)
    assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
    assert_same_bits(x, start, "singular block")
    bad = b.copy()
    bad[17] = np.nan
    res, x = solve_guarded(fc.ConjugateGradient(a), tangent, bad)
    assert res.status == "nonfinite" and res.iterations == 0


def test_the_matrix_solver_keeps_its_bits_next_to_the_operator(cube_system):
    """a ConjugateGradient(K) in the process that has run the operator's solves still gives its own oracle's bits -- which differ from
    the operator's: the two products round differently"""
    from solver_util import from_format

    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    tangent_dev = to_device(tangent, "cuda")
    for pc in ("block_jacobi", None):
        free, _ = solve_guarded(fc.ConjugateGradient(a, preconditioner=pc, rtol=0.0, maxiter=7), tangent, b)
        for fmt in ("bsr", "csr"):
            k = fc.TangentMatrix(f, format=fmt)
            k.set_constrained(mask)
            values = k(tangent_dev)
            n = b.size
            buf, out = guarded(n)
            res = fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=7)(values, to_device(b, "cuda"), out=out)
            assert_margins_intact(buf, n)
            blocks = from_format(fmt, k.indptr, k.indices, to_host(values), 3)
            want = conjugate_gradient(k.indptr, k.indices, blocks, b, preconditioner=pc, rtol=0.0, maxiter=7)
            assert_same_result(res, to_host(out), want, f"ConjugateGradient(K) {fmt} {pc}")
            assert np.allclose(to_host(out), to_host(free.x), rtol=1e-9, atol=1e-12 * np.abs(want.x).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(cube_system):
    mesh, f, tables, mask, tangent, b, a, oracle = cube_system
    n, nt = a.shape[0], tangent.size
    cg = fc.ConjugateGradient(a)
    tangent_dev, b_dev = to_device(tangent, "cuda"), to_device(b, "cuda")
    assert cg(tangent_dev, b_dev).converged  # tables uploaded, kernels loaded: what follows can only add launches
    buf, out = guarded(n)
    spare = torch.zeros(2 * max(n, nt) + 2, dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        for call in (lambda **kw: a(kw["tangent"], kw["v"], out=kw["out"]), lambda **kw: solver.matvec(a, kw["tangent"], kw["v"], out=kw["out"]),
                     lambda **kw: cg(kw["tangent"], kw["v"], out=kw["out"])):
            ok = dict(tangent=tangent_dev, v=b_dev, out=out)
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "out": buf[MARGIN + 1: MARGIN + 1 + n]})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "out": buf[MARGIN: MARGIN + n - 3]})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{**ok, "out": spare[: 2 * n: 2]})
            with pytest.raises(ValueError, match="cuda"):
                call(**{**ok, "out": torch.empty(n, dtype=torch.float64)})
            with pytest.raises(TypeError):
                call(**{**ok, "out": out.float()})
            with pytest.raises(ValueError, match="alias"):
                call(**{**ok, "out": b_dev})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "tangent": tangent_dev[:-36]})
            with pytest.raises(ValueError, match="aligned"):
                call(**{**ok, "tangent": spare[1: 1 + nt]})
            with pytest.raises(ValueError, match="entries"):
                call(**{**ok, "v": b_dev[:-3]})
            with pytest.raises(ValueError, match="contiguous"):
                call(**{**ok, "v": spare[: 2 * n: 2]})
            with pytest.raises(TypeError):
                call(**{**ok, "v": b})
        with pytest.raises(ValueError, match="entries"):
            a.diagonal_blocks(tangent_dev, out=out)
        with pytest.raises(ValueError, match="entries"):
            a.diagonal_blocks(tangent_dev[:-36])
        with pytest.raises(ValueError, match="x0 itself"):
            cg(tangent_dev, b_dev, x0=spare[2: 2 + n], out=spare[:n])
        with pytest.raises(ValueError, match="multilevel"):
            fc.ConjugateGradient(a, preconditioner="multilevel")
        with pytest.raises(ValueError, match="multilevel"):
            fc.ConjugateGradient(a, preconditioner=fc.MultilevelPreconditioner(fc.TangentMatrix(f)))
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert launches == []
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loop without a matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def test_in_the_loop_behind_a_resident_state():
    """The example's loop on Cube(3, 2, 4), eight load steps, ConjugateGradient(TangentOperator, rtol=1e-12): the Newton counts are
    those of the direct solve on the host, the reactions within 1e-8 of its (relative to the largest)."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    n = mesh.n_points
    cpu = FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), n)
    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu, steps=8)
    op, f = cube_operators(mesh)
    a = fc.TangentOperator(f)
    loop = MatrixFreeSolveLoop(ResidentState(fc.VonMises3D(VM_P), n, placement="torch"), op, f, a, fc.ConjugateGradient(a, rtol=1e-12))
    r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
    difference = np.max(np.abs(r_gpu - r_direct)) / np.max(np.abs(r_direct))
    counts = [len(h) for h in norms_gpu]
    print(f"matrix-free device solve: GPU against direct {difference:.3e}, Newton iterations {counts}, conjugate-gradient iterations {solves}")
    assert counts == [len(h) for h in norms_direct] == [2, 2, 2, 3, 3, 4, 5, 5]
    assert loop.solves == len(solves) == sum(counts) - 8
    assert difference <= 1e-8
    assert not any(isinstance(x, fc.TangentMatrix) for x in vars(loop).values())  # no matrix anywhere in the loop
