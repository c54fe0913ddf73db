"""The matrix-free tangent operator without a GPU (fenics_constitutive_amd.tangent_operator, csrc/jit/tangent_operator.hip): every
program compiles for gfx950 without scratch and with the LDS the module states, the host-side validation comes before any launch,
the oracle (tangent_operator_util.py) against the oracle of the assembled matrix -- the product within a rounding bound, the
diagonal blocks on the bits for every chunking --, and the oracle conjugate gradients on the oracle operator in the Newton loop of
examples/cube_tension_matrix_free_solve.py against the direct solver.  The tilings: the compile-time constants of the kernel's header
comment restated (tangent_operator_util.tiling_constants) against the module's, TILING_SHAPES reaching every branch they choose, and
at every such shape the oracle against a dense stiffness in np.longdouble -- what the GPU tests lean on where no TangentMatrix exists."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import gradient, jit, matrix, solver
from fenics_constitutive_amd import tangent_operator as to
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_test_device_solve  # noqa: E402
from fenics_constitutive_amd import force as force_module  # noqa: E402
from fe_gpu_util import bits  # noqa: E402
from force_util import chain_length, max_valence, random_inputs  # noqa: E402
from gradient_util import EPS, SHAPES, cube_operator_tables  # noqa: E402
from matrix_util import diagonal_blocks, matrix_oracle, to_bsr  # noqa: E402
from tangent_operator_util import (NO_MATRIX, TILING_SHAPES, dense_diagonal_blocks, dense_stiffness, diagonal_blocks_oracle,  # noqa: E402
                                   distinct_inputs, oracle_free_loop, product_chain_length, product_oracle, random_mask, tiling_constants)

VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
ORACLE_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")


def operator(shape="tet_p2", n_cells=5, seed=3, every_node=False, **kwargs):
    t = distinct_inputs(shape, n_cells, seed, False, True, every_node=every_node)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    return fc.TangentOperator(f, **kwargs), t


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. compilation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "per_point"])
@pytest.mark.parametrize("shape", sorted(TILING_SHAPES))
def test_every_program_compiles_without_scratch(shape, affine):
    d_, a_, q_, _ = TILING_SHAPES[shape]
    code = to.compile_kernels(d_, a_, q_, affine)
    lds = to.lds_bytes(d_, a_, q_)
    assert lds == gradient.lds_bytes(d_, a_, q_) <= gradient.LDS_CAP
    for kernel in to.KERNELS:
        r = kernel_resources(code.log, kernel)
        assert r["scratch_bytes"] == 0, (kernel, r)
    for kernel in (to.ELEMENT_KERNEL, to.DIAGONAL_ELEMENT_KERNEL):
        assert kernel_resources(code.log, kernel)["lds_bytes"] == lds, kernel
    assert kernel_resources(code.log, to.NODE_KERNEL)["lds_bytes"] == solver.lds_bytes(solver.DOT_KERNEL)  # the tree and the flag
    assert kernel_resources(code.log, to.DIAGONAL_NODE_KERNEL)["lds_bytes"] == 0
    r = kernel_resources(code.log, to.ELEMENT_KERNEL)
    assert code.waves in gradient.WAVES_LADDER and r["vgprs"] + (r["agprs"] or 0) <= 512 // code.waves
    assert code.slab == to.diagonal_slab(d_, a_, affine) >= 1
    k = tiling_constants(d_, a_, q_, affine)  # the header comment's constants against what the host sizes its launches with
    assert (k.W, k.CW, k.diagonal_slab) == (force_module.cells_per_tile(d_, q_), to.diagonal_cells_per_tile(a_), code.slab), (shape, k)
    before = jit.compile_count()
    assert to.compile_kernels(d_, a_, q_, affine) is code and jit.compile_count() == before  # once per program text


# ---------------------------------------------------------------------------------------------------------------------------------
# 1b. the tilings: the constants of the header comment, and that the shape list reaches every branch they choose
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tiling_constants_are_the_modules():
    for d_ in (1, 2, 3):
        for q_ in range(1, 65):
            k = tiling_constants(d_, 4, q_, True)
            assert k.W == force_module.cells_per_tile(d_, q_) and k.kPts == k.W * q_ <= 64, (d_, q_)
            assert k.kEven == ((k.kPts * d_ * d_) % 2 == 0) and (k.kEven or (k.W == 1 and q_ % 2 and d_ % 2)), (d_, q_)
            assert k.product_slab == {1: 64, 2: 16, 3: 8}[d_]
        for a_ in range(1, 150):
            for affine in (True, False):
                k = tiling_constants(d_, a_, 2, affine)
                assert k.CW == to.diagonal_cells_per_tile(a_) and k.CW * min(a_, 64) <= 64 and k.kPasses == -(-a_ // 64), (d_, a_)
                assert (k.CW == 1) == (a_ > 32) and (k.kPasses > 1) == (a_ > 64)
                try:
                    slab = to.diagonal_slab(d_, a_, affine)
                except ValueError:
                    slab = 0  # not one point fits: refused
                assert k.diagonal_slab == slab <= to.MAX_SLAB, (d_, a_, affine)


def test_the_shapes_reach_every_branch_of_the_template():
    """every compile-time branch of csrc/jit/tangent_operator.hip is taken by at least one shape of TILING_SHAPES (the GPU tests run
    them all): the list cannot shrink to the comfortable tilings without this failing"""
    rows = {name: (shape, tiling_constants(*shape[:3], True), tiling_constants(*shape[:3], False)) for name, shape in TILING_SHAPES.items()}

    def some(predicate):
        return sorted(name for name, ((d_, a_, q_, _), k, kp) in rows.items() if predicate(d_, a_, q_, k, kp))

    assert set(SHAPES) <= set(TILING_SHAPES) and all(TILING_SHAPES[name] == SHAPES[name] for name in SHAPES)
    assert some(lambda d_, a_, q_, k, kp: k.W == 64 // q_ - 1), "no shape with W one less than 64 // Q"
    assert some(lambda d_, a_, q_, k, kp: k.W == 64 // q_ - 1 and d_ == 1) and some(lambda d_, a_, q_, k, kp: k.W == 64 // q_ - 1 and d_ == 3)
    assert some(lambda d_, a_, q_, k, kp: not k.kEven and d_ == 1), "no shape off the 16-byte grid with D = 1"
    assert some(lambda d_, a_, q_, k, kp: not k.kEven and d_ == 3), "no shape off the 16-byte grid with D = 3"
    assert some(lambda d_, a_, q_, k, kp: k.W > 1 and k.kPts < 64), "no whole product tile with dead lanes"
    assert some(lambda d_, a_, q_, k, kp: k.W == 64 and q_ == 1 and d_ == 3)
    assert some(lambda d_, a_, q_, k, kp: a_ < 64 and k.CW * a_ < 64 and k.CW > 1), "no diagonal tile with dead lanes"
    assert some(lambda d_, a_, q_, k, kp: a_ == 64 and k.CW == 1 and k.kPasses == 1), "A == 64"
    assert some(lambda d_, a_, q_, k, kp: k.kPasses == 2 and a_ % 64), "no second, ragged pass"
    assert some(lambda d_, a_, q_, k, kp: k.kPasses == 3), "no third pass"
    assert some(lambda d_, a_, q_, k, kp: k.diagonal_slab == 1), "no diagonal slab of one point"
    assert some(lambda d_, a_, q_, k, kp: k.diagonal_slab == 2)
    assert some(lambda d_, a_, q_, k, kp: k.diagonal_slab % 2 == 1 and k.diagonal_slab > 1 and q_ > 1), "no odd diagonal slab"
    assert some(lambda d_, a_, q_, k, kp: kp.diagonal_slab % 2 == 1 and kp.diagonal_slab > 1 and kp.diagonal_slab != k.diagonal_slab)
    assert some(lambda d_, a_, q_, k, kp: k.diagonal_slab == to.MAX_SLAB), "no slab at the cap"
    assert some(lambda d_, a_, q_, k, kp: q_ > k.diagonal_slab), "no cell whose points straddle two slabs"
    assert some(lambda d_, a_, q_, k, kp: q_ > k.product_slab), "no cell longer than a slab of the product"
    # what each added shape is in the list for, constant by constant
    want = {"q3": dict(W=20, diagonal_slab=11), "q3_1d": dict(W=20), "q5": dict(W=12, kPts=60), "tet_p1": dict(W=64), "q7_2d": dict(W=9, kPts=63, CW=21),
            "odd33_1d": dict(W=1, kEven=False), "odd33_3d": dict(W=1, kEven=False), "wide": dict(CW=2, diagonal_slab=5),
            "wide64": dict(CW=1, kPasses=1, diagonal_slab=2), "wide70": dict(CW=1, kPasses=2), "wide130": dict(CW=1, kPasses=3, diagonal_slab=1)}
    for name, constants in want.items():
        assert {key: getattr(rows[name][1], key) for key in constants} == constants, name
    assert rows["q3"][2].diagonal_slab == 9
    # the register budgets: wide64 is the shape the ladder takes down to two waves
    budgets = {name: to.compile_kernels(*shape[:3], shape[3]).waves for name, shape in TILING_SHAPES.items() if name in ("hex8", "wide64")}
    assert budgets["wide64"] == 2 and budgets["hex8"] > 2, budgets


def test_shapes_that_do_not_fit_are_refused_before_the_compiler():
    before = jit.compile_count()
    with pytest.raises(ValueError, match="at most 64"):
        to.compile_kernels(3, 4, 65, True)
    with pytest.raises(ValueError, match="LDS"):
        to.compile_kernels(3, 400, 8, True)
    with pytest.raises(ValueError, match="LDS"):
        to.compile_kernels(3, 190, 1, True)  # the table fits, a point's basis gradients do not fit the wave's region
    with pytest.raises(ValueError, match="dimension"):
        to.compile_kernels(4, 4, 1, True)
    assert jit.compile_count() == before


def test_object_reports_what_the_compiler_made():
    a, t = operator()
    r = a.resources
    assert r["scratch_bytes"] == 0 and r["lds_bytes"] == a.lds_bytes() == to.lds_bytes(3, 10, 4)
    assert all(r[name]["scratch_bytes"] == 0 for name in ("node", "diagonal_element", "diagonal_node"))
    assert r["waves"] in gradient.WAVES_LADDER and r["slab"] == to.diagonal_slab(3, 10, True)
    assert all(kernel in a.compile_log for kernel in to.KERNELS)
    assert a.shape == (3 * t["n_nodes"],) * 2 and (a.gdim, a.n_nodes, a.n_points) == (3, t["n_nodes"], 5 * 4)
    assert a.device == a.force.device and a.scratch_bytes == matrix.SCRATCH_BYTES
    assert "TangentOperator" in fc.__all__ and fc.TangentOperator is to.TangentOperator
    assert (to.MODE_ITERATE, to.MODE_PLAIN) == (solver._MODE_ITERATE, solver._MODE_PLAIN) and to.SEG == solver.SEG


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. validation comes before any upload or launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    torch = pytest.importorskip("torch")
    a, t = operator()
    full, _ = operator(every_node=True)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        TO = fc.TangentOperator
        with pytest.raises(TypeError, match="InternalForce"):
            TO(a.op)
        with pytest.raises(TypeError, match="scratch_bytes"):
            TO(a.force, scratch_bytes=1e6)
        with pytest.raises(ValueError, match="scratch_bytes"):
            TO(a.force, scratch_bytes=8)
        twice = t["dofmap"].copy()
        twice[3, 7] = twice[3, 2]
        f2 = fc.InternalForce(fc.DisplacementGradient(twice, t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
        with pytest.raises(ValueError, match="cell 3 names a node twice"):
            TO(f2)
        # the mask: TangentMatrix's rules
        n = a.shape[0]
        with pytest.raises(TypeError, match="ndarray"):
            a.set_constrained([True] * n)
        with pytest.raises(TypeError, match="bool"):
            a.set_constrained(np.zeros(n, dtype=np.uint8))
        with pytest.raises(ValueError, match="shape"):
            a.set_constrained(np.zeros(n + 1, dtype=bool))
        lonely = np.zeros(n, dtype=bool)
        lonely[3 * t["lonely"] + 1] = True
        with pytest.raises(ValueError, match=f"node {t['lonely']} "):
            a.set_constrained(lonely)
        a.set_constrained(random_mask(t, 3, 1))
        a.set_constrained(None)
        # the tensors
        host = lambda m: torch.zeros(m, dtype=torch.float64)  # noqa: E731
        nt = 36 * a.n_points
        for call in (lambda x, y: a(x, y), lambda x, y: a.diagonal_blocks(x), lambda x, y: solver.matvec(a, x, y)):
            with pytest.raises(TypeError):
                call(np.zeros(nt), host(n))  # an ndarray
            with pytest.raises(TypeError):
                call(host(nt).float(), host(n))
            with pytest.raises(ValueError, match="cuda"):
                call(host(nt), host(n))  # on the host
        # the solver
        CG = fc.ConjugateGradient
        with pytest.raises(TypeError):
            CG(a.force)
        with pytest.raises(ValueError, match="multilevel"):
            CG(full, preconditioner="multilevel")
        k = fc.TangentMatrix(full.force)
        with pytest.raises(ValueError, match="multilevel"):
            CG(full, preconditioner=fc.MultilevelPreconditioner(k))
        with pytest.raises(ValueError, match="preconditioner"):
            CG(full, preconditioner="ilu")
        with pytest.raises(ValueError, match="belongs to no cell"):
            CG(a)  # the lonely node
        with pytest.raises(TypeError):
            fc.BiCGStab(full)
        cg = CG(full, preconditioner=None, maxiter=7, check_every=3)
        assert (cg.preconditioner, cg.maxiter, cg.check_every) == (None, 7, 3) and CG(full).maxiter == 10 * full.shape[0]
        nt = 36 * full.n_points
        with pytest.raises(TypeError):
            cg(np.zeros(nt), host(full.shape[0]))
        with pytest.raises(ValueError, match="cuda"):
            cg(host(nt), host(full.shape[0]))
    finally:
        jit.launch = real
    assert not launches
    assert not a._mask_on and not a._scratch and not a.force._on and not a.op._on and not cg._work and not cg._op._on  # nothing was uploaded


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the oracle against the oracle of the assembled matrix
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_product_against_the_matrix(shape):
    d_, a_, q_, affine = SHAPES[shape]
    for n_cells, seed in ((1, 4), (9, 11)):
        t = distinct_inputs(shape, n_cells, seed, False, affine)
        tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
        v = np.random.default_rng(seed).normal(size=d_ * t["n_nodes"])
        for mask in (None, random_mask(t, d_, seed + 1, whole_cell=n_cells // 2)):
            indptr, indices, blocks = matrix_oracle(t["tangent"], *tables, constrained=mask)
            want = to_bsr(indptr, indices, blocks, t["n_nodes"]) @ v
            have = product_oracle(t["tangent"], v, *tables, mask=mask)
            chain = product_chain_length(t["dofmap"], t["ref"], t["n_nodes"], int(np.diff(indptr).max()))
            bound = chain * EPS * product_oracle(t["tangent"], v, *tables, mask=mask, absolute=True)
            assert (np.abs(have - want) <= bound).all() and np.abs(want).max() > 0, (shape, n_cells)
            assert (bits(have.reshape(-1, d_)[t["lonely"]]) == 0).all()  # a node in no cell: +0.0
            if mask is not None:
                assert mask.any() and np.array_equal(bits(have[mask]), bits(v[mask]))  # the identity's rows, exactly
                # the constrained columns: v's values there do not reach the free rows
                other = np.where(mask, 7.0, v)
                assert np.array_equal(bits(product_oracle(t["tangent"], other, *tables, mask=mask)[~mask]), bits(have[~mask]))


@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_oracle_diagonal_blocks_are_the_matrix_on_the_bits(shape):
    d_, a_, q_, affine = SHAPES[shape]
    n_cells = 9
    t = distinct_inputs(shape, n_cells, 17, False, affine)
    tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
    for mask in (None, random_mask(t, d_, 5, whole_cell=2)):
        want = diagonal_blocks(*matrix_oracle(t["tangent"], *tables, constrained=mask))
        assert np.abs(want).max() > 0 and (bits(want[t["lonely"]]) == 0).all()
        for chunk in (None, 1, 2, 4, n_cells - 1, n_cells):
            have = diagonal_blocks_oracle(t["tangent"], *tables, mask=mask, chunk_cells=chunk)
            assert np.array_equal(bits(have), bits(want)), (shape, chunk)
    # a repeated node is why the operator refuses such cells: the matrix's block then holds off-diagonal element entries too
    r = random_inputs(shape, n_cells, 17, False, affine)
    r["dofmap"][0, -1] = r["dofmap"][0, 0]
    rt = (r["dofmap"], r["ref"], r["jinv"], r["weights"], r["n_nodes"])
    assert not np.array_equal(diagonal_blocks_oracle(r["tangent"], *rt), diagonal_blocks(*matrix_oracle(r["tangent"], *rt)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. the oracle against an independent dense stiffness in extended precision, at every tiling
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_cases():
    """per shape: the inputs, the mask and the dense K (np.longdouble, tangent_operator_util.dense_stiffness) without and with it;
    formed once, read by both comparisons"""
    cache = {}

    def get(shape):
        if shape not in cache:
            d_, a_, q_, affine = TILING_SHAPES[shape]
            cases = []
            for n_cells, seed in ((1, 4), (3 if a_ >= 64 else 9, 11)):
                t = distinct_inputs(shape, n_cells, seed, False, affine)
                tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
                mask = random_mask(t, d_, seed + 1, whole_cell=n_cells // 2)
                cases.append((n_cells, seed, t, tables, mask, {None: dense_stiffness(tables, t["tangent"]), "mask": dense_stiffness(tables, t["tangent"], mask)}))
            cache[shape] = cases
        return cache[shape]

    return get


@pytest.mark.parametrize("shape", sorted(TILING_SHAPES))
def test_oracle_product_against_the_dense_stiffness(shape, dense_cases):
    """product_oracle against K v with K = sum_p w_p B_p^T C_p B_p in np.longdouble.  The bound per entry is the chain of the
    matrix-free side alone -- the gradient's A + D + 2 roundings and the tangent action's (force_util.chain_length) -- times 2^-52
    times the S of the oracle's expression with every factor's absolute value; the reference's own error, 2^-64 per operation, is
    far inside it."""
    d_, a_, q_, affine = TILING_SHAPES[shape]
    worst = 0.0
    for n_cells, seed, t, tables, mask, dense in dense_cases(shape):
        v = np.random.default_rng(seed).normal(size=d_ * t["n_nodes"])
        for m in (None, mask):
            want = dense[None if m is None else "mask"] @ v.astype(np.longdouble)
            have = product_oracle(t["tangent"], v, *tables, mask=m)
            chain = (a_ + d_ + 2) + chain_length(d_, q_, max_valence(t["dofmap"], t["n_nodes"]), True)
            bound = chain * EPS * product_oracle(t["tangent"], v, *tables, mask=m, absolute=True)
            err = np.abs(have.astype(np.longdouble) - want).astype(np.float64)
            assert (err <= bound).all() and np.abs(want).max() > 0, (shape, n_cells, (err[bound > 0] / bound[bound > 0]).max())
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            assert (bits(have.reshape(-1, d_)[t["lonely"]]) == 0).all()
            if m is not None:
                assert m.any() and np.array_equal(bits(have[m]), bits(v[m]))
    print(f"{shape}: the ordered product against the dense stiffness at most {worst:.3f} of the bound")


@pytest.mark.parametrize("shape", sorted(TILING_SHAPES))
def test_oracle_diagonal_blocks_against_the_dense_stiffness(shape, dense_cases):
    """diagonal_blocks_oracle against the nodes' own blocks of the dense K: within the chain of an entry of the assembled matrix
    (force_util.chain_length with the node's cells for the contributions, as test_tangent_matrix.py bounds K) times 2^-52 times the
    oracle's expression with every factor's absolute value -- what makes the oracle trustworthy where no TangentMatrix exists"""
    d_, a_, q_, affine = TILING_SHAPES[shape]
    worst = 0.0
    for n_cells, seed, t, tables, mask, dense in dense_cases(shape):
        chain = chain_length(d_, q_, max_valence(t["dofmap"], t["n_nodes"]), True)
        bound = chain * EPS * diagonal_blocks_oracle(t["tangent"], *tables, absolute=True)
        for m in (None, mask):
            want = dense_diagonal_blocks(dense[None if m is None else "mask"], t["n_nodes"], d_)
            have = diagonal_blocks_oracle(t["tangent"], *tables, mask=m)
            err = np.abs(have.astype(np.longdouble) - want).astype(np.float64)
            assert (err <= bound).all() and np.abs(want).max() > 0, (shape, n_cells, (err[bound > 0] / bound[bound > 0]).max())
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            if m is not None:  # the constants of the constrained rows and columns, exactly
                hit = m.reshape(-1, d_)[:, :, None] | m.reshape(-1, d_)[:, None, :]
                assert hit.any() and np.array_equal(have[hit], want[hit].astype(np.float64))
    print(f"{shape}: the ordered diagonal blocks against the dense stiffness at most {worst:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c. the wide elements: the operator is the only route
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide64", "wide70"])
def test_wide_elements_have_no_matrix(shape):
    d_, a_, q_, affine = TILING_SHAPES[shape]
    assert shape in NO_MATRIX
    a, t = operator(shape, n_cells=3, every_node=True)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        with pytest.raises(ValueError, match="does not compile without scratch"):
            fc.TangentMatrix(a.force)
        with pytest.raises(ValueError, match="does not compile without scratch"):
            fc.MultilevelPreconditioner(a)  # its coarse levels are gathered from the element matrices
        for pc in ("block_jacobi", None):
            cg = fc.ConjugateGradient(a, preconditioner=pc)
            assert cg.preconditioner == pc and cg.maxiter == 10 * a.shape[0]
    finally:
        jit.launch = real
    assert not launches and a.shape == (d_ * t["n_nodes"],) * 2 and a.diagonal_cells_per_tile == 1


@pytest.fixture(scope="module")
def oracle_loop():
    """the Newton loop of the example on the CPU with the oracle law and the oracle conjugate gradients on the oracle operator"""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(O.von_mises_3d, VM_P, {"eps_n": 6, "alpha": 1}), mesh.n_points)

    direct = FE.tension_test(mesh, cpu_state(), steps=8)
    loop = oracle_free_loop(cpu_state(), dofmap, ref, jinv, weights, mesh.n_nodes, rtol=1e-12)
    return mesh, direct, loop, tension_test_device_solve(mesh, loop, steps=8)


def test_oracle_solves_of_the_cube_reproduce_the_direct_solver(oracle_loop):
    mesh, direct, loop, (reactions, norms, u, solves) = oracle_loop
    counts = [len(h) for h in norms]
    difference = np.max(np.abs(reactions - direct[0])) / np.max(np.abs(direct[0]))
    print(f"oracle loop on the oracle operator: Newton iterations {counts}, conjugate-gradient iterations {min(solves)} .. {max(solves)} {solves}, "
          f"largest relative reaction difference to the direct solve {difference:.2e}")
    assert counts == [len(h) for h in direct[1]] == [2, 2, 2, 3, 3, 4, 5, 5]
    assert len(loop.systems) == len(solves) == sum(counts) - 8
    assert all(result.converged and result.residual_norm <= 1e-12 * result.rhs_norm for _, _, result in loop.systems)
    assert difference <= 1e-8
