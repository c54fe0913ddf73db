"""The device solver on the GPU (fenics_constitutive_amd.ConjugateGradient, csrc/jit/conjugate_gradient.hip): the ordered dot, the
matrix-vector product and whole conjugate-gradient runs compared ON THE BITS with the NumPy oracle of solver_util.py -- in both
formats, with and without the preconditioner and a start vector, under a grid capped at one compute unit, for every
``check_every`` --, the statuses, the refusals, and the Newton loop of examples/cube_tension_device_solve.py."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import DeviceSolveLoop, tension_test_device_solve  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import gradient, jit, solver  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from fe_gpu_util import CANARY, MARGIN, bits, guarded, assert_margins_intact, assert_same_bits, solve_guarded, assert_same_result  # noqa: E402
from fe_gpu_util import one_cu  # noqa: E402, F401 (the fixture: pytest finds it in this namespace)
from force_util import MANDEL_DIM, random_inputs  # noqa: E402
from gradient_util import EPS, SHAPES, cube_operator_tables  # noqa: E402
from solver_util import SEG, conjugate_gradient, from_format, full_pattern, matvec, oracle_solve_loop, ordered_dot, spd_tangent  # noqa: E402

FORMATS = ("bsr", "csr")
CG_SHAPES = ("hex8", "tet_p2", "tri_p2", "interval")
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the ordered dot
# ---------------------------------------------------------------------------------------------------------------------------------
DOT_LENGTHS = (1, 255, 256, 257, SEG - 1, SEG, SEG + 1, 2 * SEG + 5, 256 * SEG + 1)


def dot_inputs(n, integer):
    rng = np.random.default_rng(n + integer)
    if integer:
        return rng.integers(-8, 9, size=n).astype(np.float64), rng.integers(-8, 9, size=n).astype(np.float64)
    return rng.normal(size=n), rng.normal(size=n) * np.exp(rng.normal(size=n))


def check_dots():
    for n in DOT_LENGTHS:
        for integer in (True, False):
            a, b = dot_inputs(n, integer)
            have, want = solver.dot(to_device(a, "cuda"), to_device(b, "cuda")), ordered_dot(a, b)
            assert bits(np.float64(have)) == bits(np.float64(want)), (n, integer, have, want)
            if integer:
                assert have == float((a.astype(np.int64) * b.astype(np.int64)).sum())


def test_dot_on_the_bits():
    check_dots()
    assert -(-DOT_LENGTHS[-1] // SEG) == 257  # more partials than lanes


def test_dot_on_one_compute_unit(one_cu):
    check_dots()
    assert {name for name, _ in one_cu} == {solver.DOT_KERNEL} and max(b for _, b in one_cu) == gradient.BLOCKS_PER_CU
    assert min(b for _, b in one_cu) == 1  # the last block is the only block


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the matrix-vector product
# ---------------------------------------------------------------------------------------------------------------------------------
def assembled(shape, n_cells, seed, fmt, integer=False, every_node=False, fraction=0.2):
    """(K, values on the device, blocks on the host, tables, mask): an assembled symmetric positive semi-definite matrix of random
    tables with random constrained dofs; ``every_node``: the nodes no cell touches get a block of their own and are constrained"""
    d_, a_, q_, affine = SHAPES[shape]
    t = random_inputs(shape, n_cells, seed, integer, affine)
    f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])
    pat, unused = full_pattern(t["dofmap"], t["n_nodes"])
    k = fc.TangentMatrix(f, format=fmt, pattern_dofmap=pat if every_node else None)
    used = np.ones(t["n_nodes"], dtype=bool)
    used[unused] = False
    mask = (np.random.default_rng(seed + 5).random(d_ * t["n_nodes"]) < fraction) & np.repeat(used, d_)
    if every_node:
        mask |= np.repeat(~used, d_)
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(n_cells * q_, MANDEL_DIM[d_], seed, integer), "cuda"))
    torch.cuda.synchronize()
    return k, values, from_format(fmt, k.indptr, k.indices, to_host(values), d_), t, mask


def check_matvec(k, values, blocks, p, what):
    n = k.shape[0]
    buf, out = guarded(n)
    got = solver.matvec(k, values, to_device(p, "cuda"), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert_margins_intact(buf, n)
    have = to_host(out)
    assert_same_bits(have, matvec(k.indptr, k.indices, blocks, p), what)
    # against SciPy's product of the same values, within the bound of one chain: D * (blocks of the longest row) sums and products
    a = k.to_scipy(values)
    chain = k.gdim * int(np.diff(k.indptr).max()) + 2
    bound = chain * EPS * (abs(a) @ np.abs(p))
    assert (np.abs(have - a @ p) <= bound).all(), what
    return have


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", CG_SHAPES)
def test_matvec_on_the_bits(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    for n_cells in (1, 5, -(-257 // q_)):
        for integer in (True, False):
            k, values, blocks, t, mask = assembled(shape, n_cells, 3 + n_cells + integer, fmt, integer)
            rng = np.random.default_rng(n_cells)
            p = rng.integers(-8, 9, size=k.shape[0]).astype(np.float64) if integer else rng.normal(size=k.shape[0])
            have = check_matvec(k, values, blocks, p, f"{shape} {fmt} cells={n_cells} integer={integer}")
            assert (bits(have.reshape(-1, d_)[t["lonely"]]) == 0).all()  # the row without blocks: +0.0
            assert np.array_equal(have[mask], p[mask]) and np.abs(have).max() > 0  # the identity's rows
    assert solver.matvec(k, values, to_device(p, "cuda")).shape == (k.shape[0],)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", CG_SHAPES)
def test_matvec_rows_without_blocks_at_the_end(shape, fmt):
    """the last nodes are in no cell: their rows start where the values end (block CSR: nothing of them may be read past the array)"""
    d_, a_, q_, affine = SHAPES[shape]
    for extra in (1, 2, 70):  # (70: whole waves of rows without blocks)
        t = random_inputs(shape, 5, 31, False, affine)
        n_nodes = t["n_nodes"] + extra
        f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], n_nodes), t["weights"])
        k = fc.TangentMatrix(f, format=fmt)
        assert k.indptr[-1 - extra] == k.indptr[-1] == k.nnzb and k.diag_block[-1] == -1
        buf, values = guarded(k.nnz)  # canaries behind the values: a read past them would put a NaN into a product
        k(to_device(spd_tangent(5 * q_, MANDEL_DIM[d_], 3, False), "cuda"), out=values)
        torch.cuda.synchronize()
        p = np.random.default_rng(extra).normal(size=k.shape[0])
        have = check_matvec(k, values, from_format(fmt, k.indptr, k.indices, to_host(values), d_), p, f"{shape} {fmt} {extra} empty rows at the end")
        assert (bits(have[-d_ * extra:]) == 0).all() and np.abs(have).max() > 0
        assert_margins_intact(buf, k.nnz)


@pytest.mark.parametrize("fmt", FORMATS)
def test_matvec_of_a_pattern_without_blocks(fmt):
    t = random_inputs("hex8", 1, 2, False, False)
    for n_nodes in (t["n_nodes"], 300):
        empty_f = fc.InternalForce(fc.DisplacementGradient(t["dofmap"][:0], t["ref"], t["jinv"][:0], n_nodes), t["weights"][:0])
        k = fc.TangentMatrix(empty_f, format=fmt)
        assert k.nnz == 0 and k.nnzb == 0
        n = k.shape[0]
        buf, out = guarded(n)
        values = torch.zeros(0, dtype=torch.float64, device="cuda")
        solver.matvec(k, values, to_device(np.arange(1.0, n + 1.0), "cuda"), out=out)
        torch.cuda.synchronize()
        assert_margins_intact(buf, n)
        assert (bits(to_host(out)) == 0).all()


@pytest.fixture(scope="module")
def big_cube():
    """the pattern of a cube of 32^3 hexahedra (35 937 nodes, rows of 8 to 27 blocks): 36 segments, more than two trips of the 16
    blocks a single compute unit is capped at"""
    mesh = FE.Cube(32, 32, 32)
    op, f = cube_operators(mesh)
    assert -(-mesh.n_dofs // SEG) > 2 * gradient.BLOCKS_PER_CU
    return mesh, f


@pytest.mark.parametrize("fmt", FORMATS)
def test_matvec_grid_stride_loop(fmt, big_cube, one_cu):
    mesh, f = big_cube
    k = fc.TangentMatrix(f, format=fmt)
    rng = np.random.default_rng(9)
    flat = rng.normal(size=k.nnz)  # the product does not care where the values come from
    p = rng.normal(size=k.shape[0])
    check_matvec(k, to_device(flat, "cuda"), from_format(fmt, k.indptr, k.indices, flat, 3), p, f"cube 32 {fmt}, one compute unit")
    assert one_cu == [(solver.MATVEC_KERNEL, gradient.BLOCKS_PER_CU)]  # the launch really was capped
    assert np.diff(k.indptr).min() == 8 and np.diff(k.indptr).max() == 27


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exactly k iterations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", CG_SHAPES)
def test_exactly_k_iterations(shape, fmt):
    d_, a_, q_, _ = SHAPES[shape]
    k, values, blocks, t, mask = assembled(shape, -(-257 // q_), 21, fmt, every_node=True)
    rng = np.random.default_rng(4)
    b = np.where(mask, 0.0, rng.normal(size=k.shape[0]))
    start = rng.normal(size=k.shape[0])
    for pc in ("block_jacobi", None):
        for its in (1, 2, 7):
            cg = fc.ConjugateGradient(k, preconditioner=pc, rtol=0.0, maxiter=its)
            for x0 in (None, start):
                what = f"{shape} {fmt} {pc} k={its} x0={'yes' if x0 is not None else 'no'}"
                want = conjugate_gradient(k.indptr, k.indices, blocks, b, x0=x0, preconditioner=pc, rtol=0.0, maxiter=its)
                res, x = solve_guarded(cg, values, b, x0)
                assert want.status == "maxiter" and want.iterations == its, what
                assert_same_result(res, x, want, what)
        # without out: a new tensor, x0 untouched
        x0_dev = to_device(start, "cuda")
        res = cg(values, to_device(b, "cuda"), x0=x0_dev)
        assert res.x.data_ptr() != x0_dev.data_ptr() and np.array_equal(to_host(x0_dev), start)
        assert_same_bits(to_host(res.x), want.x, f"{shape} {fmt} {pc}: without out")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a cube with two segments: check_every, the statuses
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube_system():
    """the elastic tension-test matrix of a cube of 10^3 hexahedra (3993 dofs: two segments), its right-hand side and oracle solves"""
    from cube_tension_device_solve import tension_constraints

    mesh = FE.Cube(10, 10, 10)
    op, f = cube_operators(mesh)
    mask, top = tension_constraints(mesh)
    assert SEG < mesh.n_dofs <= 2 * SEG
    tangent = spd_tangent(mesh.n_points, 6, 1, False)
    rng = np.random.default_rng(12)
    b = np.where(mask, 0.0, rng.normal(size=mesh.n_dofs))
    out = {}
    for fmt in FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        k.set_constrained(mask)
        values = k(to_device(tangent, "cuda"))
        torch.cuda.synchronize()
        out[fmt] = (k, values, from_format(fmt, k.indptr, k.indices, to_host(values), 3))
    assert_same_bits(out["bsr"][2], out["csr"][2], "the two formats hold one matrix")
    k, _, blocks = out["bsr"]
    oracle = {(pc, kw): conjugate_gradient(k.indptr, k.indices, blocks, b, preconditioner=pc, **dict(kw))
              for pc in ("block_jacobi", None) for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),))}
    return mesh, mask, b, out, oracle


@pytest.mark.parametrize("pc", ["block_jacobi", None])
@pytest.mark.parametrize("fmt", FORMATS)
def test_check_every_changes_nothing(fmt, pc, cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems[fmt]
    for kw in ((("rtol", 0.0), ("maxiter", 11)), (("rtol", 1e-6),)):
        want = oracle[(pc, kw)]
        assert want.status == ("maxiter" if "maxiter" in dict(kw) else "converged") and want.iterations >= 11
        for every in (1, 3, 16):  # (11 iterations end in the middle of a batch of 3 and of 16; so does the converged solve's last)
            res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, check_every=every, **dict(kw)), values, b)
            assert_same_result(res, x, want, f"{fmt} {pc} {dict(kw)} check_every={every}")
    assert oracle[("block_jacobi", kw)].iterations < oracle[(None, kw)].iterations


def test_on_one_compute_unit(cube_system, big_cube, one_cu):
    from cube_tension_device_solve import tension_constraints

    # two iterations on 36 segments: every kernel's grid-stride loop makes more than two trips
    big, f = big_cube
    k = fc.TangentMatrix(f, format="csr")
    mask, _ = tension_constraints(big)
    k.set_constrained(mask)
    values = k(to_device(spd_tangent(big.n_points, 6, 2, False), "cuda"))
    torch.cuda.synchronize()
    blocks = from_format("csr", k.indptr, k.indices, to_host(values), 3)
    b = np.where(mask, 0.0, np.random.default_rng(3).normal(size=big.n_dofs))
    del one_cu[:]
    res, x = solve_guarded(fc.ConjugateGradient(k, rtol=0.0, maxiter=2, check_every=2), values, b)
    assert_same_result(res, x, conjugate_gradient(k.indptr, k.indices, blocks, b, rtol=0.0, maxiter=2), "cube 32, one compute unit")
    assert {(name, nb) for name, nb in one_cu} == {(name, gradient.BLOCKS_PER_CU) for name in (solver.INVERSE_KERNEL, solver.MATVEC_KERNEL,
                                                                                                solver.UPDATE_KERNEL, solver.DIRECTION_KERNEL)}
    del one_cu[:]
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["csr"]
    kw = (("rtol", 1e-6),)
    res, x = solve_guarded(fc.ConjugateGradient(k, **dict(kw)), values, b)
    assert_same_result(res, x, oracle[("block_jacobi", kw)], "one compute unit")
    assert {name for name, _ in one_cu} == {solver.INVERSE_KERNEL, solver.MATVEC_KERNEL, solver.UPDATE_KERNEL, solver.DIRECTION_KERNEL}


def test_statuses(cube_system):
    mesh, mask, b, systems, oracle = cube_system
    k, values, blocks = systems["bsr"]
    n = b.size
    start = np.random.default_rng(2).normal(size=n)
    for pc in ("block_jacobi", None):
        cg = fc.ConjugateGradient(k, preconditioner=pc, rtol=1e-6)
        # -K: indefinite at the first product, x is x0 on the bits
        res, x = solve_guarded(cg, -values, b, start)
        assert (res.status, res.iterations, res.converged) == ("indefinite", 0, False)
        assert_same_bits(x, start, f"{pc}: indefinite")
        assert_same_result(res, x, conjugate_gradient(k.indptr, k.indices, -blocks, b, x0=start, preconditioner=pc, rtol=1e-6), f"{pc}: indefinite")
        # b = 0: converged at once, no 0/0
        for x0 in (None, np.zeros(n)):
            res, x = solve_guarded(cg, values, np.zeros(n), x0)
            assert (res.status, res.iterations, res.converged, res.residual_norm, res.rhs_norm) == ("converged", 0, True, 0.0, 0.0)
            assert res.looks == 1  # ended at the start: no iteration was enqueued
            assert (bits(x) == 0).all()
        # maxiter reached
        short = fc.ConjugateGradient(k, preconditioner=pc, rtol=1e-12, maxiter=5)
        res, x = solve_guarded(short, values, b)
        assert (res.status, res.iterations, res.converged) == ("maxiter", 5, False) and np.isfinite(x).all() and res.residual_norm > 0
        res, x = solve_guarded(fc.ConjugateGradient(k, preconditioner=pc, maxiter=0), values, b, start)
        assert (res.status, res.iterations, res.looks) == ("maxiter", 0, 1)
        assert_same_bits(x, start, f"{pc}: maxiter 0")
    # a zeroed diagonal block: no iteration, x is x0
    broken = values.clone()
    node = mesh.n_nodes // 2
    broken.reshape(-1, 3, 3)[int(k.diag_block[node])] = 0.0
    res, x = solve_guarded(fc.ConjugateGradient(k), broken, b, start)
    assert (res.status, res.iterations, res.converged, res.looks) == ("singular_block", 0, False, 1)
    assert_same_bits(x, start, "singular block")
    bad = b.copy()
    bad[17] = np.nan
    res, x = solve_guarded(fc.ConjugateGradient(k), values, bad)
    assert res.status == "nonfinite" and res.iterations == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals come before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    k, values, blocks, t, mask = assembled("hex8", 21, 11, "bsr", every_node=True)
    n, nnz = k.shape[0], k.nnz
    cg = fc.ConjugateGradient(k)
    b = to_device(np.where(mask, 0.0, 1.0), "cuda")
    assert cg(values, b).converged  # tables uploaded, kernels loaded: what follows can only add launches
    buf, out = guarded(n)
    spare = torch.zeros(2 * max(n, nnz) + 2, dtype=torch.float64, device="cuda")
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        with pytest.raises(ValueError, match="aligned"):
            cg(values, b, out=buf[MARGIN + 1: MARGIN + 1 + n])
        with pytest.raises(ValueError, match="entries"):
            cg(values, b, out=buf[MARGIN: MARGIN + n - 3])
        with pytest.raises(ValueError, match="contiguous"):
            cg(values, b, out=spare[: 2 * n: 2])
        with pytest.raises(ValueError, match="cuda"):
            cg(values, b, out=torch.empty(n, dtype=torch.float64))
        with pytest.raises(TypeError):
            cg(values, b, out=out.float())
        with pytest.raises(ValueError, match="alias"):
            cg(values, b, out=b)
        with pytest.raises(ValueError, match="x0 itself"):
            cg(values, b, x0=spare[2: 2 + n], out=spare[:n])
        with pytest.raises(ValueError, match="entries"):
            cg(values[:-9], b, out=out)
        with pytest.raises(ValueError, match="entries"):
            cg(values, b[:-3], out=out)
        with pytest.raises(ValueError, match="aligned"):
            cg(values, spare[1: 1 + n], out=out)
        with pytest.raises(ValueError, match="contiguous"):
            cg(values, b, x0=spare[: 2 * n: 2], out=out)
        with pytest.raises(TypeError):
            cg(values, to_host(b), out=out)
        with pytest.raises(TypeError):
            cg(values.float(), b, out=out)
        with pytest.raises(ValueError, match="cuda"):
            cg(values, b.cpu(), out=out)
        with pytest.raises(ValueError, match="entries"):
            solver.matvec(k, values, b[:-3])
        with pytest.raises(ValueError, match="alias"):
            solver.matvec(k, values, b, out=b)
        with pytest.raises(ValueError, match="entries"):
            solver.dot(b, b[:-1])
        with pytest.raises(ValueError, match="contiguous"):
            solver.dot(spare[: 2 * n: 2], b)
        lonely, _, _, _, _ = assembled("hex8", 21, 11, "bsr")
        with pytest.raises(ValueError, match="no diagonal block"):
            fc.ConjugateGradient(lonely)
    finally:
        jit.launch = real
    torch.cuda.synchronize()
    assert [a[-1] for a in launches if "TangentMatrix" not in a[-1]] == []  # (the last helper assembled a matrix)
    assert (bits(to_host(buf)) == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the Newton loop with the solve on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear_elasticity", "von_mises_3d"])
def test_in_the_loop_behind_a_resident_state(kind):
    """The example's loop on Cube(3, 2, 4), eight load steps, ConjugateGradient(rtol=1e-12), against the same loop on the CPU with
    the NumPy oracle law, the oracle matrix and the oracle conjugate gradients: the Newton counts are equal, the conjugate-gradient
    counts equal up to one (the solver is bit-equal, the device law's last bits are not).  The reaction tolerance: the CPU oracle
    loop differs from the host direct solve by ``delta`` relative to the largest reaction; the GPU run is allowed ten times that
    (the margin of the assembled loop's test), and never more than 1e-8.
    Measured on the CPU (von_mises_3d): Newton counts (2, 2, 2, 3, 3, 4, 5, 5), 66 to 72 iterations per solve, delta = 2.41e-14."""
    from oracle import numpy_oracle as O

    mesh = FE.Cube(3, 2, 4)
    n = mesh.n_points
    if kind == "von_mises_3d":
        oracle_law, hist, law, params = O.von_mises_3d, {"eps_n": 6, "alpha": 1}, (lambda: fc.VonMises3D(VM_P)), VM_P
    else:
        params = {"E": 42.0, "nu": 0.3}
        oracle_law, hist, law = O.linear_elasticity, None, (lambda: fc.LinearElasticityModel(params, fc.StressStrainConstraint.FULL))

    def cpu_state():
        return FE.CopyProtocolState(FE.OracleLaw(oracle_law, params, hist), n)

    r_direct, norms_direct, _ = FE.tension_test(mesh, cpu_state(), steps=8)
    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    r_cpu, norms_cpu, _, solves_cpu = tension_test_device_solve(mesh, oracle_solve_loop(cpu_state(), dofmap, ref, jinv, f._weights, mesh.n_nodes, rtol=1e-12), steps=8)
    scale = np.max(np.abs(r_direct))
    delta = np.max(np.abs(r_cpu - r_direct)) / scale
    for fmt in FORMATS:
        k = fc.TangentMatrix(f, format=fmt)
        loop = DeviceSolveLoop(ResidentState(law(), n, placement="torch"), op, f, k, fc.ConjugateGradient(k, rtol=1e-12))
        r_gpu, norms_gpu, u, solves = tension_test_device_solve(mesh, loop, steps=8)  # (raises where a solve or a load step does not converge)
        difference = np.max(np.abs(r_gpu - r_direct)) / scale
        counts = [len(h) for h in norms_gpu]
        print(f"device-solve tension test, {kind} {fmt}: delta (CPU oracle loop against direct) {delta:.3e}, GPU against direct {difference:.3e}, "
              f"Newton iterations {counts}, conjugate-gradient iterations {solves} (CPU oracle: {solves_cpu})")
        assert counts == [len(h) for h in norms_cpu] == [len(h) for h in norms_direct]
        if kind == "von_mises_3d":
            assert counts == [2, 2, 2, 3, 3, 4, 5, 5]
        assert loop.assemblies == len(solves) == len(solves_cpu) == sum(counts) - 8
        assert all(abs(a - b) <= 1 for a, b in zip(solves, solves_cpu)), (solves, solves_cpu)
        assert difference <= min(10 * delta, 1e-8), (difference, delta)
        looks = sum(1 + -(-its // 16) for its in solves)  # one after the start, one behind every batch of check_every = 16
        assert loop.bytes_up == 8 * mesh.n_dofs * loop.evaluations + 96 * len(solves)
        assert loop.bytes_down == 24 * loop.evaluations + 8 * mesh.n_dofs * len(solves) + 32 * looks
