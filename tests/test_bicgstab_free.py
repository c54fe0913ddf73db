"""BiCGStab on the matrix-free tangent operator without a GPU (fenics_constitutive_amd.bicgstab_free, csrc/jit/bicgstab_free.hip):
the program compiles for gfx950 at every tiling the operator's template generates, the new kernel without scratch and with the LDS
of the tree alone and the operator's kernels in it as the operator's own program has them; the ctypes mirror has the struct's size;
constructing and every refusal come before any upload or launch; ``fc.BiCGStab(A)`` stays a TypeError; and the oracle
(bicgstab_free_util.py) on its own: it solves the unsymmetric cube the oracle conjugate gradients do not, to the dense solve of a
stiffness that shares no code with it, and runs the iteration counts of the GPU tests without a breakdown inside."""

import ctypes
import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import bicgstab, bicgstab_free, jit, solver
from fenics_constitutive_amd import tangent_operator as to
from fenics_constitutive_amd.force import kernel_resources

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402
from bicgstab_free_util import K_CYCLES, K_ITERATIONS, K_SHAPES, k_iterations_system, operator_solve  # noqa: E402
from bicgstab_util import nonassociated_tangent  # noqa: E402
from force_util import MANDEL_DIM  # noqa: E402
from gradient_util import cube_operator_tables  # noqa: E402
from multilevel_free_util import FreeOracle  # noqa: E402
from tangent_operator_util import TILING_SHAPES, dense_stiffness, distinct_inputs  # noqa: E402
from tangent_operator_util import operator_solve as cg_operator_solve  # noqa: E402

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
    own = to.compile_kernels(d_, a_, q_, affine)
    code = bicgstab_free.compile_kernels(d_, a_, q_, affine, own.slab, own.waves)
    r = kernel_resources(code.log, bicgstab_free.NODE_DOTS_KERNEL)
    assert r["scratch_bytes"] == 0, r
    assert r["lds_bytes"] == solver.lds_bytes(solver.DOT_KERNEL) == 8 * 258  # the tree and the flag: the second tree shares the array
    assert (r["agprs"] or 0) == 0 and r["vgprs"] <= 64, r  # nothing that costs the memory-bound kernel its occupancy
    # the operator's kernels in this program are those of the operator's own
    for kernel in to.KERNELS:
        assert kernel_resources(code.log, kernel) == kernel_resources(own.log, kernel), kernel
    before = jit.compile_count()
    assert bicgstab_free.compile_kernels(d_, a_, q_, affine, own.slab, own.waves) is code and jit.compile_count() == before  # once per program text


def test_the_other_programs_keep_their_text():
    """the compile cache is keyed by the text: the operator's, the assembled BiCGStab's and the conjugate gradients' do not name the new file"""
    assert to.program(3, 8, 8, False, 4, 2) == ("#define FCAMD_TO_D 3\n#define FCAMD_TO_A 8\n#define FCAMD_TO_Q 8\n#define FCAMD_TO_AFFINE 0\n"
                                                 '#define FCAMD_TO_SLAB 4\n#define FCAMD_TO_WAVES 2\n#include "tangent_operator.hip"\n')
    assert bicgstab.program(3, "block_jacobi") == '#define FCAMD_CG_D 3\n#define FCAMD_CG_PRECOND 1\n#define FCAMD_CG_SLAB 1024\n#include "bicgstab.hip"\n'
    assert solver.program(2, False) == '#define FCAMD_CG_D 2\n#define FCAMD_CG_PRECOND 0\n#define FCAMD_CG_SLAB 1024\n#include "conjugate_gradient.hip"\n'
    text = bicgstab_free.program(3, 8, 8, False, 4, 2)
    assert text == to.program(3, 8, 8, False, 4, 2).replace("tangent_operator.hip", "bicgstab_free.hip")
    closure = [os.path.basename(p) for p in jit.include_closure(text)]
    assert closure[:2] == ["bicgstab_free.hip", "tangent_operator.hip"] and "bicgstab.hip" in closure and "conjugate_gradient.hip" in closure
    assert "bicgstab_free.hip" not in [os.path.basename(p) for p in jit.include_closure(to.program(3, 8, 8, False, 4, 2))]


def test_object_reports_what_the_compiler_made():
    a, t = operator(every_node=True)
    s = fc.MatrixFreeBiCGStab(a)
    r = s.resources
    assert r["node_dots"]["scratch_bytes"] == 0 and r["scratch_bytes"] == 0 and r["lds_bytes"] == s.lds_bytes() == 8 * 258
    assert all(r[name]["scratch_bytes"] == 0 for name in ("node_dots", "element", "start", "half", "full", "direction", "inverse"))
    assert r["element"] == kernel_resources(a.compile_log, to.ELEMENT_KERNEL)
    assert bicgstab_free.NODE_DOTS_KERNEL in s.compile_log and all(kernel in s.compile_log for kernel in bicgstab.KERNELS)
    assert s.device == a.device and s.lds_bytes(bicgstab.HALF_KERNEL) == bicgstab.lds_bytes(bicgstab.HALF_KERNEL, "block_jacobi")
    assert "MatrixFreeBiCGStab" in fc.__all__ and fc.MatrixFreeBiCGStab is bicgstab_free.MatrixFreeBiCGStab
    assert bicgstab_free.STATUSES == bicgstab.STATUSES and bicgstab_free.STATUSES[6] == "breakdown"
    # the start, half-step, full-step and direction kernels are the assembled solver's own code object, kind by kind
    assert s._code is bicgstab.compile_kernels(3, "block_jacobi") and fc.MatrixFreeBiCGStab(a, preconditioner=None)._code is bicgstab.compile_kernels(3, None)
    assert fc.MatrixFreeBiCGStab(a, preconditioner=fc.MultilevelPreconditioner(a))._code is bicgstab.compile_kernels(3, "multilevel")
    assert fc.MatrixFreeBiCGStab(a)._product is s._product  # one program per operator


def test_the_ctypes_mirror_has_the_structs_size():
    """NodeArgs plus vb and dots: eight pointers, two 64-bit counts, mode and its pad (88 bytes: the static assertion of
    bicgstab_free.hip ties NodeDotsArgs to sizeof(NodeArgs) + 16 and puts vb at sizeof(NodeArgs)), a pointer, dots and its pad"""
    assert ctypes.sizeof(to.NodeArgs) == 88
    assert ctypes.sizeof(bicgstab_free.NodeDotsArgs) == 88 + 16 == 104
    assert bicgstab_free.NodeDotsArgs.vb.offset == 88 and bicgstab_free.NodeDotsArgs.dots.offset == 96
    assert [name for name, _ in bicgstab_free.NodeDotsArgs._fields_[:len(to.NodeArgs._fields_)]] == [name for name, _ in to.NodeArgs._fields_]
    assert ctypes.sizeof(bicgstab.Params) == ctypes.sizeof(solver.Args) + 32
    # the doubles of the control block the products' last blocks write: rr, bb, four ints, rho, rho_old, rv, thr2, rtol, atol, dot, ts, tt, alpha, omega
    assert (bicgstab_free._RV, bicgstab_free._TS, bicgstab_free._TT, bicgstab_free._OMEGA) == (6, 11, 12, 14) and bicgstab._SCALARS == 16
    assert (bicgstab_free.DOT_V, bicgstab_free.DOT_T) == (bicgstab._DOT_V, bicgstab._DOT_T)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. constructing and the refusals launch and upload nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_constructing_and_the_refusals_launch_nothing():
    a, t = operator()  # with a node in no cell
    full, _ = operator(every_node=True)
    other, _ = operator(every_node=True)
    launches = []
    real = jit.launch
    jit.launch = lambda *args, **kwargs: launches.append(args) or real(*args, **kwargs)
    try:
        S = fc.MatrixFreeBiCGStab
        k = fc.TangentMatrix(full.force)
        for wrong in (k, full.force, 3.0):
            with pytest.raises(TypeError, match="TangentOperator"):
                S(wrong)
        with pytest.raises(ValueError, match="multilevel"):
            S(full, preconditioner="multilevel")
        with pytest.raises(ValueError, match="preconditioner must be one of"):
            S(full, preconditioner="amg")
        with pytest.raises(ValueError, match="another object"):
            S(full, preconditioner=fc.MultilevelPreconditioner(other))
        with pytest.raises(ValueError, match="another object"):
            S(full, preconditioner=fc.MultilevelPreconditioner(k))
        with pytest.raises(ValueError, match="rigid_body"):
            S(full, preconditioner=fc.MultilevelPreconditioner(full, coarse_space="rigid_body", coordinates=np.zeros((full.n_nodes, 3))))
        with pytest.raises(ValueError, match=f"node {t['lonely']} belongs to no cell"):
            S(a)
        for bad, error in (({"rtol": -1.0}, ValueError), ({"rtol": np.inf}, ValueError), ({"rtol": "1e-8"}, TypeError), ({"atol": np.nan}, ValueError),
                           ({"maxiter": -1}, ValueError), ({"maxiter": 2**31}, ValueError), ({"maxiter": 2.0}, TypeError), ({"maxiter": True}, TypeError),
                           ({"check_every": 0}, ValueError), ({"check_every": 1.5}, TypeError)):
            with pytest.raises(error, match=next(iter(bad))):
                S(full, **bad)
        with pytest.raises(TypeError):
            fc.BiCGStab(full)  # the assembled solver does not change: this class is the entry point
        with pytest.raises(TypeError, match="TangentOperator"):
            bicgstab_free.product(k, None, None, None)
        s = S(full, preconditioner=None, maxiter=7, check_every=3, rtol=1e-6, atol=1e-3)
        assert (s.preconditioner, s.maxiter, s.check_every, s.rtol, s.atol) == (None, 7, 3, 1e-6, 1e-3) and S(full).maxiter == 10 * full.shape[0]
        pc = fc.MultilevelPreconditioner(full)
        assert S(full, preconditioner=pc).preconditioner is pc and S(full).preconditioner == "block_jacobi"
        torch = pytest.importorskip("torch")
        host = lambda m: torch.zeros(m, dtype=torch.float64)  # noqa: E731
        n, nt = full.shape[0], 36 * full.n_points
        for call in (lambda x, y: s(x, y), lambda x, y: bicgstab_free.product(full, x, y, y)):
            with pytest.raises(TypeError):
                call(np.zeros(nt), host(n))  # an ndarray
            with pytest.raises(TypeError):
                call(host(nt).float(), host(n))
            with pytest.raises(ValueError, match="cuda"):
                call(host(nt), host(n))  # on the host
    finally:
        jit.launch = real
    assert not launches
    for x in (a, full, other):
        assert not x._mask_on and not x._scratch and not x.force._on and not x.op._on  # nothing was uploaded
    assert not s._work and not s._work_blocks and not s._op._on and not s._product._control


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the oracle on its own
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unsymmetric_cube():
    """the tension-test system of a 3 x 3 x 3 cube of hexahedra with the non-associated tangent of bicgstab_util (b = 0.6, b_flow = 0 at
    30 % of the points)"""
    mesh = FE.Cube(3, 3, 3)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, cube_operators(mesh)[1]._weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    tangent = nonassociated_tangent(mesh.n_points)
    b = np.where(mask, 0.0, np.random.default_rng(12).normal(size=mesh.n_dofs))
    return tables, mask, tangent, b


def test_the_oracle_solves_what_the_oracle_conjugate_gradients_do_not(unsymmetric_cube):
    tables, mask, tangent, b = unsymmetric_cube
    k = dense_stiffness(tables, tangent, mask).astype(np.float64)
    assert np.linalg.norm(k - k.T) / np.linalg.norm(k) >= 0.1
    direct = np.linalg.solve(k, b)
    for pc in ("block_jacobi", None, FreeOracle(*tables, mask=mask, cycle="additive", coarsest_nodes=8),
               FreeOracle(*tables, mask=mask, cycle="multiplicative", coarsest_nodes=8)):
        res = operator_solve(tangent, b, *tables, mask=mask, preconditioner=pc, rtol=1e-10)
        assert res.status == "converged" and res.converged and 0 < res.iterations <= 200, (pc, res.status, res.iterations)
        assert res.residual_norm <= 1e-10 * res.rhs_norm
        assert np.linalg.norm(res.x - direct) <= 1e-6 * np.linalg.norm(direct), (pc, np.linalg.norm(res.x - direct) / np.linalg.norm(direct))
    cg = cg_operator_solve(tangent, b, *tables, mask=mask, rtol=1e-10, maxiter=10 * b.size)
    assert not cg.converged and cg.status in ("indefinite", "maxiter"), cg.status


@pytest.mark.parametrize("shape", K_SHAPES)
def test_the_oracle_runs_k_iterations_without_a_breakdown(shape):
    """for every k, shape, preconditioner and start of test_gpu_bicgstab_free.py::test_exactly_k_iterations the oracle ends as maxiter
    with k iterations counted: the GPU comparison is one of whole iterations, not of a breakdown's early end"""
    d_ = TILING_SHAPES[shape][0]
    t, mask, tangent, b, start = k_iterations_system(shape)
    tables = (t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"])
    assert tangent.size == MANDEL_DIM[d_] ** 2 * t["dofmap"].shape[0] * TILING_SHAPES[shape][2]
    if d_ > 1:
        c = tangent.reshape(-1, MANDEL_DIM[d_], MANDEL_DIM[d_])
        assert np.abs(c - c.transpose(0, 2, 1)).max() > 1.0  # the input is unsymmetric
    kinds = ["block_jacobi", None]
    if shape != "wide70":  # (no element matrix of 210 x 210 in the multilevel setup: tangent_operator_util.NO_MATRIX)
        kinds += [FreeOracle(*tables, mask=mask, cycle=cycle, coarsest_nodes=4) for cycle in K_CYCLES]
    for pc in kinds:
        for k in K_ITERATIONS:
            for x0 in (None, start):
                res = operator_solve(tangent, b, *tables, mask=mask, x0=x0, preconditioner=pc, rtol=0.0, maxiter=k)
                assert (res.status, res.iterations) == ("maxiter", k), (shape, getattr(pc, "cycle", pc), k, x0 is not None, res.status)
                assert np.isfinite(res.x).all() and res.residual_norm > 0.0
