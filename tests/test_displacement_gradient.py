"""The gradient producer without a GPU (fenics_constitutive_amd.gradient, csrc/jit/displacement_gradient.hip): every shape compiles
for gfx950 without scratch and with the LDS of the documented formula, the compile cache, the host-side validation, the
inverse Jacobians, and the ordered oracle (gradient_util.py) on fields whose gradient is known."""

import os
import re
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import _capi, gradient, jit

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini  # noqa: E402
from fenics_constitutive_amd.gradient import hex8_reference_gradients  # noqa: E402
from gradient_util import EPS, LAYOUTS, SHAPES, TET_P1_REFERENCE_GRADIENTS, cube_operator_tables, oracle, random_tables, rounding_bound  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def operator(shape, n_cells=3, affine=None, layout="nabla_grad", seed=0):
    affine = SHAPES[shape][3] if affine is None else affine
    du, dofmap, ref, jinv, n_nodes = random_tables(shape, n_cells, seed, False, affine)
    return fc.DisplacementGradient(dofmap, ref, jinv, n_nodes, layout=layout), (du, dofmap, ref, jinv, n_nodes)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_shape_compiles_without_scratch(shape):
    d_, a_, q_, natural = SHAPES[shape]
    for affine in (True, False):
        for layout in LAYOUTS:
            op, _ = operator(shape, affine=affine, layout=layout)
            r = op.resources
            assert r["scratch_bytes"] == 0, (shape, affine, layout, r)
            assert r["lds_bytes"] == gradient.lds_bytes(d_, a_, q_) == 8 * ((d_ * a_ * q_ + 1) // 2 * 2) + 4 * 64 * d_ * d_ * 8
            assert "fcamd_displacement_gradient_kernel" in op.compile_log
            assert (op.gdim, op.nodes_per_cell, op.points_per_cell, op.affine, op.layout) == (d_, a_, q_, affine, layout)
            assert (op.n_cells, op.n_points) == (3, 3 * q_)
    # no scratch at any register budget
    for waves in gradient.WAVES_LADDER:
        for affine in (True, False):
            code = gradient.compile_kernel(d_, a_, q_, affine, "nabla_grad", waves)
            assert code.resources["scratch_bytes"] == 0, (shape, affine, waves, code.resources)


def test_same_shape_compiles_once():
    operator("tet_p2", n_cells=2, seed=1)
    before = jit.compile_count()
    op, _ = operator("tet_p2", n_cells=7, seed=2)  # other tables, other mesh size: the same program
    assert jit.compile_count() == before
    operator("tet_p2", n_cells=2, layout="grad")  # another program (first time here or cached by an earlier test)
    assert op.resources["scratch_bytes"] == 0


def test_validation_errors():
    du, dofmap, ref, jinv, n_nodes = random_tables("tet_p2", 5, 3, False, True)
    ok = fc.DisplacementGradient(dofmap, ref, jinv, n_nodes)
    assert ok.n_nodes == n_nodes and ok.affine
    DG = fc.DisplacementGradient
    with pytest.raises(TypeError):
        DG(dofmap.astype(np.int64), ref, jinv, n_nodes)
    with pytest.raises(TypeError):
        DG(dofmap, ref.astype(np.float32), jinv, n_nodes)
    with pytest.raises(TypeError):
        DG(dofmap, ref, jinv.astype(np.float32), n_nodes)
    with pytest.raises(TypeError):
        DG(dofmap.tolist(), ref, jinv, n_nodes)
    with pytest.raises(TypeError):
        DG(dofmap, ref, jinv, float(n_nodes))
    with pytest.raises(ValueError):
        DG(dofmap.reshape(-1), ref, jinv, n_nodes)  # dofmap not 2-D
    with pytest.raises(ValueError):
        DG(dofmap, ref[:, :-1], jinv, n_nodes)  # nodes per cell differ
    with pytest.raises(ValueError):
        DG(dofmap, ref, jinv[:-1], n_nodes)  # one cell short
    with pytest.raises(ValueError):
        DG(dofmap, ref, jinv[:, :2], n_nodes)
    with pytest.raises(ValueError):
        DG(dofmap, np.zeros((4, 10, 4)), np.zeros((5, 4, 4)), n_nodes)  # dimension 4
    bad = dofmap.copy()
    bad[2, 1] = n_nodes
    with pytest.raises(ValueError, match="dofmap entries"):
        DG(bad, ref, jinv, n_nodes)
    bad[2, 1] = -1
    with pytest.raises(ValueError, match="dofmap entries"):
        DG(bad, ref, jinv, n_nodes)
    for k, value in ((1, np.nan), (2, np.inf)):
        tables = [dofmap, ref.copy(), jinv.copy()]
        tables[k].reshape(-1)[3] = value
        with pytest.raises(ValueError, match="non-finite"):
            DG(*tables, n_nodes)
    with pytest.raises(ValueError, match="layout"):
        DG(dofmap, ref, jinv, n_nodes, layout="transposed")


def test_table_over_the_lds_cap_is_refused():
    # D = 3: 18432 bytes of transposition regions, so 5888 doubles of table fit and 5889 (padded: 5890) do not
    assert gradient.lds_bytes(3, 64, 30) <= gradient.LDS_CAP < gradient.lds_bytes(3, 64, 31)
    before = jit.compile_count()
    dofmap = np.zeros((1, 64), dtype=np.int32)
    with pytest.raises(ValueError, match="LDS"):
        fc.DisplacementGradient(dofmap, np.zeros((31, 64, 3)), np.zeros((1, 3, 3)), 1)
    assert jit.compile_count() == before  # refused before anything is compiled


def test_inverse_jacobians_of_the_cube():
    mesh = fe_mini.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    assert jinv.shape == (mesh.n_cells, 8, 3, 3) and dofmap.shape == (mesh.n_cells, 8)
    dn = np.einsum("qak,cqkx->cqax", ref, jinv)
    # the rounding bound entry by entry: (A + D + 2) 2^-52 S, S = sum_k |ref[q][a][k]| |jinv[c][q][k][x]|
    bound = (8 + 3 + 2) * EPS * np.einsum("qak,cqkx->cqax", np.abs(ref), np.abs(jinv))
    assert (np.abs(dn - mesh.dN[None]) <= bound).all(), (np.abs(dn - mesh.dN[None]) / bound).max()
    x = mesh.nodes[mesh.cells]
    # the tabulation at one point: [C][D][D]
    one = gradient.inverse_jacobians(x, ref[:1])
    assert one.shape == (mesh.n_cells, 3, 3) and np.array_equal(one, jinv[:, 0])
    with pytest.raises(ValueError):
        gradient.inverse_jacobians(x, ref[:, :4])


def linear_field(nodes, rng):
    a, b = rng.normal(size=3), rng.normal(size=(3, 3))
    return (a[None, :] + nodes @ b.T).reshape(-1), b


def test_oracle_on_sheared_affine_tets():
    rng = np.random.default_rng(5)
    n_cells = 40
    corners = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    shear = np.eye(3)[None] + 0.3 * rng.normal(size=(n_cells, 3, 3))
    x = np.einsum("cxy,gy->cgx", shear, corners) + rng.normal(size=(n_cells, 1, 3))  # [c][g][x]
    nodes = x.reshape(-1, 3)
    dofmap = np.arange(4 * n_cells, dtype=np.int32).reshape(n_cells, 4)
    jinv = gradient.inverse_jacobians(x, TET_P1_REFERENCE_GRADIENTS)
    assert jinv.shape == (n_cells, 3, 3)
    u, b = linear_field(nodes, rng)
    got = oracle(u, dofmap, TET_P1_REFERENCE_GRADIENTS, jinv, "grad").reshape(n_cells, 3, 3)
    bound = rounding_bound(u, dofmap, TET_P1_REFERENCE_GRADIENTS, jinv, "grad").reshape(n_cells, 3, 3)
    assert (np.abs(got - b[None]) <= bound).all(), (np.abs(got - b[None]) / bound).max()
    # nabla_grad is the transpose
    assert np.array_equal(oracle(u, dofmap, TET_P1_REFERENCE_GRADIENTS, jinv, "nabla_grad").reshape(n_cells, 3, 3), got.transpose(0, 2, 1))


def test_oracle_on_distorted_hexahedra():
    rng = np.random.default_rng(6)
    mesh = fe_mini.Cube(3, 2, 4)
    h = 1.0 / np.array(mesh.shape)
    nodes = mesh.nodes + rng.uniform(-0.15, 0.15, size=mesh.nodes.shape) * h[None, :]
    ref = hex8_reference_gradients()
    dofmap = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    jinv = gradient.inverse_jacobians(nodes[mesh.cells], ref)
    jac = np.linalg.inv(jinv)
    cond = (np.linalg.norm(jac, 2, axis=(-2, -1)) * np.linalg.norm(jinv, 2, axis=(-2, -1))).max()
    u, b = linear_field(nodes, rng)
    got = oracle(u, dofmap, ref, jinv, "grad").reshape(-1, 3, 3)
    bound = cond * rounding_bound(u, dofmap, ref, jinv, "grad").reshape(-1, 3, 3)
    assert (np.abs(got - b[None]) <= bound).all(), (np.abs(got - b[None]) / bound).max()
    # and the mesh's own gradient operator on the undistorted box
    dofmap, ref, jinv = cube_operator_tables(mesh)
    u, _ = linear_field(mesh.nodes, rng)
    got = oracle(u, dofmap, ref, jinv, "grad")
    assert (np.abs(got - mesh.gradient(u)) <= rounding_bound(u, dofmap, ref, jinv, "grad")).all()


def test_flag_matches_the_header():
    with open(os.path.join(ROOT, "include", "fcamd.h")) as fh:
        m = re.search(r"#define FCAMD_EVAL_GRAD_ON_DEVICE (\d+)", fh.read())
    assert m and int(m.group(1)) == _capi.EVAL_GRAD_ON_DEVICE == 32
    assert "DisplacementGradient" in fc.__all__
