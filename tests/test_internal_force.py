"""The force operator without a GPU (fenics_constitutive_amd.force, csrc/jit/internal_force.hip): every shape compiles for gfx950
without scratch at every register budget and with the LDS of the documented formula, the compile cache, the host-side validation,
the node adjacency, the integration weights, and the ordered oracle (force_util.py) against fe_mini's assembly and on a constant
stress field over sheared tetrahedra."""

import os
import sys

import numpy as np
import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import force, gradient, jit

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
import fe_mini  # noqa: E402
from force_util import (chain_length, force_bound, force_oracle, kuhn_tets, max_valence, random_inputs, tangent_action_bound,  # noqa: E402
                        tangent_action_oracle)
from gradient_util import EPS, SHAPES, TET_P1_REFERENCE_GRADIENTS, cube_operator_tables, oracle, random_tables  # noqa: E402


def operators(shape, n_cells=3, affine=None, layout="nabla_grad", seed=0):
    affine = SHAPES[shape][3] if affine is None else affine
    t = random_inputs(shape, n_cells, seed, False, affine)
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"], layout=layout)
    return fc.InternalForce(op, t["weights"]), t


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_shape_compiles_without_scratch(shape):
    d_, a_, q_, _ = SHAPES[shape]
    want_lds = 8 * ((d_ * a_ * q_ + 1) // 2 * 2) + 4 * 64 * d_ * d_ * 8
    assert force.lds_bytes(d_, a_, q_) == want_lds
    for source in force.SOURCES:
        for affine in (True, False):
            for accumulate in (False, True):
                for waves in gradient.WAVES_LADDER:
                    code = force.compile_kernels(d_, a_, q_, affine, "nabla_grad", source, accumulate, waves)
                    for kernel, lds in ((force.ELEMENT_KERNEL, want_lds), (force.NODE_KERNEL, 0)):
                        r = force.kernel_resources(code.log, kernel)
                        assert r["scratch_bytes"] == 0, (shape, source, affine, accumulate, waves, kernel, r)
                        assert r["lds_bytes"] == lds, (shape, source, affine, accumulate, waves, kernel, r)
    # the other gradient layout of the tangent action; the operator keeps the first budget of the ladder
    for affine in (True, False):
        f, _ = operators(shape, affine=affine, layout="grad")
        r = f.resources
        assert r["scratch_bytes"] == 0 and r["tangent_action"]["scratch_bytes"] == 0 and r["node"]["scratch_bytes"] == 0
        assert r["lds_bytes"] == r["tangent_action"]["lds_bytes"] == f.lds_bytes() == want_lds
        assert r["waves_per_simd"] == gradient.WAVES_LADDER[0]
        assert force.ELEMENT_KERNEL in f.compile_log and force.NODE_KERNEL in f.compile_log
        assert (f.gdim, f.nodes_per_cell, f.points_per_cell, f.stress_dim) == (d_, a_, q_, {1: 1, 2: 4, 3: 6}[d_])
        assert (f.n_cells, f.n_points) == (3, 3 * q_)


@pytest.mark.parametrize("shape", [(1, 2, 33), (3, 4, 33)])
def test_one_odd_cell_per_tile_compiles_without_scratch(shape):
    """W = 1 with Q and D odd: no tile base stays on the 16-byte grid, the kernel takes its guarded 8-byte loads.  At 8 waves per
    SIMD such a cell needs more than 64 registers, so the operator keeps the first budget its registers fit"""
    d_, a_, q_ = shape
    assert force.cells_per_tile(d_, q_) == 1 and (q_ * d_ * d_) % 2 == 1
    for source in force.SOURCES:
        for affine in (True, False):
            code = force.compile_kernels(d_, a_, q_, affine, "nabla_grad", source)
            r = force.kernel_resources(code.log, force.ELEMENT_KERNEL)
            waves = int(code.waves)
            assert r["scratch_bytes"] == 0 and waves in gradient.WAVES_LADDER and r["vgprs"] <= 512 // waves, (shape, source, affine, r)


def test_cells_per_tile():
    # W = 64 // Q, one less where W * Q * D * D would be odd
    assert [force.cells_per_tile(*SHAPES[s][:3:2]) for s in ("hex8", "tet_p1", "tet_p2", "q5", "tri_p2", "interval")] == [8, 64, 16, 12, 21, 64]
    assert force.cells_per_tile(3, 3) == 20 and force.cells_per_tile(1, 3) == 20 and force.cells_per_tile(2, 3) == 21
    assert force.cells_per_tile(3, 64) == 1 and force.cells_per_tile(3, 33) == 1


def test_same_shape_compiles_once():
    operators("tet_p2", n_cells=2, seed=1)[0].resources  # (both forms)
    before = jit.compile_count()
    f, _ = operators("tet_p2", n_cells=7, seed=2)  # other tables, other mesh size: the same programs
    f.resources
    assert jit.compile_count() == before
    texts = {force.program(3, 10, 4, True, "nabla_grad", s, a, 8) for s in force.SOURCES for a in (False, True)}
    assert len(texts) == 4


def test_validation_errors():
    torch = pytest.importorskip("torch")
    f, t = operators("tet_p2", n_cells=5, seed=3)
    op, w = f.op, t["weights"]
    IF = fc.InternalForce
    with pytest.raises(TypeError):
        IF((t["dofmap"], t["ref"], t["jinv"]), w)  # not an operator
    with pytest.raises(TypeError):
        IF(op, w.tolist())
    with pytest.raises(TypeError):
        IF(op, w.astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        IF(op, w[:-1])
    with pytest.raises(ValueError, match="shape"):
        IF(op, w.reshape(-1))
    with pytest.raises(ValueError, match="shape"):
        IF(op, w.T.copy())
    for value in (np.nan, np.inf):
        bad = w.copy()
        bad[2, 1] = value
        with pytest.raises(ValueError, match="non-finite"):
            IF(op, bad)
    # calls: refused on the host, before any device is touched (this test runs without one)
    n, nd = f.n_points, 3 * f.n_nodes
    with pytest.raises(TypeError):
        f(t["stress"])  # an ndarray
    with pytest.raises(TypeError):
        f(torch.zeros(6 * n, dtype=torch.float32))
    with pytest.raises(ValueError, match="cuda"):
        f(torch.zeros(6 * n, dtype=torch.float64))  # on the host
    with pytest.raises(ValueError, match="accumulate"):
        f(torch.zeros(6 * n, dtype=torch.float64), accumulate=True)
    with pytest.raises(ValueError, match="accumulate"):
        f.tangent_action(torch.zeros(36 * n, dtype=torch.float64), torch.zeros(9 * n, dtype=torch.float64), accumulate=True)
    with pytest.raises(TypeError):
        f.tangent_action(t["tangent"], t["grad_v"])
    with pytest.raises(TypeError):
        f.tangent_action(torch.zeros(36 * n, dtype=torch.float32), torch.zeros(9 * n, dtype=torch.float64))
    with pytest.raises(ValueError, match="cuda"):
        f.tangent_action(torch.zeros(36 * n, dtype=torch.float64), torch.zeros(9 * n, dtype=torch.float64))
    assert not f._on and not f._fe and not op._on  # nothing was uploaded


def test_too_many_points_and_the_lds_cap_are_refused():
    dofmap = np.zeros((1, 4), dtype=np.int32)
    op = fc.DisplacementGradient(dofmap, np.zeros((65, 4, 3)), np.zeros((1, 3, 3)), 1)  # the producer takes Q = 65
    with pytest.raises(ValueError, match="at most 64"):
        fc.InternalForce(op, np.ones((1, 65)))
    fc.InternalForce(fc.DisplacementGradient(dofmap, np.zeros((64, 4, 3)), np.zeros((1, 3, 3)), 1), np.ones((1, 64)))
    # the producer's cap: 5888 doubles of table fit next to the regions of D = 3
    assert force.lds_bytes(3, 64, 30) <= force.LDS_CAP < force.lds_bytes(3, 64, 31)
    before = jit.compile_count()
    with pytest.raises(ValueError, match="LDS"):
        force.compile_kernels(3, 64, 31, True)
    assert jit.compile_count() == before  # refused before anything is compiled


def test_node_adjacency_of_the_cube():
    mesh = fe_mini.Cube(3, 2, 4)
    dofmap = np.ascontiguousarray(mesh.cells, dtype=np.int32)
    node_ptr, entries = force.node_adjacency(dofmap, mesh.n_nodes)
    assert node_ptr.dtype == np.int32 and entries.dtype == np.int32
    assert node_ptr.shape == (mesh.n_nodes + 1,) and node_ptr[0] == 0 and node_ptr[-1] == dofmap.size == entries.size
    assert np.array_equal(np.sort(entries), np.arange(dofmap.size))  # every (c, a) exactly once
    for v in range(mesh.n_nodes):
        mine = entries[node_ptr[v]: node_ptr[v + 1]]
        assert (dofmap.reshape(-1)[mine] == v).all()  # under its own node
        assert (np.diff(mine) > 0).all()  # ascending
    assert (np.diff(node_ptr) >= 1).all() and np.diff(node_ptr).max() == 8
    # a node no cell touches has an empty row
    ptr2, ent2 = force.node_adjacency(dofmap, mesh.n_nodes + 2)
    assert ptr2[-1] == ptr2[-2] == ptr2[-3] == dofmap.size and np.array_equal(ent2, entries)
    f = fc.InternalForce(fc.DisplacementGradient(*cube_operator_tables(mesh), mesh.n_nodes), np.full((mesh.n_cells, 8), mesh.w))
    assert np.array_equal(f.node_ptr, node_ptr) and np.array_equal(f.adjacency, entries)


def test_integration_weights_of_the_cube():
    mesh = fe_mini.Cube(3, 2, 4)
    ref = gradient.hex8_reference_gradients()
    x = mesh.nodes[mesh.cells]
    w = gradient.integration_weights(x, ref, np.ones(8))
    assert w.shape == (mesh.n_cells, 8) and w.dtype == np.float64
    # Bit equality with Cube.w cannot be reached: the Jacobian entries are rounded sums of 8 products with the Gauss points'
    # 1/sqrt(3) in them, so they are not exactly h/2, and the determinant rounds again.  Measured: at most 4.5 * 2^-52 * w.
    assert np.max(np.abs(w - mesh.w)) <= 5 * EPS * mesh.w, np.max(np.abs(w - mesh.w)) / (EPS * mesh.w)
    one = gradient.integration_weights(x, ref[:1], np.full(8, 0.5))  # the tabulation at one point: an affine mesh
    assert one.shape == (mesh.n_cells, 8) and np.array_equal(one, 0.5 * w[:, :1] * np.ones((1, 8)))
    with pytest.raises(ValueError):
        gradient.integration_weights(x, ref, np.ones(7))
    with pytest.raises(ValueError):
        gradient.integration_weights(x, ref[:, :4], np.ones(8))


def cube_case(seed):
    mesh = fe_mini.Cube(3, 2, 4)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    weights = gradient.integration_weights(mesh.nodes[mesh.cells], ref, np.ones(8))
    rng = np.random.default_rng(seed)
    return mesh, dofmap, ref, jinv, weights, rng


def test_oracle_against_the_cube_internal_force():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(7)
    stress = rng.normal(scale=100.0, size=6 * mesh.n_points)
    got = force_oracle(stress, dofmap, ref, jinv, weights, mesh.n_nodes)
    want = mesh.internal_force(stress)
    bound = force_bound(stress, dofmap, ref, jinv, weights, mesh.n_nodes)
    assert max_valence(dofmap, mesh.n_nodes) == 8 and chain_length(3, 8, 8) == 26
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()
    assert np.abs(want).max() > 0


def test_oracle_against_the_cube_stiffness():
    mesh, dofmap, ref, jinv, weights, rng = cube_case(8)
    c = rng.normal(scale=1e4, size=(mesh.n_points, 6, 6))
    c = (c + c.transpose(0, 2, 1)).reshape(-1)  # fe_mini's stiffness is that of any tangent; a symmetric one as in the issue's prototype
    v = rng.normal(scale=1e-3, size=mesh.n_dofs)
    for layout in ("nabla_grad", "grad"):
        grad_v = oracle(v, dofmap, ref, jinv, layout)
        got = tangent_action_oracle(c, grad_v, dofmap, ref, jinv, weights, mesh.n_nodes, layout)
        want = mesh.stiffness(c) @ v
        bound = tangent_action_bound(c, grad_v, dofmap, ref, jinv, weights, mesh.n_nodes, layout)
        assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()
    # an unsymmetric tangent: C[i][j] and C[j][i] are told apart
    cu = rng.normal(scale=1e4, size=(mesh.n_points, 6, 6))
    grad_v = oracle(v, dofmap, ref, jinv, "grad")
    a = tangent_action_oracle(cu.reshape(-1), grad_v, dofmap, ref, jinv, weights, mesh.n_nodes, "grad")
    b = tangent_action_oracle(cu.transpose(0, 2, 1).reshape(-1).copy(), grad_v, dofmap, ref, jinv, weights, mesh.n_nodes, "grad")
    want = mesh.stiffness(cu.reshape(-1)) @ v
    assert np.abs(a - want).max() <= 1e-12 * np.abs(want).max() < 1e-3 * np.abs(b - want).max()


def test_oracle_on_sheared_tets_under_constant_stress():
    shear = np.eye(3) + 0.3 * np.random.default_rng(5).normal(size=(3, 3))
    nodes, cells, interior = kuhn_tets(3, 2, 3, shear, jitter=0.2, seed=6)
    assert interior.size == 2 * 1 * 2 and cells.shape == (6 * 18, 4)
    x = nodes[cells]
    jinv = gradient.inverse_jacobians(x, TET_P1_REFERENCE_GRADIENTS)
    weights = gradient.integration_weights(x, TET_P1_REFERENCE_GRADIENTS, np.array([1.0 / 6.0]))
    assert jinv.shape == (cells.shape[0], 3, 3) and weights.shape == (cells.shape[0], 1)
    volume = abs(np.linalg.det(shear))
    assert abs(weights.sum() - volume) <= 1e-13 * volume  # the tetrahedra fill the sheared box
    sigma = np.array([3.0, -1.0, 2.0, 0.7, -0.4, 1.1])
    stress = np.tile(sigma, cells.shape[0])
    n_nodes = nodes.shape[0]
    got = force_oracle(stress, cells, TET_P1_REFERENCE_GRADIENTS, jinv, weights, n_nodes).reshape(-1, 3)
    bound = force_bound(stress, cells, TET_P1_REFERENCE_GRADIENTS, jinv, weights, n_nodes).reshape(-1, 3)
    # div sigma = 0: the contributions of the cells around an interior node cancel
    assert (np.abs(got[interior]) <= bound[interior]).all(), (np.abs(got[interior]) / bound[interior]).max()
    boundary = np.setdiff1d(np.arange(n_nodes), interior)
    assert np.abs(got[boundary]).max() > 1e3 * np.abs(got[interior]).max()
    # and the whole body is in equilibrium
    assert (np.abs(got.sum(axis=0)) <= bound.sum(axis=0)).all()
    # the same through the tangent action: C = sigma (x) e1 with a gradient whose strain is e1
    tangent = np.zeros((cells.shape[0], 6, 6))
    tangent[:, :, 0] = sigma
    grad_v = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0]), cells.shape[0])
    via = tangent_action_oracle(tangent.reshape(-1), grad_v, cells, TET_P1_REFERENCE_GRADIENTS, jinv, weights, n_nodes, "grad")
    assert np.array_equal(via.reshape(-1, 3), got)


def test_oracle_start_value_and_untouched_node():
    t = random_inputs("tri_p2", 9, 4, False, True)
    n_nodes = t["n_nodes"]
    assert not (t["dofmap"] == t["lonely"]).any() and t["dofmap"].min() == 0 and t["dofmap"].max() == n_nodes - 1
    args = (t["dofmap"], t["ref"], t["jinv"], t["weights"], n_nodes)
    f0 = force_oracle(t["stress"], *args)
    assert (f0.reshape(-1, 2)[t["lonely"]] == 0.0).all()
    start = np.random.default_rng(0).normal(size=2 * n_nodes)
    f1 = force_oracle(t["stress"], *args, start=start)
    assert np.array_equal(f1.reshape(-1, 2)[t["lonely"]], start.reshape(-1, 2)[t["lonely"]])
    assert np.abs(f1 - (start + f0)).max() <= 16 * EPS * (np.abs(start) + np.abs(f0)).max()
    assert "InternalForce" in fc.__all__
