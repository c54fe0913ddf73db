"""The launch sequence of a solve, pinned for the four pairings of a Krylov solver with an operator: ConjugateGradient on a
TangentMatrix and on a TangentOperator, BiCGStab on the matrix, MatrixFreeBiCGStab on the operator.  The bit tests of the other
files compare every solve with the NumPy oracles; they cannot see a launch that does nothing, or one moved behind the end of a
solve.  Here every kernel a solve enqueues is recorded and compared with the sequence the module docstrings state:

* ``solver.py``: once per call the block inverses, the product of ``x0`` when there is one, the start (the update kernel in its
  start mode); per iteration product, update, direction.  With the multilevel preconditioner its setup stands where the inverse
  kernel stood, and its cycle and closing kernel follow the update kernel in the start and in every iteration.  On an operator a
  product is its element and node launch and block-Jacobi's blocks come from its diagonal-block kernels before the inverse kernel.
* ``bicgstab.py``: inverses (or the setup), ``K x0`` by the conjugate gradients' matrix-vector kernel, the start kernel; per iteration
  five launches -- product, half step, product, full step, direction -- and the multilevel cycle before either product (the closing
  kernel is not used).
* ``bicgstab_free.py``: the same around the operator's products: ``A x0`` by its element and node launch, per iteration seven
  launches -- element, node-dots, half step, element, node-dots, full step, direction.

The system is the symmetric one of test_bicgstab.py -- Cube(3, 2, 4), the tension constraints, the elastic tangent, its right-hand
side (180 dofs, one segment) --, on which every solver under every preconditioner runs its two iterations: ``rtol = 0``,
``maxiter = 2``, ``check_every = 1``, so three looks.  What the multilevel preconditioner launches is taken from the object itself: its
setup is the trace of a standalone ``pc.setup``, its cycle that of ``pc.apply`` less the setup; the diagonal-block launches are the
trace of ``A.diagonal_blocks``."""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fe_mini as FE  # noqa: E402
from cube_tension_device_solve import tension_constraints  # noqa: E402
from cube_tension_matrix_free import cube_operators  # noqa: E402

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import bicgstab, bicgstab_free, jit, multilevel, solver  # noqa: E402
from fenics_constitutive_amd import tangent_operator as to  # noqa: E402
from fenics_constitutive_amd.hostio import to_device  # noqa: E402
from bicgstab_util import elastic_mandel  # noqa: E402

KINDS = (None, "block_jacobi", "multilevel")
#: (solver class, on the operator)
PAIRINGS = {"cg_matrix": (fc.ConjugateGradient, False), "cg_operator": (fc.ConjugateGradient, True), "bicgstab": (fc.BiCGStab, False),
            "bicgstab_free": (fc.MatrixFreeBiCGStab, True)}


@pytest.fixture(scope="module")
def system():
    """the matrix, the operator, each one's first argument and multilevel preconditioner, the right-hand side and a start vector"""
    mesh = FE.Cube(3, 2, 4)
    _, f = cube_operators(mesh)
    mask, _ = tension_constraints(mesh)
    rng = np.random.default_rng(12)
    b = to_device(np.where(mask, 0.0, rng.normal(size=mesh.n_dofs)), "cuda")
    x0 = to_device(np.where(mask, 0.0, rng.normal(size=mesh.n_dofs)), "cuda")
    tangent = to_device(np.tile(elastic_mandel().reshape(-1), mesh.n_points), "cuda")
    k, a = fc.TangentMatrix(f), fc.TangentOperator(f)
    k.set_constrained(mask)
    a.set_constrained(mask)
    assert k.shape[0] == 180 and -(-k.shape[0] // solver.SEG) == 1
    sides = {False: (k, k(tangent), fc.MultilevelPreconditioner(k, coarsest_nodes=4)), True: (a, tangent, fc.MultilevelPreconditioner(a, coarsest_nodes=4))}
    torch.cuda.synchronize()
    return sides, b, x0


@pytest.fixture
def recorded(monkeypatch):
    """the names of the kernels launched, in order"""
    names = []
    real = jit.launch

    def launch(code, device, nblocks, args, what, kernel=None):
        names.append(kernel or code.kernel)
        return real(code, device, nblocks, args, what, kernel=kernel)

    monkeypatch.setattr(jit, "launch", launch)
    return names


def trace(recorded, call):
    del recorded[:]
    call()
    torch.cuda.synchronize()
    return list(recorded)


def expected(cls, on_operator, kind, has_x0, own_blocks, setup, cycle):
    """the kernels of a solve of two iterations, from the module docstrings"""
    product = [to.ELEMENT_KERNEL, to.NODE_KERNEL] if on_operator else [solver.MATVEC_KERNEL]
    inverses = {None: [], "block_jacobi": own_blocks + [solver.INVERSE_KERNEL], "multilevel": setup}[kind]
    cycle = cycle if kind == "multilevel" else []
    first = inverses + (product if has_x0 else [])
    if cls is fc.ConjugateGradient:
        close = cycle + [multilevel.CLOSE_KERNEL] if kind == "multilevel" else []
        start = first + [solver.UPDATE_KERNEL] + close
        iteration = product + [solver.UPDATE_KERNEL] + close + [solver.DIRECTION_KERNEL]
    else:
        dots = [to.ELEMENT_KERNEL, bicgstab_free.NODE_DOTS_KERNEL] if on_operator else [bicgstab.PRODUCT_KERNEL]
        start = first + [bicgstab.START_KERNEL]
        iteration = cycle + dots + [bicgstab.HALF_KERNEL] + cycle + dots + [bicgstab.FULL_KERNEL, bicgstab.DIRECTION_KERNEL]
    return start + 2 * iteration


@pytest.mark.parametrize("has_x0", [False, True], ids=["zero", "x0"])
@pytest.mark.parametrize("kind", KINDS, ids=["plain", "block_jacobi", "multilevel"])
@pytest.mark.parametrize("pairing", list(PAIRINGS))
def test_the_launch_sequence_of_a_solve(system, recorded, pairing, kind, has_x0):
    sides, b, x0 = system
    cls, on_operator = PAIRINGS[pairing]
    K, first, pc = sides[on_operator]
    own_blocks, setup, cycle = [], [], []
    if on_operator and kind == "block_jacobi":
        own_blocks = trace(recorded, lambda: K.diagonal_blocks(first))
        assert own_blocks and set(own_blocks) == {to.DIAGONAL_ELEMENT_KERNEL, to.DIAGONAL_NODE_KERNEL}
    if kind == "multilevel":
        setup = trace(recorded, lambda: pc.setup(first))
        applied = trace(recorded, lambda: pc.apply(first, b))
        assert setup and len(applied) > len(setup) and applied[:len(setup)] == setup
        cycle = applied[len(setup):]
        assert len(pc.levels) > 1 and setup[-1] == solver.INVERSE_KERNEL and multilevel.CLOSE_KERNEL not in applied
    s = cls(K, preconditioner=pc if kind == "multilevel" else kind, rtol=0.0, maxiter=2, check_every=1)
    del recorded[:]
    res = s(first, b, x0=x0 if has_x0 else None)
    assert (res.looks, res.iterations, res.status) == (3, 2, "maxiter")
    assert recorded == expected(cls, on_operator, kind, has_x0, own_blocks, setup, cycle)
