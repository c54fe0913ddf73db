"""The harness the GPU tests of the finite-element operators and the device solvers share (test_gpu_displacement_gradient.py,
test_gpu_internal_force.py, test_gpu_tangent_matrix.py, test_gpu_tangent_operator.py, test_gpu_conjugate_gradient.py,
test_gpu_bicgstab*.py, test_gpu_multilevel*.py): the comparison ON THE BITS, the canary margins around every output a caller hands
in, the cap of one compute unit with its launch record, and a solve into a guarded output.

Nothing at module level imports torch, the package or the examples: the CPU tests take ``bits``, ``assert_same_bits`` and ``tables_of``
from here too.  The fixture is taken by name -- ``from fe_gpu_util import one_cu  # noqa: F401`` --, pytest finds it in the test
module's namespace.  The user-law and material-point tests (userlaw_probe_util.py) have a canary scheme of their own."""

import numpy as np
import pytest

MARGIN = 64  # doubles on either side of an output (a multiple of two: the output stays on the 16-byte grid)
CANARY = np.uint64(0x7FF8DEADBEEF0BAD)  # a NaN no arithmetic produces


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_bits(have, want, what):
    diff = bits(have).reshape(-1) != bits(want).reshape(-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} entries differ, first at {int(np.argmax(diff))}"


def guarded(nout, fill=None):
    """(buffer, view of nout doubles) with canary margins; the view canaries too, or ``fill``"""
    from fenics_constitutive_amd.hostio import to_device

    h = np.full(nout + 2 * MARGIN, CANARY, dtype=np.uint64).view(np.float64)
    if fill is not None:
        h[MARGIN: MARGIN + nout] = fill
    buf = to_device(h, "cuda")
    return buf, buf[MARGIN: MARGIN + nout]


def assert_margins_intact(buf, nout):
    from fenics_constitutive_amd.hostio import to_host

    h = bits(to_host(buf))
    assert (h[:MARGIN] == CANARY).all() and (h[MARGIN + nout:] == CANARY).all(), "a kernel wrote outside its output"


@pytest.fixture
def one_cu(monkeypatch):
    """the launches capped at the blocks of ONE compute unit (``num_cu`` is looked up on jit at launch); yields (kernel, blocks)"""
    from fenics_constitutive_amd import jit

    launches = []
    real = jit.launch

    def launch(code, device, nblocks, args, what, kernel=None):
        launches.append((kernel or code.kernel, nblocks))
        return real(code, device, nblocks, args, what, kernel=kernel)

    monkeypatch.setattr(jit, "num_cu", lambda dev: 1)
    monkeypatch.setattr(jit, "launch", launch)
    return launches


def solve_guarded(solver, first, b, x0=None):
    """``solver(first, b, x0=x0, out=...)`` into a guarded output: (the result, x on the host); ``first``, the values of a matrix or
    the tangent of an operator, is a device tensor or an ndarray"""
    import torch
    from fenics_constitutive_amd.hostio import to_device, to_host

    n = b.size
    buf, out = guarded(n)
    first = first if torch.is_tensor(first) else to_device(first, "cuda")
    res = solver(first, to_device(b, "cuda"), x0=None if x0 is None else to_device(x0, "cuda"), out=out)
    assert res.x.data_ptr() == out.data_ptr()
    assert_margins_intact(buf, n)
    return res, to_host(out)


def assert_same_result(res, x, want, what):
    assert_same_bits(x, want.x, what)
    assert (res.iterations, res.status, res.converged) == (want.iterations, want.status, want.converged), what
    assert bits(np.float64(res.residual_norm)) == bits(np.float64(want.residual_norm)), what
    assert bits(np.float64(res.rhs_norm)) == bits(np.float64(want.rhs_norm)), what


def tables_of(t):
    return t["dofmap"], t["ref"], t["jinv"], t["weights"], t["n_nodes"]


def force_of(t):
    import fenics_constitutive_amd as fc

    return fc.InternalForce(fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"]), t["weights"])


def status_of(pc):
    """the status the preconditioner's own control block holds behind setup() or apply()"""
    from fenics_constitutive_amd import solver

    control = pc._on[pc.device].control
    control.download(pc.device)
    return int(control.ints[solver._STATUS])


def cube_system_of(mesh, seed, scratch_bytes=None):
    """(force, tables, mask, operator, tangent): the tension-test operator of ``mesh`` on a random positive definite tangent; the
    caller has examples/ on ``sys.path``"""
    import fenics_constitutive_amd as fc
    from cube_tension_device_solve import tension_constraints
    from cube_tension_matrix_free import cube_operators
    from gradient_util import cube_operator_tables
    from solver_util import spd_tangent

    op, f = cube_operators(mesh)
    dofmap, ref, jinv = cube_operator_tables(mesh)
    tables = (dofmap, ref, jinv, f._weights, mesh.n_nodes)
    mask, _ = tension_constraints(mesh)
    a = fc.TangentOperator(f, scratch_bytes=scratch_bytes)
    a.set_constrained(mask)
    return f, tables, mask, a, spd_tangent(mesh.n_points, 6, seed, False)
