"""The harness of fe_gpu_util.py itself: what the comparison on the bits lets pass and what it reports (no GPU, no torch), and on the
GPU the canary margins, the cap of one compute unit with its launch record, and a solve into a guarded output -- each on a mesh of
two cells.  The writes that must be noticed land inside the guarded allocation."""

import ast
import inspect

import numpy as np
import pytest

import fe_gpu_util
from fe_gpu_util import CANARY, MARGIN, assert_margins_intact, assert_same_bits, bits, force_of, guarded, solve_guarded
from fe_gpu_util import one_cu  # noqa: F401 (the fixture: pytest finds it in this namespace)

QUIET_NAN = np.uint64(0x7FF8000000000000)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the comparison on the bits (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_module_level_imports_neither_torch_nor_the_package():
    tree = ast.parse(inspect.getsource(fe_gpu_util))
    imported = {a.name for node in tree.body if isinstance(node, ast.Import) for a in node.names}
    imported |= {node.module for node in tree.body if isinstance(node, ast.ImportFrom)}
    assert imported == {"numpy", "pytest"}


def test_same_bits_passes_on_equal_arrays():
    a = np.array([1.5, -0.0, 0.0, np.inf, -np.inf, 5e-324])
    assert_same_bits(a, a.copy(), "finite and infinite")
    nans = np.array([QUIET_NAN, QUIET_NAN | np.uint64(1), CANARY, QUIET_NAN | np.uint64(1 << 63)], dtype=np.uint64).view(np.float64)
    assert np.isnan(nans).all()
    assert_same_bits(nans, nans.copy(), "equal NaN payloads")
    assert_same_bits(a.reshape(2, 3), a, "both sides are flattened")
    assert_same_bits(np.stack([a, a])[:, ::2], np.stack([a[::2], a[::2]]), "a strided view")
    assert bits(np.float64(1.0)) == np.uint64(0x3FF0000000000000)


def test_same_bits_raises_on_the_sign_of_zero():
    assert 0.0 == -0.0
    with pytest.raises(AssertionError, match="zeros: 1 of 3 entries differ, first at 1"):
        assert_same_bits(np.array([1.0, 0.0, 2.0]), np.array([1.0, -0.0, 2.0]), "zeros")


def test_same_bits_raises_on_another_nan_payload():
    have = np.array([QUIET_NAN, CANARY], dtype=np.uint64).view(np.float64)
    want = np.array([QUIET_NAN, QUIET_NAN], dtype=np.uint64).view(np.float64)
    assert np.isnan(have).all() and np.isnan(want).all()
    with pytest.raises(AssertionError, match="payloads: 1 of 2 entries differ, first at 1"):
        assert_same_bits(have, want, "payloads")


def test_same_bits_reports_the_count_and_the_first_index():
    want = np.arange(12.0).reshape(3, 4)
    have = want.copy()
    have[1, 3] += 1.0
    have[2, 0] = np.nextafter(have[2, 0], np.inf)  # one unit in the last place
    have[2, 3] = -have[2, 3]
    with pytest.raises(AssertionError, match="the case at hand: 3 of 12 entries differ, first at 7"):
        assert_same_bits(have, want, "the case at hand")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the canary margins
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fill", [None, np.array([1.0, -0.0, 2.5, np.inf, -3.0])], ids=["canaries", "fill"])
def test_guarded_and_its_margins(fill):
    from fenics_constitutive_amd.hostio import to_host

    nout = 5
    buf, out = guarded(nout, fill=fill)
    assert buf.numel() == nout + 2 * MARGIN and out.numel() == nout and buf.is_cuda
    assert out.data_ptr() == buf.data_ptr() + 8 * MARGIN and out.data_ptr() % 16 == 0  # the view of the buffer, on the 16-byte grid
    h = bits(to_host(buf))
    assert (h[:MARGIN] == CANARY).all() and (h[MARGIN + nout:] == CANARY).all()
    if fill is None:
        assert (h[MARGIN: MARGIN + nout] == CANARY).all()
    else:
        assert_same_bits(h[MARGIN: MARGIN + nout].view(np.float64), fill, "the filled view")
    assert_margins_intact(buf, nout)
    out.fill_(7.0)  # a write of the whole view and nothing else
    assert_margins_intact(buf, nout)
    assert (to_host(out) == 7.0).all()
    for at in (MARGIN - 1, MARGIN + nout):  # one double in front of the view, one behind it: inside the allocation
        buf, out = guarded(nout, fill=fill)
        buf[at] = 7.0
        with pytest.raises(AssertionError, match="wrote outside its output"):
            assert_margins_intact(buf, nout)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the cap of one compute unit and a solve into a guarded output, on two cells
# ---------------------------------------------------------------------------------------------------------------------------------
def interval_tables():
    """two two-node cells of lengths 0.5 and 2 over three nodes (D = 1, one point per cell), one tangent modulus per point"""
    h = np.array([0.5, 2.0])
    return dict(dofmap=np.array([[0, 1], [1, 2]], dtype=np.int32), ref=np.array([[[-1.0], [1.0]]]), jinv=np.ascontiguousarray((1.0 / h)[:, None, None]),
                weights=h[:, None].copy(), n_nodes=3, tangent=np.array([3.0, 8.0]))


@pytest.mark.gpu
def test_one_cu_records_the_launch_and_caps_it(one_cu):
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd import gradient, jit
    from fenics_constitutive_amd.hostio import to_host

    assert one_cu == [] and jit.num_cu(0) == 1
    t = interval_tables()
    op = fc.DisplacementGradient(t["dofmap"], t["ref"], t["jinv"], t["n_nodes"])  # (launches without ``kernel``: the name is the code object's)
    buf, out = guarded(2)
    assert op(np.array([1.0, 2.0, 6.0]), out=out).data_ptr() == out.data_ptr()
    assert_margins_intact(buf, 2)
    assert_same_bits(to_host(out), np.array([2.0, 2.0]), "(2 - 1) / 0.5 and (6 - 2) / 2")
    (name, blocks), = one_cu
    assert name == gradient.KERNEL and 1 == blocks <= gradient.BLOCKS_PER_CU


@pytest.mark.gpu
def test_solve_guarded_returns_x_in_the_guarded_view():
    import fenics_constitutive_amd as fc
    from fenics_constitutive_amd.hostio import to_device, to_host

    t = interval_tables()
    a = fc.TangentOperator(force_of(t))
    mask = np.array([True, False, False])
    a.set_constrained(mask)
    b = np.array([0.0, 1.0, 2.0])
    stiffness = np.array([[1.0, 0.0, 0.0], [0.0, 3.0 / 0.5 + 8.0 / 2.0, -8.0 / 2.0], [0.0, -8.0 / 2.0, 8.0 / 2.0]])  # modulus / length per cell
    cg = fc.ConjugateGradient(a, rtol=1e-12)
    res, x = solve_guarded(cg, t["tangent"], b)  # the tangent as an ndarray
    assert res.converged and res.status == "converged" and 1 <= res.iterations <= 2
    assert res.x.numel() == 3 and res.x.storage_offset() == MARGIN and res.x.untyped_storage().nbytes() == 8 * (3 + 2 * MARGIN)
    assert_same_bits(to_host(res.x), x, "the second return value is x on the host")
    assert np.allclose(x, np.linalg.solve(stiffness, b), rtol=1e-10, atol=0.0)
    again, x_again = solve_guarded(cg, to_device(t["tangent"], "cuda"), b, x0=np.array([0.0, 0.25, -1.0]))  # as a device tensor, with a start vector
    assert again.converged and again.x.data_ptr() != res.x.data_ptr() and again.x.storage_offset() == MARGIN
    assert np.allclose(x_again, x, rtol=1e-10, atol=0.0)
