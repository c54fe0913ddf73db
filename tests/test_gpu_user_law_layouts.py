"""The kernel templates of user-defined laws over the layouts they can generate (userlaw_probe_util.py): history fields of every
width class, up to eight fields and 32 parameters, both tangent modes, every autodiff pass count, the grid-stride loop with the
ragged tile on a later trip, the lane mask of the non-converged count, rotated blocks in general position, and refused
(misaligned) calls.  Probe laws compute exact integers, so every comparison is on the bits; every output lives between canary
margins."""

import numpy as np
import pytest
from objective_rate_util import rotate_state
from userlaw_probe_util import (LAYOUTS, LOOP_SIZES, MODES, NARROW, ROTATED, SIZES, Probe, assert_exact, integer_inputs,
                                random_inputs, run_probe, same)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import jit, userlaw  # noqa: E402
from fenics_constitutive_amd import userlaw_sources as S  # noqa: E402
from fenics_constitutive_amd.hostio import to_device, to_host  # noqa: E402

FULL = fc.StressStrainConstraint.FULL
DEV = "cuda"
FORMS = ("ndarray", "in_place", "from")
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
RS_P = {"mu": np.array([80769.0]), "kappa": np.array([175000.0]), "y_0": np.array([1200.0]), "h": np.array([200.0])}
TOL_PL = 1e-6  # TOL["pl"] of test_gpu_user_law_autodiff.py
_laws = {}


def law(probe: Probe, extra=None):
    """one compiled law per probe (and ``extra``, what else decided the build) for the module"""
    key = (probe.key, extra)
    if key not in _laws:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # wide layouts spill: legal laws (test_user_law_layouts.py pins which)
            _laws[key] = probe.build(fc)
    return _laws[key]


def check(m, probe, n, form, tangent, inputs=None):
    """one guarded call against the reference: every word, the canaries, the non-converged count"""
    g, s0, h0 = inputs if inputs is not None else integer_inputs(probe, n)
    got = run_probe(m, probe, n, form, tangent, (g, s0, h0))
    ref = probe.reference(g, s0, h0)
    assert_exact(probe, got, ref, tangent)
    assert got[3] == int(ref[3].sum()), (got[3], int(ref[3].sum()))


@pytest.fixture
def one_cu(monkeypatch):
    """the launch capped at 512 blocks (userlaw looks ``num_cu`` up on jit at launch); yields the block counts of the launches"""
    blocks = []
    real = jit.launch

    def launch(code, device, nblocks, args, what):
        blocks.append(nblocks)
        return real(code, device, nblocks, args, what)

    monkeypatch.setattr(jit, "num_cu", lambda dev: 1)
    monkeypatch.setattr(jit, "launch", launch)
    return blocks


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the sweep: every layout, both modes, every size; all forms, with and without a tangent
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_sweep(layout, mode, n):
    fields, nparams = LAYOUTS[layout]
    probe = Probe(fields, nparams, mode)
    m = law(probe)
    for form in FORMS:
        for tangent in (True, False):
            check(m, probe, n, form, tangent)


def test_argument_block_sizes():
    """the ctypes mirror of UserArgs at the history counts the sweep runs: 4 pointers, 2 nh history pointers, the counter, n,
    three doubles, 32 parameters"""
    import ctypes

    for nh in (1, 2, 3, 4, 8):
        assert ctypes.sizeof(userlaw._args_type(nh)) == 8 * (4 + 2 * nh + 1 + 1 + 3 + 32)
    assert {max(1, len(f)) for f, _ in LAYOUTS.values()} >= {1, 2, 4, 8}


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the grid-stride loop: several trips per wave, the ragged tile on a later trip
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LOOP_SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["narrow", "wide4"])
def test_grid_stride_loop(layout, mode, n, one_cu):
    fields, nparams = LAYOUTS[layout]
    probe = Probe(fields, nparams, mode)
    m = law(probe)
    inputs = integer_inputs(probe, n)
    for form in ("in_place", "from"):
        for tangent in (True, False):
            check(m, probe, n, form, tangent, inputs)
    assert one_cu and all(b == 512 for b in one_cu), one_cu  # the launches really were capped: every wave made several trips


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the non-converged count when every lane returns non-zero: dead lanes of the ragged tile must not count
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 65, 257) + LOOP_SIZES)
@pytest.mark.parametrize("mode", MODES)
def test_count_is_exact_when_every_point_fails(mode, n, one_cu):
    probe = Probe(NARROW, 1, mode, rc="always")
    m = law(probe)
    inputs = integer_inputs(probe, n)
    for tangent in (True, False):  # autodiff: the tangent kernel and the stress-only kernel
        got = run_probe(m, probe, n, "in_place", tangent, inputs)
        assert got[3] == n, (got[3], n)
        assert_exact(probe, got, probe.reference(*inputs), tangent)
    if n >= LOOP_SIZES[0]:
        assert all(b == 512 for b in one_cu), one_cu


# ---------------------------------------------------------------------------------------------------------------------------
# 5. every pass count of the autodiff tangent kernel
# ---------------------------------------------------------------------------------------------------------------------------
KS = (6, 3, 2, 1)


def force_k(monkeypatch, k):
    monkeypatch.setattr(userlaw, "AD_LADDER", ((4, k), (3, k), (2, k)))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("layout", ["narrow", "wide4"])
def test_every_pass_count_of_the_probe(layout, k, monkeypatch, one_cu):
    force_k(monkeypatch, k)
    fields, nparams = LAYOUTS[layout]
    probe = Probe(fields, nparams, "autodiff")
    m = law(probe, extra=k)
    assert m.resources["directions_per_pass"] == k
    for n in (1, 63, 64, 65, 257, 4099, LOOP_SIZES[1]):
        inputs = integer_inputs(probe, n)
        for form in ("in_place", "from"):
            check(m, probe, n, form, True, inputs)
    assert one_cu[-1] == 512


@pytest.mark.parametrize("k", (3, 2, 1))
def test_every_pass_recomputes_the_first_pass(k, monkeypatch):
    """FCAMD_USER_AD_DEBUG (user_law_ad.hip): a later pass whose stress or return code differs from the first pass's counts the
    point as not converged, so the count stays the law's own"""
    force_k(monkeypatch, k)
    probe = Probe(NARROW, 1, "autodiff", debug=True)
    m = law(probe, extra=k)
    assert m.resources["directions_per_pass"] == k
    for n in (1, 65, 257, 4099):
        check(m, probe, n, "in_place", True)


SHIPPED = {"von_mises_3d_ad": (VM_P, {"eps_n": 6, "alpha": 1}, lambda: fc.VonMises3D(VM_P), TOL_PL),
           "spring_maxwell_ad": (SLS_P, {"strain_visco": 6, "strain": 6}, lambda: fc.SpringMaxwellModel(SLS_P, FULL), 1e-12)}


def rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("n", [65, 4099])
@pytest.mark.parametrize("name", list(SHIPPED))
def test_shipped_laws_at_every_pass_count(name, n, monkeypatch):
    """stress and history come from pass 0 whatever K is: bitwise equal across K.  The tangent of every K against the built-in
    law, at the tolerances of test_gpu_user_law_autodiff.py; across K it is bitwise equal too (each direction's partials see the
    same operations)"""
    p, hist, builtin, tol = SHIPPED[name]
    rng = np.random.default_rng(11)
    vm = name.startswith("von_mises")
    g = rng.normal(scale=3e-3 if vm else 1e-3, size=9 * n)
    s0 = (30.0 if vm else 1.0) * rng.normal(size=6 * n)
    h0 = {k: rng.normal(scale=1e-3, size=d * n) for k, d in hist.items()}
    if "alpha" in h0:
        h0["alpha"] = np.abs(h0["alpha"])

    def run(m):
        s, t, h = s0.copy(), np.full(36 * n, np.nan), {k: v.copy() for k, v in h0.items()}
        m.evaluate(0.0, 1.0, g, s, t, h)
        return s, t, h

    _, t_bi, _ = run(builtin())
    outs = {}
    for k in KS:
        force_k(monkeypatch, k)
        m = getattr(S, name)(p)
        assert m.resources["directions_per_pass"] == k
        outs[k] = run(m)
        assert rel_err(outs[k][1], t_bi) <= tol, (k, rel_err(outs[k][1], t_bi))
    if vm:
        assert np.count_nonzero(outs[6][2]["alpha"] != h0["alpha"]) > 0  # some points were plastic
    for k in KS[1:]:
        assert same(outs[k][0], outs[6][0]), k
        for f in hist:
            assert same(outs[k][2][f], outs[6][2][f]), (k, f)
        assert same(outs[k][1], outs[6][1]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rotated blocks in general position
# ---------------------------------------------------------------------------------------------------------------------------
def jaumann(probe, rot, fused):
    key = ("jaumann", probe.key, tuple(sorted((k, tuple(v)) for k, v in rot.items())), fused)
    if key not in _laws:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            j = fc.JaumannRate(law(probe), rot)
        j.fused = fused
        assert j.path == ("fused" if fused else "array")
        _laws[key] = j
    return _laws[key]


@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(ROTATED))
def test_rotated_blocks_in_general_position(case, mode, n):
    fields, rot = ROTATED[case]
    probe = Probe(fields, 1, mode)
    plain, fused, arr = law(probe), jaumann(probe, rot, True), jaumann(probe, rot, False)
    inputs = random_inputs(probe, n, seed=100 + n)
    g, s0, h0 = inputs
    sr, hr = rotate_state(g, s0, h0, rot)
    ref = probe.reference(g, sr, hr)
    outside = {name: np.ones(dim, dtype=bool) for name, dim in probe.dims}
    for name, offs in rot.items():
        for o in offs:
            outside[name][o:o + 6] = False
    for form in FORMS:
        a = run_probe(fused, probe, n, form, True, inputs)
        b = run_probe(arr, probe, n, form, True, inputs)
        u = run_probe(plain, probe, n, form, True, inputs)
        # fused == array-level, bit for bit; stress-only launches too
        assert_exact(probe, a, b)
        assert_exact(probe, run_probe(fused, probe, n, form, False, inputs), run_probe(arr, probe, n, form, False, inputs), False)
        assert a[3] == b[3] == u[3] == int(ref[3].sum())
        assert not same(a[0], u[0])  # the rotation did something
        # the NumPy rotation followed by the probe's reference
        assert rel_err(a[0], ref[0]) <= 1e-12 and rel_err(a[1], ref[1]) <= 1e-12
        for name, dim in probe.dims:
            assert rel_err(a[2][name], ref[2][name]) <= 1e-12, name
            # outside the rotated blocks: the unrotated probe's bits
            w = outside[name]
            assert same(a[2][name].reshape(n, dim)[:, w], u[2][name].reshape(n, dim)[:, w]), name
            if name in rot:
                assert not same(a[2][name], u[2][name]), name
        assert same(a[1], u[1])  # the probe's tangent does not depend on the committed state
    # a symmetric gradient has no spin: the unwrapped probe's bits everywhere
    sym = random_inputs(probe, n, seed=200 + n, symmetric=True)
    for form in FORMS:
        u = run_probe(plain, probe, n, form, True, sym)
        assert_exact(probe, run_probe(fused, probe, n, form, True, sym), u)
        assert_exact(probe, run_probe(arr, probe, n, form, True, sym), u)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. refused calls write nothing
# ---------------------------------------------------------------------------------------------------------------------------
class Buffers:
    """the tensors of one call on random inputs, each an 8-byte but not 16-byte aligned view when named in ``misaligned``"""

    def __init__(self, hist, n, misaligned, seed=5, out_of_place=False):
        rng = np.random.default_rng(seed)
        g = rng.normal(scale=0.02, size=(n, 3, 3))  # not symmetric: a finite spin
        self.host = {"grad": g.reshape(-1), "stress": rng.normal(scale=300.0, size=6 * n), "tangent": np.full(36 * n, np.nan)}
        for k, d in (hist or {}).items():
            self.host[k] = np.abs(rng.normal(scale=1e-3, size=d * n))
        self.dev = {}
        for k, v in self.host.items():
            big = to_device(np.concatenate([np.zeros(2 + (k in misaligned)), v]), DEV)
            self.dev[k] = big[2 + (k in misaligned):]
            assert self.dev[k].data_ptr() % 16 == (8 if k in misaligned else 0)
        self.hist = None if hist is None else {k: self.dev[k] for k in hist}
        self.out = {}
        if out_of_place:
            for k in ["stress"] + list(hist or {}):
                self.out[k] = torch.full_like(self.dev[k], float("nan")) if k not in misaligned else \
                    torch.full((self.dev[k].numel() + 1,), float("nan"), dtype=torch.float64, device=DEV)[1:]

    def unchanged(self):
        torch.cuda.synchronize()
        return all(same(to_host(self.dev[k]), v) for k, v in self.host.items()) and \
            all(bool(torch.isnan(v).all()) for v in self.out.values())


@pytest.mark.parametrize("which", ["grad", "stress", "tangent", "a"])
@pytest.mark.parametrize("mode", MODES)
def test_misaligned_tensor_is_refused_before_anything_is_written(mode, which):
    probe = Probe(NARROW, 1, mode)
    m = law(probe)
    n = 100
    hist = dict(probe.dims)
    b = Buffers(hist, n, {which})
    with pytest.raises(ValueError, match="16-byte aligned"):
        m.evaluate(3.0, 0.5, b.dev["grad"], b.dev["stress"], b.dev["tangent"], b.hist)
    assert b.unchanged()
    b = Buffers(hist, n, {which}, out_of_place=True)
    with pytest.raises(ValueError, match="16-byte aligned"):
        m.evaluate_from(3.0, 0.5, b.dev["grad"], b.dev["stress"], b.out["stress"], b.dev["tangent"], b.hist,
                        {k: b.out[k] for k in hist})
    assert b.unchanged()
    # the committed arrays aligned, an output misaligned
    b = Buffers(hist, n, set(), out_of_place=True)
    out = torch.full((6 * n + 1,), float("nan"), dtype=torch.float64, device=DEV)[1:]
    with pytest.raises(ValueError, match="16-byte aligned"):
        m.evaluate_from(3.0, 0.5, b.dev["grad"], b.dev["stress"], out, b.dev["tangent"], b.hist, {k: b.out[k] for k in hist})
    assert b.unchanged() and bool(torch.isnan(out).all())


def _array_path_cases():
    probe = Probe(NARROW, 1, "explicit")
    return {
        "kelvin": (lambda: fc.JaumannRate(fc.SpringKelvinModel(SLS_P, FULL)), {"strain_visco": 6, "strain": 6}, "strain"),
        "comfe_mises": (lambda: fc.JaumannRate(fc.MisesPlasticityLinearHardening3D(RS_P)), {"history": 7}, "history"),
        "user_law": (lambda: fc.JaumannRate(law(probe), {"a": [0]}), dict(probe.dims), "a"),
    }


@pytest.mark.parametrize("which", ["tangent", "history"])
@pytest.mark.parametrize("case", ["kelvin", "comfe_mises", "user_law"])
def test_refused_array_level_call_leaves_the_committed_state(case, which):
    """JaumannRate's array-level path rotates the committed state in place before the wrapped law runs; what the law will refuse
    is refused before that, with the law's own error"""
    make, hist, field = _array_path_cases()[case]
    j = make()
    j.fused = False
    assert j.path == "array"
    n = 100
    bad = "tangent" if which == "tangent" else field
    b = Buffers(hist, n, {bad})
    with pytest.raises(ValueError, match="16-byte aligned"):
        j.evaluate(0.0, 1.0, b.dev["grad"], b.dev["stress"], b.dev["tangent"], b.hist)
    assert b.unchanged()
    b = Buffers(hist, n, {bad}, out_of_place=True)
    with pytest.raises(ValueError, match="16-byte aligned"):
        j.evaluate_from(0.0, 1.0, b.dev["grad"], b.dev["stress"], b.out["stress"], b.dev["tangent"], b.hist,
                        {k: b.out[k] for k in hist})
    assert b.unchanged()
    # the same call with aligned tensors goes through and rotates
    b = Buffers(hist, n, set())
    j.evaluate(0.0, 1.0, b.dev["grad"], b.dev["stress"], b.dev["tangent"], b.hist)
    torch.cuda.synchronize()
    assert not same(to_host(b.dev["stress"]), b.host["stress"])


def test_wrapped_law_gives_the_same_error_as_unwrapped():
    """the error type and text of the array-level path are the wrapped law's own"""
    n = 100
    for make, hist, field in _array_path_cases().values():
        j = make()
        j.fused = False
        for bad in ("tangent", field):
            errs = []
            for m in (j.model, j):
                b = Buffers(hist, n, {bad})
                with pytest.raises(ValueError) as ei:
                    m.evaluate(0.0, 1.0, b.dev["grad"], b.dev["stress"], b.dev["tangent"], b.hist)
                errs.append(str(ei.value))
            assert errs[0] == errs[1], errs
