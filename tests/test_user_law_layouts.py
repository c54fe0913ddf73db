"""The probe laws of tests/test_gpu_user_law_layouts.py (userlaw_probe_util.py), the part that needs no GPU: every program of the
sweep, of the forced pass counts and of the rotated layouts compiles for gfx950, and the compiler's report is what the templates
promise: an LDS region that does not grow with the history, the forced pass count, no scratch for the narrow layouts.  Which
wide or many-field layouts spill is pinned as observed, so that a change of the templates that makes a narrow law spill, or a
wide one stop spilling, is seen."""

import warnings

import numpy as np
import pytest
from userlaw_probe_util import DEL_T, LAYOUTS, MODES, NARROW, ROTATED, T, Probe, integer_inputs, prod

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import userlaw

LDS_BYTES = 4 * 64 * 18 * 8  # four waves' regions of 64 points x 18 doubles (user_law_tile.h), whatever the history
#: observed: the layouts whose kernels use scratch at every register budget (both tangent modes, the stress-only kernel too).
#: The single-field layouts of 19 to 36 doubles do not: they fit 168 (19, 20, 23) or 256 (35, 36) VGPRs.
SPILLS = {"wide4", "eight"}
ROTATED_SPILLS = {"wide_25_13"}
KS = (6, 3, 2, 1)


def build(probe, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # the scratch warning of the spilling layouts
        return probe.build(fc, **kw)


def kernels(law):
    """the resource reports of the law's kernels: one in explicit mode, the tangent and the stress-only kernel in autodiff mode"""
    r = law.resources
    return [r] + ([r["stress_only"]] if "stress_only" in r else [])


def waves_of(dim: int, mode: str) -> int:
    """observed: the register budget a single-field layout lands on (waves per SIMD: 128 / 168 / 256 VGPRs)"""
    if dim <= 17 or (dim == 18 and mode == "explicit"):
        return 4
    return 3 if dim <= 23 else 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sweep_layouts_compile(layout, mode):
    fields, nparams = LAYOUTS[layout]
    probe = Probe(fields, nparams, mode)
    law = build(probe)
    for r in kernels(law):
        assert r["lds_bytes"] == LDS_BYTES, r
        assert bool(r["scratch_bytes"]) == (layout in SPILLS), r
    r = law.resources
    if len(fields) == 1:
        assert r["waves_per_simd"] == waves_of(prod(fields[0][1]), mode), r
    if mode == "autodiff":  # a layout that spills at every rung ends on the ladder's last: (2 waves, K = 1)
        assert r["directions_per_pass"] == (1 if layout in SPILLS else 6), r
    assert law._args_cls is not None and len(law._hist) == len(fields)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("layout", ["narrow", "wide4"])
def test_forced_pass_counts_compile(layout, k, monkeypatch):
    monkeypatch.setattr(userlaw, "AD_LADDER", ((4, k), (3, k), (2, k)))
    fields, nparams = LAYOUTS[layout]
    law = build(Probe(fields, nparams, "autodiff"))
    r = law.resources
    assert r["directions_per_pass"] == k
    for x in kernels(law):
        assert x["lds_bytes"] == LDS_BYTES, x
        assert bool(x["scratch_bytes"]) == (layout in SPILLS), x
    if k < 6 and layout == "narrow":
        dbg = build(Probe(NARROW, nparams, "autodiff", debug=True))
        assert dbg.resources["directions_per_pass"] == k and not dbg.resources["scratch_bytes"]
        assert dbg._compiled is not law._compiled  # the define reached the template


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(ROTATED))
def test_rotated_layouts_compile(case, mode):
    fields, rot = ROTATED[case]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        j = fc.JaumannRate(build(Probe(fields, 1, mode)), rot)
    assert j.path == "fused"
    for r in kernels(j._fused):
        assert r["lds_bytes"] == LDS_BYTES, r
        assert bool(r["scratch_bytes"]) == (case in ROTATED_SPILLS), r
    j.fused = False
    assert j.path == "array" and j.resources["scratch_bytes"] == 0 and j.resources["lds_bytes"] == 0


def test_reference_is_exact_integer_arithmetic():
    """the probe's NumPy reference on its integer inputs: every history and tangent word is an integer (the clock's words a
    multiple of 0.5) far below 2^53, so no operation of the law rounds; the 36 tangent entries of a point do not repeat (at more than nine points of ten)"""
    for mode in MODES:
        probe = Probe(LAYOUTS["eight"][0], 32, mode)
        n = 4099
        g, s0, h0 = integer_inputs(probe, n)
        s, D, h, rc = probe.reference(g, s0, h0)
        for name, v in h.items():
            assert np.array_equal(2.0 * v, np.round(2.0 * v)) and np.abs(v).max() < 2.0 ** 40, name
        assert np.array_equal(D, np.round(D)) and np.abs(D).max() < 2.0 ** 40
        assert np.mean([np.unique(row).size == 36 for row in D.reshape(n, 36)]) > 0.9  # (the product term collides at a few points)
        assert np.array_equal(h["clk"].reshape(n, 2) - h0["clk"].reshape(n, 2), np.tile([T, DEL_T], (n, 1)))
        assert np.unique(h["pvals"].reshape(n, 32)[0] - h0["pvals"].reshape(n, 32)[0]).size == 32
        assert 0 < rc.sum() < n and rc[0] and rc[-1]
        if mode == "explicit":
            assert np.array_equal(s, np.round(s))
