"""User laws in autodiff mode (UserLaw(..., tangent="autodiff")), the parts that need no GPU: the four autodiff laws of
userlaw_sources compile for gfx950 without scratch, the resource report, the keyword's validation, compile errors and the
compile cache keys of both modes."""

import hashlib
import os

import pytest

import fenics_constitutive_amd as fc
from fenics_constitutive_amd import jit, userlaw, userlaw_sources as S

LE_P = {"E": 42.0, "nu": 0.3}
SLS_P = {"E0": 42.0, "E1": 10.0, "tau": 10.0, "nu": 0.2}
VM_P = {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0}
SWIFT_P = {"p_ka": 175000.0, "p_mu": 80769.0, "K": 1500.0, "eps0": 1e-3, "m": 0.2}

ZERO_AD = r"""
template <class T>
__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6], UserHistoryT<T>& h) {
    return 0;
}
"""


@pytest.mark.parametrize("make,p", [(S.linear_elasticity_ad, LE_P), (S.spring_maxwell_ad, SLS_P), (S.von_mises_3d_ad, VM_P),
                                    (S.von_mises_swift_ad, SWIFT_P)], ids=["le", "maxwell", "von_mises_3d", "swift"])
def test_autodiff_laws_compile_without_scratch(make, p):
    law = make(p)
    r = law.resources
    assert law.tangent_mode == "autodiff"
    assert r["scratch_bytes"] == 0 and r["stress_only"]["scratch_bytes"] == 0, r
    assert r["directions_per_pass"] in (1, 2, 3, 6), r
    assert r["waves_per_simd"] in userlaw.WAVES_PER_SIMD and r["vgprs"] is not None, r
    assert isinstance(law, fc.IncrSmallStrainModel) and law.stress_strain_dim == 6


def test_le_autodiff_runs_at_four_waves():
    r = S.linear_elasticity_ad(LE_P).resources
    assert r["waves_per_simd"] == 4 and r["vgprs"] <= 128 and r["directions_per_pass"] == 6, r
    assert r["stress_only"]["waves_per_simd"] == 4, r


def test_explicit_resources_have_no_directions():
    r = S.linear_elasticity(LE_P).resources
    assert "directions_per_pass" not in r and "stress_only" not in r


@pytest.mark.parametrize("mode", ["Autodiff", "forward", "", None, 1])
def test_bad_tangent_mode_raises_value_error(mode):
    with pytest.raises(ValueError, match="tangent"):
        fc.UserLaw(ZERO_AD, {"k": 1.0}, None, tangent=mode)


def test_missing_user_stress_raises_compile_error():
    src = ZERO_AD.replace("fcamd_user_stress", "my_stress_update")
    with pytest.raises(fc.UserLawCompileError) as ei:
        fc.UserLaw(src, {"k": 1.0}, None, name="no_stress_fn", tangent="autodiff")
    assert "fcamd_user_stress" in str(ei.value) and "no_stress_fn" in str(ei.value)


def test_autodiff_compile_error_carries_the_source_line():
    bad = ZERO_AD.replace("return 0;", "T x = ;  // the offending line\n    return 0;")
    with pytest.raises(fc.UserLawCompileError) as ei:
        fc.UserLaw(bad, {"k": 1.0}, None, name="broken_ad_law", tangent="autodiff")
    assert "T x = ;" in str(ei.value) and "error" in ei.value.log


def test_explicit_source_in_autodiff_mode_does_not_compile():
    with pytest.raises(fc.UserLawCompileError, match="fcamd_user_stress"):
        fc.UserLaw(S.LINEAR_ELASTICITY, LE_P, None, tangent="autodiff")


def test_modes_do_not_share_cache_entries():
    ex = S.linear_elasticity(LE_P)
    ad = S.linear_elasticity_ad(LE_P)
    keys_ad = {ad._compiled.key, ad._compiled_stress.key}
    assert ex._compiled.key not in keys_ad and len(keys_ad) == 2
    assert ex._compiled is ex._compiled_stress
    # the same parameters again: cache hits, no compile
    n = userlaw.compile_count()
    ad2 = S.linear_elasticity_ad({"E": 7.0, "nu": 0.25})
    assert userlaw.compile_count() == n and ad2._compiled is ad._compiled


def test_cache_key_is_the_hash_of_the_include_closure():
    """the key of either mode, recomputed from the program and the files it includes (found by following the #include lines);
    the closure reaches the library headers that user_law_api.h and tile_io.h include"""

    def read(path):
        with open(path) as fh:
            return fh.read()

    csrc = os.path.dirname(jit.JIT_DIR)
    common = {"jit/user_law_api.h", "jit/user_law_tile.h", "kernels/tile_io.h", "kernels/param_source.h", "fcamd_internal.h"}
    ex, ad = S.linear_elasticity(LE_P), S.linear_elasticity_ad(LE_P)
    for law, program, own in [(ex, ex._program(ex.source, 4), {"jit/user_law.hip"}),
                              (ad, ad._program_ad(ad.source, 4, 6), {"jit/user_law_ad.h", "jit/user_law_ad.hip"})]:
        files = jit.include_closure(program)
        assert {os.path.relpath(f, csrc) for f in files} == common | own
        h = hashlib.sha256()
        for part in (program, " ".join(jit.OPTIONS), jit.rtc_version(), *jit._STUB_HEADERS.values(), *map(read, files)):
            h.update(part.encode() + b"\0")
        assert law._compiled.key == h.hexdigest()
    assert "user_law_ad" not in ex._program(ex.source, 4)


def test_autodiff_program_text():
    law = fc.UserLaw(ZERO_AD, {"k": 1.0}, {"F": (3, 3), "alpha": 1}, name="ad_text", tangent="autodiff")
    prog = law._program_ad(ZERO_AD, 4, 3)
    assert "template <class T> struct UserHistoryT { T F[9]; T alpha[1]; };" in prog
    assert "#define FCAMD_USER_AD_K 3" in prog and prog.rstrip().endswith('#include "user_law_ad.hip"')


def test_refused_forms_in_autodiff_mode_need_no_gpu():
    law = S.linear_elasticity_ad(LE_P)
    with pytest.raises(NotImplementedError):
        law.use_devices([0, 1])
    with pytest.raises(NotImplementedError):
        law.evaluate_indexed(0.0, 1.0, None, None, None, None, None, None, None)
    with pytest.raises(NotImplementedError):
        fc.UserLaw(ZERO_AD, {"k": [1.0, 2.0]}, None, tangent="autodiff")
    for c in fc.StressStrainConstraint:
        if c.name != "FULL":
            with pytest.raises(NotImplementedError):
                fc.UserLaw(ZERO_AD, {"k": 1.0}, None, constraint=c, tangent="autodiff")
    from fenics_constitutive_amd.resident import ResidentState

    with pytest.raises(NotImplementedError):
        ResidentState(law, 64)
