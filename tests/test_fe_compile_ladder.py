"""The register-budget ladder of the four finite-element operators, pinned without a GPU: ``gradient.compile_kernel``,
``force.compile_kernels``, ``matrix.compile_kernels`` and ``tangent_operator.compile_kernels``.

Every rung of ``gradient.WAVES_LADDER`` is compiled with an explicit ``waves=w``, the rule of the module's docstring is applied
here to the compiler's own remarks, and ``waves=None`` must return the code object of the rung the rule picks: the same cache key
(so the same program text), the same ``waves`` and ``slab``.  The rules, as the modules state them:

* gradient: the first budget whose kernel has no scratch; no register test; ``RuntimeError`` when every budget spills;
* force: the first budget at which neither kernel has scratch and the element kernel's ``vgprs <= 512 // w``; failing that the
  first budget without scratch whose registers overran it; ``RuntimeError`` when every budget spills;
* matrix: the first budget at which neither kernel has scratch and the element kernel's ``vgprs + agprs <= 512 // w``;
  ``ValueError`` otherwise, with the last budget's scratch in the message;
* tangent_operator: as the matrix, with none of its four kernels in scratch and the registers of the product's element kernel.

Because the rule is evaluated on the remarks of the compiler that is installed, nothing here depends on its version.  Exhaustion
is reached by doctoring the remarks (every kernel "spills", or every kernel "overruns" its registers): no real spilling kernel is
needed."""

import re
import types

import pytest

from fenics_constitutive_amd import force, gradient, jit, matrix
from fenics_constitutive_amd import tangent_operator as to

#: name -> (D, A, Q, affine); the last one's 33 points per cell need more than the 64 registers of 8 waves per SIMD
SHAPES = {"hex8": (3, 8, 8, False), "tet_p2": (3, 10, 4, True), "tri_p2": (2, 6, 3, True), "odd33_3d": (3, 4, 33, False)}
LADDER = gradient.WAVES_LADDER
MODULES = ("gradient", "force", "force_tangent", "matrix", "operator")


def registers(log, kernel, agprs):
    r = force.kernel_resources(log, kernel)
    return r["vgprs"] + ((r["agprs"] or 0) if agprs else 0)


class Spec:
    """one module's ladder: how to compile a budget, the program text of a budget, and the documented rule"""

    def __init__(self, module, shape):
        d_, a_, q_, affine = shape
        self.module = module
        if module == "gradient":
            self.name = f"displacement_gradient_{d_}d_{a_}n_{q_}q"
            self.compile = lambda w: gradient.compile_kernel(d_, a_, q_, affine, "nabla_grad", waves=w)
            self.program = lambda w: gradient.program(d_, a_, q_, affine, "nabla_grad", w)
            self.scratch_free, self.element, self.agprs, self.fallback, self.slab = (gradient.KERNEL,), None, False, False, None
            self.error = RuntimeError
            self.spilled = lambda s: f"{self.name}: the kernel uses {s[0]} bytes of scratch per lane at every register budget"
        elif module in ("force", "force_tangent"):
            source = "stress" if module == "force" else "tangent"
            self.name = f"internal_force_{d_}d_{a_}n_{q_}q_{source}"
            self.compile = lambda w: force.compile_kernels(d_, a_, q_, affine, "nabla_grad", source, False, waves=w)
            self.program = lambda w: force.program(d_, a_, q_, affine, "nabla_grad", source, False, w)
            self.scratch_free, self.element, self.agprs, self.fallback, self.slab = (force.ELEMENT_KERNEL, force.NODE_KERNEL), force.ELEMENT_KERNEL, False, True, None
            self.error = RuntimeError
            self.spilled = lambda s: f"{self.name}: the kernels use {s} bytes of scratch per lane at every register budget"
        elif module == "matrix":
            self.name = f"tangent_matrix_{d_}d_{a_}n_{q_}q"
            self.slab = matrix.slab_points(d_, a_, q_, affine)
            self.compile = lambda w: matrix.compile_kernels(d_, a_, q_, affine, waves=w)
            self.program = lambda w: matrix.program(d_, a_, q_, affine, self.slab, w)
            self.scratch_free, self.element, self.agprs, self.fallback = (matrix.ELEMENT_KERNEL, matrix.GATHER_KERNEL), matrix.ELEMENT_KERNEL, True, False
            self.error = ValueError
            self.spilled = lambda s: (f"{self.name}: the element matrix of {d_ * a_} columns does not compile without scratch at any register budget "
                                      f"(last: {s} bytes per lane)")
        else:
            self.name = f"tangent_operator_{d_}d_{a_}n_{q_}q"
            self.slab = to.diagonal_slab(d_, a_, affine)
            self.compile = lambda w: to.compile_kernels(d_, a_, q_, affine, waves=w)
            self.program = lambda w: to.program(d_, a_, q_, affine, self.slab, w)
            self.scratch_free, self.element, self.agprs, self.fallback = to.KERNELS, to.ELEMENT_KERNEL, True, False
            self.error = ValueError
            self.spilled = lambda s: f"{self.name}: the kernels do not compile without scratch at any register budget (last: {s} bytes per lane)"

    def scratch(self, code):
        return [force.kernel_resources(code.log, k)["scratch_bytes"] for k in self.scratch_free]

    def rule(self, rungs):
        """the budget the documented rule keeps among ``rungs`` = {w: code}; ``None``: the ladder is exhausted"""
        fallback = None
        for w in LADDER:
            if any(self.scratch(rungs[w])):
                continue
            if self.element is None or registers(rungs[w].log, self.element, self.agprs) <= 512 // w:
                return w
            if self.fallback and fallback is None:
                fallback = w
        return fallback


@pytest.mark.parametrize("module", MODULES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_ladder_keeps_the_budget_of_the_documented_rule(shape, module):
    spec = Spec(module, SHAPES[shape])
    rungs = {w: spec.compile(w) for w in LADDER}
    for w, code in rungs.items():
        assert code.key == jit.cache_key(spec.program(w)), (shape, module, w)  # the program text of the module's own program()
        print(f"{shape} {module} waves={w}: scratch {spec.scratch(code)}"
              + ("" if spec.element is None else f", registers {registers(code.log, spec.element, spec.agprs)} of {512 // w}"))
    assert len({code.key for code in rungs.values()}) == len(LADDER)
    want = spec.rule(rungs)
    assert want is not None, f"{shape} {module}: no budget passes on this compiler"
    kept = spec.compile(None)
    assert kept.key == rungs[want].key and kept is rungs[want], (shape, module, want)
    if module == "gradient":
        assert kept.resources == rungs[want].resources and not kept.resources["scratch_bytes"]
    else:
        assert kept.waves == want
    if spec.slab is not None:
        assert kept.slab == spec.slab
    for w, code in rungs.items():  # an explicit budget is marked as the ladder's is
        assert module == "gradient" or code.waves == w
        assert spec.slab is None or code.slab == spec.slab


def test_a_shape_overruns_a_budget_without_scratch():
    """the ladder's register test is not idle on the shapes above: 33 points per cell overrun the first budget in every module
    that has the test, and none of them spills there"""
    overran = []
    for module in MODULES[1:]:
        spec = Spec(module, SHAPES["odd33_3d"])
        code = spec.compile(LADDER[0])
        if not any(spec.scratch(code)) and registers(code.log, spec.element, spec.agprs) > 512 // LADDER[0]:
            overran.append(module)
            assert spec.compile(None).waves != LADDER[0]
    assert overran, "no module's element kernel overruns the first budget at 33 points per cell"


def doctored(monkeypatch, pattern, value):
    """every compile returns a stand-in whose remarks have ``value`` wherever ``pattern`` (one group: the text before the number)
    matches"""
    real = jit.compile_program

    def compile_program(program, name, kernel):
        code = real(program, name, kernel)
        log = re.sub(pattern + r"\d+", lambda m: m.group(1) + str(value), code.log)
        return types.SimpleNamespace(log=log, resources=jit.parse_resources(log), key=code.key, kernel=code.kernel, name=name)

    monkeypatch.setattr(jit, "compile_program", compile_program)


@pytest.mark.parametrize("module", MODULES)
def test_every_budget_spills(monkeypatch, module):
    spec = Spec(module, SHAPES["tri_p2"])
    doctored(monkeypatch, r"(ScratchSize \[bytes/lane\]:\s*)", 64)
    with pytest.raises(spec.error) as e:
        spec.compile(None)
    assert type(e.value) is spec.error and str(e.value) == spec.spilled([64] * len(spec.scratch_free))
    for w in LADDER:  # an explicit budget is returned unchecked
        code = spec.compile(w)
        assert code.key == jit.cache_key(spec.program(w)) and spec.scratch(code) == [64] * len(spec.scratch_free)
        assert module == "gradient" or code.waves == w


@pytest.mark.parametrize("module", MODULES)
def test_every_budget_overruns_its_registers(monkeypatch, module):
    """no scratch, 512 vector registers at every budget: the gradient has no register test and the force keeps the first budget
    (its fallback); the matrix and the operator refuse the shape, with the last budget's zeros in the message"""
    spec = Spec(module, SHAPES["tri_p2"])
    doctored(monkeypatch, r"(\bVGPRs:\s*)", 512)
    if module in ("matrix", "operator"):
        with pytest.raises(ValueError) as e:
            spec.compile(None)
        assert type(e.value) is ValueError and str(e.value) == spec.spilled([0] * len(spec.scratch_free))
    else:
        code = spec.compile(None)
        assert code.key == jit.cache_key(spec.program(LADDER[0]))
        assert module == "gradient" or code.waves == LADDER[0]
