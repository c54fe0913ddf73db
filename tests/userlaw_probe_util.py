"""Probe laws for the kernel templates of user-defined laws (csrc/jit/user_law.hip, user_law_ad.hip, user_law_tile.h): generated
HIP sources whose every output word is an exact function, in float64, of integer inputs that encode the array, point and
component they came from, the NumPy references of those sources, and output buffers with canary margins.

A layout is a list of ``(field name, dim)`` and a parameter count.  Two field names are special: ``clk`` (2 doubles: records
``t`` and ``del_t``) and ``pvals`` (32 doubles: records ``p.p0 .. p.p31``).  Every other field adds a constant that is distinct
per (field, component) and, with parameters, one parameter chosen by (field, component).  The comparison with the reference is
on the bits; there is no tolerance to choose."""

import numpy as np

FACTOR_PY = float.fromhex("0x1.6a09e667f3bccp-1")  # userlaw.FACTOR_PY: the off-diagonal Mandel factor
T, DEL_T = 3.0, 0.5  # the scalars every probe call passes: distinct, non-zero, exact when added to an integer
RC_LIMIT = 2.5  # a point does not converge when eps[3] = FACTOR_PY (g1 + g3) exceeds it: g1 + g3 is 2 (converged) or 4
CANARY = 0x7FF8C0DE00000000  # quiet NaN with a payload; the word index is added
NAN_FILL = 0x7FF8F111F111F111  # the pre-fill of outputs (another NaN payload)
MARGIN_ROWS = 64

#: autodiff mode: sigma_i += sum_j M[i][j] eps_j + Q[i] eps_0 eps_1 eps_2; the 36 entries of M are distinct
M = np.array([[7.0 * (6 * i + j) + 1.0 for j in range(6)] for i in range(6)])
Q = np.array([float(i + 1) for i in range(6)])


def prod(dim) -> int:
    return int(np.prod(dim)) if isinstance(dim, tuple) else int(dim)


def param_values(nparams: int) -> dict:
    """p0 .. p{n-1}: distinct integers"""
    return {f"p{j}": float(4096 * (j + 1) + j) for j in range(nparams)}


def field_constant(k: int, i: int) -> float:
    return float(1000 * (k + 1) + i)


def field_param(k: int, i: int, nparams: int):
    """index of the parameter that component i of field k adds, or None"""
    return (3 * k + i) % nparams if nparams else None


class Probe:
    """one probe layout: ``fields`` [(name, dim)], ``nparams`` parameters, ``mode`` "explicit" / "autodiff", ``rc`` "flag" (the
    point's gradient decides) or "always" (every point returns non-zero)"""

    def __init__(self, fields, nparams=0, mode="explicit", rc="flag", debug=False):
        self.fields = [(n, d) for n, d in fields]
        self.dims = [(n, prod(d)) for n, d in self.fields]
        self.nparams = int(nparams)
        self.mode = mode
        self.rc = rc
        self.debug = debug
        if any(n == "pvals" for n, _ in self.fields):
            assert self.nparams == 32 and dict(self.dims)["pvals"] == 32
        if any(n == "clk" for n, _ in self.fields):
            assert dict(self.dims)["clk"] == 2

    @property
    def key(self):
        return (tuple(self.fields), self.nparams, self.mode, self.rc, self.debug)

    @property
    def name(self) -> str:
        return "probe_" + "_".join(f"{n}{d}" for n, d in self.dims) + f"_p{self.nparams}_{self.mode[:2]}_{self.rc}"

    @property
    def parameters(self) -> dict:
        return param_values(self.nparams)

    @property
    def history_dim(self):
        return dict(self.fields) if self.fields else None

    # -- the HIP source ---------------------------------------------------------------------------------------------------
    def _history_lines(self) -> list:
        lines = []
        for k, (name, dim) in enumerate(self.dims):
            for i in range(dim):
                if name == "clk":
                    add = "t" if i == 0 else "del_t"
                elif name == "pvals":
                    add = f"p.p{i}"
                else:
                    j = field_param(k, i, self.nparams)
                    add = f"{field_constant(k, i)!r}" + ("" if j is None else f" + p.p{j}")
                lines.append(f"    h.{name}[{i}] = h.{name}[{i}] + ({add});")
        return lines

    def source(self) -> str:
        value = "eps[3]" if self.mode == "explicit" else "fcamd_value(eps[3])"
        rc = "1" if self.rc == "always" else f"({value} > {RC_LIMIT!r} ? 1 : 0)"
        head = "#define FCAMD_USER_AD_DEBUG\n" if self.debug else ""
        if self.mode == "explicit":
            body = ["__device__ int fcamd_user_point(const UserParams& p, double t, double del_t, const double (&grad)[9],",
                    "                                const double (&eps)[6], double (&sigma)[6], double (&D)[36], UserHistory& h) {"]
            body += self._history_lines()
            body += [f"    sigma[{i}] = sigma[{i}] + ({i + 1}.0 * grad[0] + {i + 2}.0 * grad[4] + {i + 3}.0 * grad[8]);" for i in range(6)]
            body += ["    for (int k = 0; k < 36; ++k) D[k] = 64.0 * grad[0] + (double)k;", f"    return {rc};", "}"]
        else:
            body = ["template <class T>",
                    "__device__ int fcamd_user_stress(const UserParams& p, double t, double del_t, const T (&eps)[6], T (&sigma)[6],",
                    "                                 UserHistoryT<T>& h) {"]
            body += self._history_lines()
            body.append("    const T prod = (eps[0] * eps[1]) * eps[2];")
            for i in range(6):
                body.append(f"    {{ T acc = {float(M[i, 0])!r} * eps[0];")
                body += [f"      acc = acc + {float(M[i, j])!r} * eps[{j}];" for j in range(1, 6)]
                body.append(f"      acc = acc + {float(Q[i])!r} * prod;")
                body.append(f"      sigma[{i}] = sigma[{i}] + acc; }}")
            body += [f"    return {rc};", "}"]
        return head + "\n".join(body) + "\n"

    def build(self, fc, **kw):
        return fc.UserLaw(self.source(), self.parameters, self.history_dim, name=self.name, tangent=self.mode, **kw)

    # -- the NumPy reference ------------------------------------------------------------------------------------------------
    def reference(self, grad, stress, hist, t=T, del_t=DEL_T):
        """(stress, tangent, history, return codes) of one call on the committed ``stress`` [6 n] and ``hist`` {name: [dim n]}:
        the law's operations in the law's order, one IEEE operation each"""
        n = grad.size // 9
        g = grad.reshape(n, 9)
        s = stress.reshape(n, 6)
        p = self.parameters
        out_h = {}
        for k, (name, dim) in enumerate(self.dims):
            add = np.empty(dim)
            for i in range(dim):
                if name == "clk":
                    add[i] = t if i == 0 else del_t
                elif name == "pvals":
                    add[i] = p[f"p{i}"]
                else:
                    j = field_param(k, i, self.nparams)
                    add[i] = field_constant(k, i) + (0.0 if j is None else p[f"p{j}"])
            out_h[name] = (hist[name].reshape(n, dim) + add[None, :]).reshape(-1)
        eps = np.stack([g[:, 0], g[:, 4], g[:, 8], FACTOR_PY * (g[:, 1] + g[:, 3]), FACTOR_PY * (g[:, 2] + g[:, 6]),
                        FACTOR_PY * (g[:, 5] + g[:, 7])], axis=1)
        out_s = np.empty((n, 6))
        D = np.empty((n, 36))
        if self.mode == "explicit":
            for i in range(6):
                out_s[:, i] = s[:, i] + (((i + 1.0) * g[:, 0] + (i + 2.0) * g[:, 4]) + (i + 3.0) * g[:, 8])
            D[:] = 64.0 * g[:, 0:1] + np.arange(36.0)[None, :]
        else:
            pr = (eps[:, 0] * eps[:, 1]) * eps[:, 2]
            dpr = np.stack([eps[:, 1] * eps[:, 2], eps[:, 0] * eps[:, 2], eps[:, 0] * eps[:, 1]], axis=1)
            Dv = np.tile(M.reshape(1, 6, 6), (n, 1, 1))
            for i in range(6):
                acc = M[i, 0] * eps[:, 0]
                for j in range(1, 6):
                    acc = acc + M[i, j] * eps[:, j]
                acc = acc + Q[i] * pr
                out_s[:, i] = s[:, i] + acc
                Dv[:, i, :3] += Q[i] * dpr
            D[:] = Dv.reshape(n, 36)
        rc = np.ones(n, dtype=bool) if self.rc == "always" else eps[:, 3] > RC_LIMIT
        return out_s.reshape(-1), D.reshape(-1), out_h, rc


# -- inputs -----------------------------------------------------------------------------------------------------------------
def integer_inputs(probe: Probe, n: int):
    """gradient, committed stress and history of n points as small integers that say where they came from (array id, point,
    component), all below 2^24: array a holds 65536 a + point * dim + i.  The gradient's diagonal carries the point; its
    off-diagonal pairs sum to small integers, and g1 + g3 is 4 at the points that are not to converge (about a third, the first
    and the last among them)"""
    pt = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(1000 + n)
    flag = rng.random(n) < 0.3
    flag[0] = flag[-1] = True
    if n > 2:
        flag[n // 2] = False
    g = np.zeros((n, 9))
    g[:, 0], g[:, 4], g[:, 8] = pt, pt % 1021 + 1, pt % 13 + 1
    g[:, 1], g[:, 3] = 1.0 + 2.0 * flag, 1.0
    g[:, 2], g[:, 6] = 2.0, 1.0
    g[:, 5], g[:, 7] = 3.0, 2.0
    s = 65536.0 + np.arange(6.0 * n)
    h = {name: 65536.0 * (k + 2) + np.arange(float(dim) * n) for k, (name, dim) in enumerate(probe.dims)}
    assert max([s.max()] + [v.max() for v in h.values()]) < 2 ** 24
    return g.reshape(-1), s, h


def random_inputs(probe: Probe, n: int, seed: int, symmetric=False):
    """random committed state and a gradient with a finite spin (the objective-rate tests); the gradient's diagonal stays
    integer, so the probe's stress update is one addition per word"""
    rng = np.random.default_rng(seed)
    g = rng.normal(scale=0.05, size=(n, 3, 3))
    if symmetric:
        g = g + g.transpose(0, 2, 1)
    for i in range(3):
        g[:, i, i] = rng.integers(-3, 4, size=n)
    s = rng.normal(scale=300.0, size=6 * n)
    h = {name: rng.normal(size=dim * n) for name, dim in probe.dims}
    return g.reshape(-1), s, h


# -- canaries -----------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


class Guarded:
    """a 16-byte aligned float64 array of ``words`` doubles inside a larger one whose margins (``MARGIN_ROWS`` rows of ``row``
    doubles on either side, rounded up to an even count) hold canary NaNs.  ``device`` None: NumPy, else a torch device."""

    def __init__(self, words: int, row: int, device=None, fill=None):
        self.m = MARGIN_ROWS * row + (MARGIN_ROWS * row) % 2
        self.words = words
        total = 2 * self.m + words
        pattern = (np.uint64(CANARY) + np.arange(total, dtype=np.uint64))
        if fill is None:
            pattern[self.m:self.m + words] = np.uint64(NAN_FILL)
        else:
            pattern[self.m:self.m + words] = bits(fill)
        self._expected = pattern.copy()
        host = pattern.view(np.float64)
        if device is None:
            self.big = host
        else:
            from fenics_constitutive_amd.hostio import to_device

            self.big = to_device(host, device)
        self.view = self.big[self.m:self.m + words]
        if device is not None:
            assert self.view.data_ptr() % 16 == 0

    def host(self):
        if isinstance(self.big, np.ndarray):
            return self.big
        from fenics_constitutive_amd.hostio import to_host

        return to_host(self.big)

    def values(self):
        return self.host()[self.m:self.m + self.words].copy()

    def margins_intact(self) -> bool:
        b = bits(self.host())
        e = self._expected
        return np.array_equal(b[:self.m], e[:self.m]) and np.array_equal(b[self.m + self.words:], e[self.m + self.words:])

    def untouched(self) -> bool:
        """margins and body hold the bits they were made with"""
        return np.array_equal(bits(self.host()), self._expected)


def first_mismatch(got, want, row: int) -> str:
    """where the first wrong word is and what it holds: the integer encoding names the array, point and component it came from"""
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size == 0:
        return "equal"
    w = int(bad[0])
    return (f"{bad.size} of {got.size} words differ; first at word {w} (point {w // row}, component {w % row}): got {got[w]!r}, "
            f"expected {want[w]!r}; last at word {int(bad[-1])} (point {int(bad[-1]) // row})")


def run_probe(law, probe: Probe, n: int, form: str, tangent: bool = True, inputs=None, device="cuda", t=T, del_t=DEL_T):
    """one call of ``law`` (the compiled ``probe``, or a JaumannRate around it) in ``form`` ("ndarray", "in_place", "from") on
    guarded buffers.  Asserts the canary margins, for "from" the committed arrays' bits, and returns (stress, tangent or None,
    history, non-converged count) with NumPy arrays.  The caller compares them with the reference."""
    g, s0, h0 = integer_inputs(probe, n) if inputs is None else inputs
    dev = None if form == "ndarray" else device
    G = Guarded(9 * n, 9, dev, fill=g)
    Tn = Guarded(36 * n, 36, dev) if tangent else None
    hist = probe.history_dim is not None
    raised = False
    if form == "from":
        Sp, S = Guarded(6 * n, 6, dev, fill=s0), Guarded(6 * n, 6, dev)
        Hp = {k: Guarded(d * n, d, dev, fill=h0[k]) for k, d in probe.dims}
        H = {k: Guarded(d * n, d, dev) for k, d in probe.dims}
        law.evaluate_from(t, del_t, G.view, Sp.view, S.view, None if Tn is None else Tn.view,
                          {k: v.view for k, v in Hp.items()} if hist else None, {k: v.view for k, v in H.items()} if hist else None)
    else:
        S = Guarded(6 * n, 6, dev, fill=s0)
        H = {k: Guarded(d * n, d, dev, fill=h0[k]) for k, d in probe.dims}
        try:
            law.evaluate(t, del_t, G.view, S.view, None if Tn is None else Tn.view, {k: v.view for k, v in H.items()} if hist else None)
        except RuntimeError as e:  # the ndarray form raises on non-convergence, after the results are written
            if form != "ndarray" or "converge" not in str(e).lower():
                raise
            raised = True
    count = law.device_stats(0)  # synchronises
    if form == "ndarray":
        assert raised == (count > 0), "the ndarray form raises exactly when a point did not converge"
    assert G.untouched(), "grad_del_u was written"
    if form == "from":
        assert Sp.untouched(), "the committed stress was written"
        for k, v in Hp.items():
            assert v.untouched(), f"the committed history '{k}' was written"
    assert S.margins_intact(), "a store outside the stress array"
    assert Tn is None or Tn.margins_intact(), "a store outside the tangent array"
    for k, v in H.items():
        assert v.margins_intact(), f"a store outside history '{k}'"
    return S.values(), None if Tn is None else Tn.values(), {k: v.values() for k, v in H.items()}, count


def assert_exact(probe: Probe, got, ref, tangent: bool = True):
    """every word of stress, tangent and history carries the reference's bits"""
    s, t, h = got[:3]
    assert same(s, ref[0]), "stress: " + first_mismatch(s, ref[0], 6)
    if tangent:
        assert same(t, ref[1]), "tangent: " + first_mismatch(t, ref[1], 36)
    for name, dim in probe.dims:
        assert same(h[name], ref[2][name]), f"history '{name}': " + first_mismatch(h[name], ref[2][name], dim)


# -- the layouts of the sweep (tests/test_gpu_user_law_layouts.py runs them, tests/test_user_law_layouts.py compiles them) -------------
SINGLE_DIMS = (1, 2, 3, 5, 7, 8, 9, 17, 18, 19, 20, 23, 35, 36, (3, 3))
NARROW = [("a", 6), ("b", 1), ("clk", 2)]  # the narrow probe of the grid-stride, count and pass-count tests (nh = 3)
WIDE4 = [("w", 36), ("x", 19), ("y", 7), ("z", 1)]
#: name -> (fields, parameters): one field (1 parameter), then mixes of narrow-even, narrow-odd and wide fields at nh = 2, 3, 4, 8
LAYOUTS = {f"f{prod(d)}" + ("t" if isinstance(d, tuple) else ""): ([("f", d)], 1) for d in SINGLE_DIMS}
LAYOUTS.update({
    "even_clk": ([("a", 8), ("clk", 2)], 0),
    "narrow": (NARROW, 1),
    "wide4": (WIDE4, 1),
    "eight": ([("pvals", 32), ("clk", 2), ("a", 3), ("b", 18), ("c", 1), ("d", 20), ("e", 6), ("g", 9)], 32),
})
SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4099)
MODES = ("explicit", "autodiff")
TRIP = 512 * 4 * 64  # points of one trip of the grid-stride loop when the launch is capped at 512 blocks (one CU)
LOOP_SIZES = (2 * TRIP, 3 * TRIP + 64 * 5 + 17)
#: name -> (fields, rotatable) of the objective-rate probes: blocks in general position
ROTATED = {
    "off3_of_9": ([("f", 9)], {"f": [3]}),
    "two_blocks_0_6": ([("f", 14)], {"f": [0, 6]}),
    "two_blocks_1_8": ([("f", 14)], {"f": [1, 8]}),
    "wide_25_13": ([("w", 36), ("x", 19)], {"w": [25], "x": [13]}),
    "middle_of_three": ([("a", 7), ("m", 8), ("c", 1)], {"m": [2]}),
}
