"""law.evaluate(ndarrays) with the tangent rebuilt by the host's threads under DEFAULT options (automatic thread count, automatic
chunk plan, default "bounce_max" and "host_tangent_min_points": the path an unchanged dolfinx loop takes), from the smallest call that
takes it -- one 65 536-point chunk and a short ragged tail -- upwards, against the float64 C oracle: stress, tangent and every history
array at TOL and STRICT, bit for bit against the same call with the kernel's own tangent stores, the plastic count against the oracle's.

One such call (VonMises3D, 70 003 points) was once seen with a tangent off by 0.32 relative and never again, so
five cases are also repeated 200 times in one process with fresh arrays per call.  A mismatch is CLASSIFIED (diagnose() below): which
chunk, ring slot, tile, lane and pool task; whether the wrong row is the law's elastic row (a lost ballot bit, a stale ballot word),
another point's correct row (misplaced parameters, a stale slot) or unwritten; and whether the same point's stress and history are right
(they are written by the kernel straight into the caller's arrays: if they are wrong too, the inputs or the page locks are at fault and
not the parameter ring or the expansion).  The classification goes into the assertion message and into an .npz under pytest's tmp path.
"""

import time

import numpy as np
import pytest
from golden_util import rel_err
from host_tangent_util import locate, plan

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402,F401
from fenics_constitutive_amd import _capi  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from test_gpu_drucker_prager import make as make_dp  # noqa: E402
from test_gpu_parity import STRICT, TOL, VM_P, make_law, random_case  # noqa: E402
from test_gpu_user_law_autodiff import vm_inputs  # noqa: E402
from test_oracle_golden import dp_inputs  # noqa: E402

HOST_TANGENT_CPU = 16  # include/fcamd.h: FCAMD_HOST_TANGENT_CPU
# (stress and history, tangent): the bounds of test_gpu_parity.py; Drucker-Prager: those of test_gpu_drucker_prager.py
BOUNDS = {"le": [(TOL["le"], TOL["le"]), (STRICT["le"], STRICT["le"])], "pl": [(TOL["pl"], TOL["pl"]), (STRICT["pl"], STRICT["pl"])],
          "dp": [(1e-6, 1e-6), (1e-9, 1e-7)]}
KINDS = ["von_mises_3d", "comfe_mises_plasticity", "dp_classic", "dp_hyperbolic", "linear_elasticity"]
CLASS = {"von_mises_3d": "pl", "comfe_mises_plasticity": "pl", "dp_classic": "dp", "dp_hyperbolic": "dp", "linear_elasticity": "le"}
PRM = {"von_mises_3d": 8, "comfe_mises_plasticity": 8, "dp_classic": 12, "dp_hyperbolic": 12, "linear_elasticity": 0}
# one chunk; one chunk and a tail of 1 / 63 / 64 / 4467 points; two chunks less one point; two chunks and a point; four; a tapered
# tail (300 001 = 4 x 65 536 + 37 857); twelve chunks and a point
SIZES = [65_536, 65_537, 65_599, 65_600, 70_003, 131_071, 131_073, 201_075, 300_001, 786_433]
REPEATS = 200


@pytest.fixture
def ctx():
    """the thread's context with its options as they come; only where the box grants too few CPUs for the automatic thread count
    (it resolves to 0 = off) six threads are asked for -- every message of this file names the count in use"""
    c = _capi.get_context(_capi.default_device())
    auto = c.get_option("host_tangent_threads")
    if auto == 0:
        c.set_option("host_tangent_threads", 6)
    yield c
    c.set_option("host_tangent_threads", -1)
    assert c.get_option("host_tangent_threads") == auto


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Case:
    """a law, its inputs and the oracle's outputs"""

    def __init__(self, kind, n, seed=None, flaky_inputs=False):
        self.kind, self.n, self.del_t = kind, n, 1.0
        seed = n % 1009 + len(kind) if seed is None else seed
        if kind.startswith("dp_"):
            self.law, p = make_dp(kind == "dp_hyperbolic")
            self.g, self.s0, self.h0 = dp_inputs(n, seed)
            run = lambda g, s, t, h: CO.comfe_drucker_prager(p, 0.0, self.del_t, g, s, t, h, hyperbolic=kind == "dp_hyperbolic")[0]  # noqa: E731
        else:
            p, self.g, self.s0, self.h0 = random_case(kind, n, seed)
            if flaky_inputs:  # test_gpu_user_law_autodiff.py::test_von_mises_values_bitwise_and_tangent[70003]
                p, (self.g, self.s0, self.h0) = VM_P, vm_inputs(n, 11)
            self.law = make_law(kind, p)
            run = lambda g, s, t, h: CO.MODELS[kind](p, 0.0, self.del_t, g, s, t, h)  # noqa: E731
        self.s_ref, self.t_ref = self.s0.copy(), np.zeros(36 * n)
        self.h_ref = None if self.h0 is None else {k: v.copy() for k, v in self.h0.items()}
        out = run(self.g, self.s_ref, self.t_ref, self.h_ref)
        self.npl_ref = None if kind == "linear_elasticity" else int(out[0] if isinstance(out, tuple) else out)
        # the oracle's plastic points: the hardening variable moved
        if kind == "von_mises_3d":
            self.plastic_ref = self.h_ref["alpha"] != self.h0["alpha"]
        elif kind == "linear_elasticity":
            self.plastic_ref = np.zeros(n, dtype=bool)
        else:
            self.plastic_ref = self.h_ref["history"].reshape(n, 7)[:, 0] != self.h0["history"].reshape(n, 7)[:, 0]

    def call(self):
        """one in-place host call on FRESH arrays (allocating and freeing them is part of the scenario): stress, tangent, history"""
        s, t = self.s0.copy(), np.full(36 * self.n, np.nan)
        h = None if self.h0 is None else {k: v.copy() for k, v in self.h0.items()}
        self.law.evaluate(0.0, self.del_t, self.g, s, t, h)
        return s, t, h


def point_ok(a, b, dim, p, tol, scale_of):
    """does point p of array a agree with the oracle's b within tol (relative to the array's largest entry, as rel_err)?"""
    return bool(np.max(np.abs(a.reshape(-1, dim)[p] - b.reshape(-1, dim)[p])) <= tol * scale_of)


def diagnose(ctx, case, got, kernel, call_no, tmp_path, what):
    """Classify the first wrong tangent rows of `got` (see the module's docstring); returns the text, leaves the .npz behind."""
    n, kind = case.n, case.kind
    s, t, h = got
    threads = ctx.get_option("last_host_tangent_threads")
    mode = ctx.last_host_mode()
    const = kind == "linear_elasticity"
    chunk, nslots, starts = (0, 0, [0, n]) if const else plan(n, 0, PRM[kind])
    T, Tk, Tr = t.reshape(n, 36), kernel[1].reshape(n, 36), case.t_ref.reshape(n, 36)
    tol_s, tol_t = BOUNDS[CLASS[kind]][1]
    tscale = np.max(np.abs(Tr))
    wrong = np.flatnonzero((bits(T) != bits(Tk)).any(axis=1) | ~(np.abs(T - Tr).max(axis=1) <= tol_t * tscale))
    # stress / history rows that differ from the kernel-stores call, wherever they are
    others = {"stress": (s, kernel[0], case.s_ref, 6)}
    for k in (h or {}):
        others[k] = (h[k], kernel[2][k], case.h_ref[k], h[k].size // n)
    other_wrong = {k: np.flatnonzero((bits(a.reshape(n, d)) != bits(b.reshape(n, d))).any(axis=1)) for k, (a, b, _, d) in others.items()}
    # a wrong stretch of stress or history: where it lies (a 4 KiB page is 512 doubles) and whether it still holds the INPUT (a lost write)
    inputs = dict({"stress": case.s0}, **(case.h0 or {}))
    stretches = {}
    for k, (a_, b_, _, _) in others.items():
        flat = np.flatnonzero(bits(a_) != bits(b_))
        if flat.size:
            stretches[k] = (int(flat[0]), int(flat[-1]), int(flat.size), bool(np.array_equal(bits(a_)[flat], bits(inputs[k])[flat])),
                            int(a_.ctypes.data % 4096))
    el = np.flatnonzero(~case.plastic_ref)
    elastic_row = Tk[el[0]] if el.size and kind != "linear_elasticity" else Tk[0]
    rows_void = np.ascontiguousarray(Tk).view(np.dtype((np.void, 288))).ravel()
    lines = [f"{what}: call {call_no}: {wrong.size} wrong tangent rows of {n}; threads {threads}, last_host_mode {mode}, chunk {chunk}, "
             f"nslots {nslots}, starts {starts[:6]}{'...' if len(starts) > 6 else ''}; rows of other arrays that differ from the "
             f"kernel-stores call: { {k: v.size for k, v in other_wrong.items()} }; their wrong doubles (first, last, count, still the input's bits, "
             f"array address mod 4096): {stretches}"]
    rec = {"call": call_no, "n": n, "threads": threads, "mode": mode, "chunk": chunk, "nslots": nslots, "starts": np.array(starts),
           "wrong_points": wrong, "other_stretches": np.array([v for v in stretches.values()], dtype=np.int64).reshape(-1, 5), "got_rows": T[wrong[:64]], "kernel_rows": Tk[wrong[:64]], "oracle_rows": Tr[wrong[:64]]}
    codes = []
    for p in wrong[:8].tolist():
        where = locate(p, n, max(threads, 1), 0, PRM[kind] or 8, const)
        row = T[p]
        same_as = np.flatnonzero(rows_void == np.ascontiguousarray(row).view(np.dtype((np.void, 288)))[0])
        same_as = same_as[same_as != p]
        is_nan = bool(np.isnan(row).any())
        is_elastic = bool(np.array_equal(bits(row), bits(elastic_row)))
        side_ok = all(point_ok(a, r, d, p, tol_s, np.max(np.abs(r))) and np.array_equal(bits(a.reshape(n, d)[p]), bits(b.reshape(n, d)[p]))
                      for a, b, r, d in others.values())
        if is_nan:
            verdict = "UNWRITTEN (NaN): no task covered the row or its task never ran"
        elif is_elastic and case.plastic_ref[p]:
            verdict = "the law's ELASTIC row at a plastic point: a lost ballot bit or a stale ballot word"
        elif same_as.size:
            verdict = f"ANOTHER point's correct row (point {same_as[:3].tolist()}): misplaced parameters or a stale slot"
        else:
            verdict = "no row of this call: stale parameters of an earlier call or chunk, or a wrong expansion"
        verdict += ("; stress and history of the point are right -> the parameter ring or the expansion" if side_ok else
                    "; stress or history of the point are WRONG too -> the inputs / page locks, not the tangent path")
        codes.append((p, int(is_nan), int(is_elastic), int(same_as[0]) if same_as.size else -1, int(side_ok), int(case.plastic_ref[p])))
        lines.append(f"  point {p} ({where}), oracle says {'plastic' if case.plastic_ref[p] else 'elastic'}, "
                     f"|row - oracle| / max|oracle| = {np.max(np.abs(row - Tr[p])) / tscale:.3e}: {verdict}")
    rec["classified"] = np.array(codes, dtype=np.int64).reshape(-1, 6)  # point, nan, elastic row, same as point, side arrays ok, oracle plastic
    path = tmp_path / f"host_tangent_mismatch_{kind}_{n}_call{call_no}.npz"
    np.savez_compressed(path, **rec)
    lines.append(f"  record: {path}")
    return "\n".join(lines)


def check_call(ctx, case, got, kernel, scales, call_no, tmp_path, what):
    """every output against the oracle at TOL and STRICT and bit for bit against the kernel-stores call; a failure is classified"""
    s, t, h = got
    mode = ctx.last_host_mode()
    assert mode & HOST_TANGENT_CPU, f"{what}: call {call_no} did not take the host-tangent path (mode {mode})"
    arrays = [("stress", s, kernel[0], case.s_ref, 0), ("tangent", t, kernel[1], case.t_ref, 1)]
    arrays += [(k, h[k], kernel[2][k], case.h_ref[k], 0) for k in (h or {})]
    failed = []
    for name, a, b, r, which in arrays:
        err = float(np.max(np.abs(a - r))) / scales[name]
        if call_no == 0:
            print(f"{what}: {name}: rel. error against the oracle {err:.3e}")
        for level, bound in zip(("TOL", "STRICT"), BOUNDS[CLASS[case.kind]]):
            if not err <= bound[which]:
                failed.append(f"{name}: {err:.3e} > {level} {bound[which]:.0e}")
        if not np.array_equal(bits(a), bits(b)):
            failed.append(f"{name}: {int(np.sum(bits(a) != bits(b)))} entries differ in bits from the call with the kernel's tangent stores")
    if failed:
        raise AssertionError(f"{what}: call {call_no}: " + "; ".join(failed) + "\n" + diagnose(ctx, case, got, kernel, call_no, tmp_path, what))
    if case.npl_ref is not None:
        npl = case.law.last_stats.n_plastic
        assert 0 < npl < case.n and npl == case.npl_ref, f"{what}: call {call_no}: {npl} plastic points, the oracle has {case.npl_ref} of {case.n}"


def kernel_stores_call(ctx, case):
    """the same call with "host_tangent_threads" = 0 (the kernel writes the tangent); the option is put back"""
    was = ctx.get_option("host_tangent_threads")
    ctx.set_option("host_tangent_threads", 0)
    try:
        out = case.call()
        assert not (ctx.last_host_mode() & HOST_TANGENT_CPU)
    finally:
        ctx.set_option("host_tangent_threads", was)
    return out


def scales_of(case):
    sc = {"stress": np.max(np.abs(case.s_ref)), "tangent": np.max(np.abs(case.t_ref))}
    sc.update({k: np.max(np.abs(v)) for k, v in (case.h_ref or {}).items()})
    return {k: float(v) for k, v in sc.items()}


def run_once(ctx, case, tmp_path, what):
    kernel = kernel_stores_call(ctx, case)
    threads = ctx.get_option("host_tangent_threads")
    what = f"{what} (threads {threads})"
    check_call(ctx, case, case.call(), kernel, scales_of(case), 0, tmp_path, what)
    assert ctx.get_option("last_host_tangent_threads") == threads, what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_default_path_against_the_oracle(ctx, tmp_path, kind, n):
    run_once(ctx, Case(kind, n), tmp_path, f"{kind} n={n}")


@pytest.mark.parametrize("n", [32_768, 32_769])
def test_linear_elasticity_from_its_own_threshold(ctx, tmp_path, n):
    """the one-shot fill of a constant tangent starts at half of "host_tangent_min_points" """
    run_once(ctx, Case("linear_elasticity", n), tmp_path, f"linear_elasticity n={n}")


def test_a_default_plan_that_reuses_ring_slots(ctx, tmp_path):
    """up to 786 433 points the default plan has fewer chunks than ring slots; from some 4e6 points the chunks (a twelfth of the call)
    are large enough for 256 MiB to hold fewer slots than the call has chunks"""
    n = 4_000_037
    _, nslots, starts = plan(n, 0, 8)
    assert len(starts) - 1 > nslots, (nslots, starts)
    run_once(ctx, Case("von_mises_3d", n), tmp_path, f"von_mises_3d n={n}")


def test_the_inputs_of_the_flaky_observation(ctx, tmp_path):
    run_once(ctx, Case("von_mises_3d", 70_003, flaky_inputs=True), tmp_path, "VonMises3D vm_inputs(70003, 11)")


REPEATED = [("von_mises_3d", 70_003, True), ("comfe_mises_plasticity", 70_003, False), ("dp_classic", 70_003, False),
            ("dp_hyperbolic", 65_599, False), ("linear_elasticity", 70_003, False)]


@pytest.mark.parametrize("kind,n,flaky", REPEATED, ids=[f"{k}-{n}" for k, n, _ in REPEATED])
def test_repeated_calls_in_one_process(ctx, tmp_path, kind, n, flaky):
    """REPEATS calls, a fixed count and no retry: fresh arrays per call, every call against the oracle's outputs computed once; the loop
    ends at the first mismatch (classified) or the first error a call raises"""
    case = Case(kind, n, flaky_inputs=flaky)
    kernel = kernel_stores_call(ctx, case)
    scales = scales_of(case)
    what = f"{kind} n={n} (threads {ctx.get_option('host_tangent_threads')})"
    t0 = time.perf_counter()
    for call_no in range(REPEATS):
        check_call(ctx, case, case.call(), kernel, scales, call_no, tmp_path, what)
    print(f"{what}: {REPEATS} calls in {time.perf_counter() - t0:.2f} s")


def test_diagnosis_names_what_was_done_to_a_row(ctx, tmp_path):
    """the classification itself, on outputs spoiled on purpose AFTER a correct call (no kernel is involved): an elastic row at a plastic
    point, a neighbour's row, an unwritten row, and a point whose stress is wrong as well"""
    case = Case("von_mises_3d", 70_003, flaky_inputs=True)
    kernel = kernel_stores_call(ctx, case)
    s, t, h = case.call()
    pl, el = np.flatnonzero(case.plastic_ref), np.flatnonzero(~case.plastic_ref)
    a, b, c, d = (int(x) for x in (pl[pl > 65_536][0], pl[100], pl[200], pl[300]))
    T = t.reshape(-1, 36)
    T[a] = T[el[0]]
    T[b] = T[pl[101]]
    T[c] = np.nan
    T[d] = T[pl[301]]
    s.reshape(-1, 6)[d] += 1.0
    text = diagnose(ctx, case, (s, t, h), kernel, 7, tmp_path, "spoiled")
    by_point = {int(line.split()[1]): line for line in text.splitlines() if line.startswith("  point")}
    assert "ELASTIC row" in by_point[a] and "'chunk': 1" in by_point[a] and "the parameter ring or the expansion" in by_point[a]
    assert f"ANOTHER point's correct row (point [{int(pl[101])}" in by_point[b] and "'chunk': 0" in by_point[b]
    assert "UNWRITTEN" in by_point[c]
    assert "WRONG too" in by_point[d]
    rec = np.load(next(tmp_path.glob("host_tangent_mismatch_*call7.npz")))
    assert sorted(rec["wrong_points"].tolist()) == sorted([a, b, c, d]) and int(rec["call"]) == 7 and rec["starts"].tolist() == [0, 65_536, 70_003]
    with pytest.raises(AssertionError, match="4 wrong tangent rows"):
        check_call(ctx, case, (s, t, h), kernel, scales_of(case), 7, tmp_path, "spoiled")
