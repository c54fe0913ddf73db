"""The host half of the rebuilt tangent (csrc/fcamd_hosttangent.cpp) without a GPU: the pool of expansion threads, expand_mises /
expand_dp / fill_const and the chunk plan, in tests/host_tangent_harness.cpp -- a producer that plays the kernel's part of
run_param_chunks' protocol (parameters of the plastic points only, the ballots behind prm * roundup(np, 64) doubles, slots reused after
their ticket) -- built plain (-O3), with ThreadSanitizer and with AddressSanitizer + UBSan, each run in a child process.

The reference is NumPy float64 written out from the expressions in expand_row, expand_dp and fill_const, operand by operand in the same
order.  NumPy does not contract a product into a following sum and the harness is built with -ffp-contract=off, so rows are compared BIT
FOR BIT; one np.longdouble evaluation of the same rows bounds the reference's own rounding.  A NaN left in the tangent (it is prefilled),
a changed canary on either side of it, a non-zero exit status or any sanitizer report fails the case.
"""

import functools
import os
import shutil
import subprocess

import host_tangent_util as U
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "fenics-constitutive_amd", "csrc")
HARNESS = os.path.join(HERE, "host_tangent_harness.cpp")

CONST, MISES, MISES_COMFE, DRUCKER_PRAGER = 0, 1, 2, 3  # HostTangentJob::Kind
PRM = {MISES: 8, MISES_COMFE: 8, DRUCKER_PRAGER: 12}
MARGIN = 256  # kMargin of the harness
CANARY = np.uint64(0x7FF4C0DEC0DEC0DE)

BUILDS = {
    "plain": ["-O3"],
    "tsan": ["-O1", "-g", "-fsanitize=thread"],
    "asan_ubsan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
}
SAN_ENV = {
    "TSAN_OPTIONS": "exitcode=66 halt_on_error=0 report_signal_unsafe=0",
    "ASAN_OPTIONS": "exitcode=67 detect_leaks=1",
    "UBSAN_OPTIONS": "print_stacktrace=1 halt_on_error=1",
}


def find_clangxx():
    """the clang++ of the ROCm installation hipcc belongs to (hipcc: as _build.py finds it)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(root, "llvm", "bin", "clang++"), os.path.join(root, "lib", "llvm", "bin", "clang++"),
                 "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand, root
    raise RuntimeError("no clang++ next to hipcc")


def compile_harness(out, flags, csrc=CSRC):
    cxx, root = find_clangxx()
    inc = root if os.path.isdir(os.path.join(root, "include", "hip")) else "/opt/rocm"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{inc}/include", f"-I{csrc}", "-ffp-contract=off", "-pthread",
           "-Wall", "-Wno-unused-function", *flags, "-o", out, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    return out


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_tangent_harness")
    return {name: compile_harness(str(d / name), flags) for name, flags in BUILDS.items()}


def call(binary, *args, timeout=600, stdin=None):
    env = dict(os.environ, **SAN_ENV)
    r = subprocess.run([binary, *map(str, args)], capture_output=True, text=True, env=env, timeout=timeout, input=stdin)
    report = "Sanitizer" in r.stderr or "runtime error" in r.stderr
    assert r.returncode == 0 and not report, f"{os.path.basename(binary)} {' '.join(map(str, args))}: exit {r.returncode}\n{r.stderr[-4000:]}"
    return r.stdout


def parse_plan(line):
    v = np.array(line.split(), dtype=np.int64)
    chunk, nslots, slot_doubles, nchunks = (int(x) for x in v[:4])
    start = v[4:]
    assert start.size == nchunks + 1
    return chunk, nslots, slot_doubles, start


def plan(binary, n, opt_chunk, prm):
    return parse_plan(call(binary, "plan", n, opt_chunk, prm))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: the expressions of expand_row / expand_dp / fill_const in NumPy, same operands, same order
# ---------------------------------------------------------------------------------------------------------------------------
I, J = np.arange(36) // 6, np.arange(36) % 6


def rows_mises(ta, tb, t, comfe, dt=np.float64):
    """expand_row: (ta[e] + B tb[e]) + C (ni nj); COMFE: (ta[e] + B tb[e]) + (C nj) ni -- e = 6 i + j, N = t[2:8]"""
    ta, tb, t = ta.astype(dt), tb.astype(dt), t.astype(dt)
    B, C, N = t[:, 0:1], t[:, 1:2], t[:, 2:8]
    ni, nj = N[:, I], N[:, J]
    if comfe:
        return (ta + B * tb) + (C * nj) * ni
    return (ta + B * tb) + C * (ni * nj)


def elastic_params(kind, s):
    """host_tangent_job: what an elastic point publishes"""
    t = np.zeros((1, 8))
    if kind == MISES:
        two_mu, four_mu2, xc1, xc2 = s[2], s[9], 0.0, 0.0
        t[0, 0] = two_mu * (1.0 - two_mu * xc2)
        t[0, 1] = four_mu2 * (xc2 - xc1)
    else:
        t[0, 0] = s[5]
    return t


def rows_dp(t11, pd, t, dt=np.float64):
    """expand_dp: (c0x t11[e] + c0y pd[e]) + ((c1x si) sj + (c1y oi) sj + (ts1 si) dj), oi = [i < 3], dj = [j < 3], s = t[6:12]"""
    t11, pd, t = t11.astype(dt), pd.astype(dt), t.astype(dt)
    c0x, c0y, c1x, c1y, ts1 = (t[:, k:k + 1] for k in range(5))
    s = t[:, 6:12]
    si, sj = s[:, I], s[:, J]
    oi, dj = (I < 3).astype(dt), (J < 3).astype(dt)
    return (c0x * t11 + c0y * pd) + (((c1x * si) * sj + (c1y * oi) * sj) + (ts1 * si) * dj)


def magnitude(kind, tables, t):
    """sum of the absolute values of the terms of a row: what the rounding of its evaluation is relative to"""
    ta, tb = tables[0], tables[1]
    if kind in (MISES, MISES_COMFE):
        B, C, N = t[:, 0:1], t[:, 1:2], t[:, 2:8]
        return np.abs(ta) + np.abs(B * tb) + np.abs(C * N[:, I] * N[:, J])
    c0x, c0y, c1x, c1y, ts1 = (t[:, k:k + 1] for k in range(5))
    s = t[:, 6:12]
    return (np.abs(c0x * ta) + np.abs(c0y * tb) + np.abs(c1x * s[:, I] * s[:, J]) + np.abs(c1y * s[:, J]) + np.abs(ts1 * s[:, I]))


@functools.lru_cache(maxsize=4)
def case_inputs(kind, n, ballot):
    """tables, scalars, parameters of EVERY point (the producer copies the plastic ones), ballot words, expected rows"""
    rng = np.random.default_rng(1000 * kind + n % 977 + 7 * len(ballot))
    tables = rng.normal(scale=1e5, size=(3, 36))
    s = rng.uniform(1e4, 2e5, size=16)
    s[9] = (2.0 * s[2]) * s[2]
    words = (n + 63) // 64
    if ballot == "zeros":
        w = np.zeros(words, dtype=np.uint64)
    elif ballot == "ones":
        w = np.full(words, ~np.uint64(0))
    elif ballot == "lane0":
        w = np.full(words, np.uint64(1))
    elif ballot == "lane63":
        w = np.full(words, np.uint64(1) << np.uint64(63))
    else:  # random, with all-0 and all-1 words among them; bits beyond a ragged last tile's count stay set
        w = rng.integers(0, 1 << 63, size=words, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=words, dtype=np.uint64)
        w[rng.random(words) < 0.1] = 0
        w[rng.random(words) < 0.1] = ~np.uint64(0)
        if n % 64:
            w[-1] |= ~np.uint64(0) << np.uint64(n % 64)
    p = np.arange(n)
    bit = ((w[p >> 6] >> (p & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    prm = PRM[kind]
    t = rng.normal(size=(n, prm))
    if kind == DRUCKER_PRAGER:
        t[:, :5] *= rng.uniform(1.0, 1e5, size=(n, 5))
        t[:, 5] = 1.0
        t[rng.random(n) < 0.02, 5] = 0.0  # the record's own flag: such a point gets the elastic table
        t[:, 6:] *= 30.0
        plastic = bit & (t[:, 5] != 0.0)
        rows = rows_dp(tables[0], tables[1], t)
        rows[~plastic] = tables[2]
        exact = rows_dp(tables[0], tables[1], t, np.longdouble)
    else:
        t[:, 0] = rng.uniform(1e4, 2e5, size=n)
        t[:, 1] = -rng.uniform(1e4, 2e5, size=n)
        plastic = bit
        rows = rows_mises(tables[0], tables[1], t, kind == MISES_COMFE)
        rows[~plastic] = rows_mises(tables[0], tables[1], elastic_params(kind, s), kind == MISES_COMFE)
        exact = rows_mises(tables[0], tables[1], t, kind == MISES_COMFE, np.longdouble)
    # the reference against itself in extended precision: three to seven roundings of terms no larger than `magnitude`
    err = np.abs(rows[plastic].astype(np.longdouble) - exact[plastic])
    assert np.all(err <= 8 * np.finfo(np.float64).eps * magnitude(kind, tables, t)[plastic]), "the float64 reference is off"
    return tables, s, t, w, rows, int(plastic.sum())


def read_tangent(path, td, n):
    raw = np.fromfile(path, dtype=np.uint64)
    assert raw.size == 2 * MARGIN + td * n
    assert np.all(raw[:MARGIN] == CANARY), "a write BEFORE the tangent array"
    assert np.all(raw[MARGIN + td * n:] == CANARY), "a write BEHIND the tangent array"
    return raw[MARGIN: MARGIN + td * n]


def describe_mismatch(got, want, td):
    bad = np.flatnonzero(got != want)
    rows = np.unique(bad // td)
    nan = np.isnan(got.view(np.float64)[bad]).sum()
    return (f"{bad.size} entries in {rows.size} rows differ ({nan} of them unwritten NaN); first rows {rows[:8].tolist()}, "
            f"first entry {bad[0]} (point {bad[0] // td}, tile {bad[0] // td // 64}, lane {bad[0] // td % 64})")


def run_case(binary, tmp, kind, n, opt_chunk, threads, ballot, off, mode, nslots=None):
    what = f"kind={kind} n={n} chunk={opt_chunk} threads={threads} ballot={ballot} off={off} mode={mode} nslots={nslots}"
    tables, s, t, w, rows, _ = case_inputs(kind, n, ballot)
    _, plan_slots, _, start = plan(binary, n, opt_chunk, PRM[kind])
    d = tmp / f"k{kind}_{n}"
    d.mkdir(exist_ok=True)
    np.concatenate([tables.ravel(), s]).tofile(d / "tables.f64")
    t.tofile(d / "params.f64")
    w.tofile(d / "ballots.u64")
    start.tofile(d / "starts.i64")
    call(binary, "run", kind, 36, n, threads, nslots or plan_slots, mode, off, d)
    got = read_tangent(d / "tangent.f64", 36, n)
    want = rows.ravel().view(np.uint64)
    assert np.array_equal(got, want), f"{what}: {describe_mismatch(got, want, 36)}"
    return start, nslots or plan_slots


# sizes around one tile, one pool task (2048 points), the short tail of the smallest default call (4467 = 70 003 - 65 536), one default
# chunk, and several chunks; chunk sizes with one task per chunk (64), two (4096), all threads (65 536) and the automatic plan
NS = [64, 65, 127, 2047, 2048, 2049, 4467, 65_536, 65_537, 70_003, 131_071, 300_001]
CHUNKS = [64, 4096, 65_536, 0]
THREADS = [1, 2, 3, 16]
BALLOTS = ["zeros", "ones", "lane0", "lane63", "random"]


def sweep(kind):
    """(n, chunk, threads, ballot, off, mode, nslots): every n; chunk, threads, ballot, alignment and producer cycled with coprime
    strides so that each kind meets every value of every dimension; then the cases the issue names"""
    out = []
    for q, n in enumerate(NS):
        chunk = CHUNKS[(q + kind) % 4]
        if chunk == 64 and n > 70_003:  # (thousands of one-tile chunks say nothing new)
            chunk = 4096
        out.append((n, chunk, THREADS[(q // 2 + kind) % 4], BALLOTS[(2 * q + kind) % 5], (q + q // 4) % 2, (q // 2 + q // 6) % 2, None))
    out += [
        (70_003, 0, 16, "random", 0, 1, None),      # the observed configuration: 65 536 + 4467 points, the tail two tasks
        (70_003, 0, 16, "random", 1, 0, None),
        (70_003, 65_536, 3, "lane63", 0, 1, None),
        (65_537, 0, 16, "random", 0, 1, None),      # a one-point tail: one task
        (300_001, 4096, 16, "random", 0, 1, 4),     # 74 chunks through four slots
        (300_001, 4096, 2, "random", 1, 0, 4),
        (131_071, 64, 3, "random", 0, 1, 4),        # 2048 one-tile chunks, the last one ragged
        (2049, 64, 1, "ones", 1, 1, None),
        (4467, 64, 16, "lane0", 0, 0, 4),
    ]
    return out


@pytest.mark.parametrize("kind", [MISES, MISES_COMFE, DRUCKER_PRAGER], ids=["mises", "mises_comfe", "drucker_prager"])
def test_sweep_covers_what_it_claims(kind, binaries):
    cases = sweep(kind)
    assert {c[0] for c in cases} >= set(NS) and {c[1] for c in cases} == set(CHUNKS) and {c[2] for c in cases} == set(THREADS)
    assert {c[3] for c in cases} == set(BALLOTS) and {c[4] for c in cases} == {0, 1} and {c[5] for c in cases} == {0, 1}
    reuse, tails = False, set()
    for n, chunk, threads, *_rest, nslots in cases:
        _, plan_slots, _, start = plan(binaries["plain"], n, chunk, PRM[kind])
        reuse |= start.size - 1 > (nslots or plan_slots)
        tail = int(start[-1] - start[-2])
        tails.add(len(call(binaries["plain"], "parts", tail, threads, kind).splitlines()))
    assert reuse and {1, 2} <= tails, (reuse, tails)
    for ballot in BALLOTS:  # every ballot kind mixes or fixes what it says
        npl = case_inputs(kind, 4467, ballot)[5]
        assert (npl == 0) == (ballot == "zeros") and (ballot != "random" or 0 < npl < 4467)


@pytest.mark.parametrize("kind", [MISES, MISES_COMFE, DRUCKER_PRAGER], ids=["mises", "mises_comfe", "drucker_prager"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_parameter_pipeline_bit_for_bit(binaries, tmp_path, build, kind):
    for case in sweep(kind):
        run_case(binaries[build], tmp_path, kind, *case)


@pytest.mark.parametrize("td", [36, 16, 1])
@pytest.mark.parametrize("build", list(BUILDS))
def test_constant_tangent_bit_for_bit(binaries, tmp_path, build, td):
    """fill_const: np.tile(table[:td], n); td = 1 has the two-point pattern, whose tasks must end right with an odd and an even count"""
    rng = np.random.default_rng(td)
    tables = rng.normal(size=(3, 36))
    np.concatenate([tables.ravel(), np.ones(16)]).tofile(tmp_path / "tables.f64")
    for q, n in enumerate(NS + [16_384, 32_768, 32_769, 98_305]):
        for threads in ((1, 16) if n > 60_000 else (THREADS[q % 4],)):
            for off in (0, 1):
                call(binaries[build], "run", CONST, td, n, threads, 4, 0, off, tmp_path)
                got = read_tangent(tmp_path / "tangent.f64", td, n)
                want = np.tile(tables[2, :td], n).view(np.uint64)
                assert np.array_equal(got, want), f"td={td} n={n} threads={threads} off={off}: {describe_mismatch(got, want, td)}"


# ---------------------------------------------------------------------------------------------------------------------------
# the chunk plan and the split of a chunk into tasks
# ---------------------------------------------------------------------------------------------------------------------------
def check_plan(line, n, opt, prm):
    chunk, nslots, slot_doubles, start = parse_plan(line)
    what = f"n={n} host_tangent_chunk={opt} prm={prm}: chunk={chunk} nslots={nslots}"
    assert chunk % 64 == 0 and chunk >= 64, what
    assert start[0] == 0 and start[-1] == n and np.all(start[:-1] % 64 == 0), what
    size = np.diff(start)
    assert np.all(size > 0) and size.max() <= chunk, what  # strictly increasing starts from 0 to n: the chunks tile [0, n)
    taper_min = chunk if opt > 0 else min(chunk, 1 << 16)  # the tail is cut in halves no further than this: only the last chunk is smaller
    assert size.size == 1 or size[:-1].min() >= taper_min, f"{what}: sizes {size[-4:].tolist()}"
    up = (size + 63) // 64 * 64
    assert np.all(prm * up + up // 64 <= slot_doubles), f"{what}: a chunk's parameters and ballots do not fit its slot ({slot_doubles} doubles)"
    assert 4 <= nslots <= 16, what
    words = nslots * (slot_doubles - chunk * prm)
    assert nslots * slot_doubles * 8 <= (256 << 20) + 8 * words, f"{what}: a ring of {nslots * slot_doubles * 8} bytes"
    assert (chunk, nslots, start.tolist()) == U.plan(n, opt, prm), f"host_tangent_util.plan({n}, {opt}, {prm}) is not the library's"


OPT_CHUNKS = [0, 64, 128, 4160, 65_536, 1 << 20]


@pytest.mark.parametrize("opt", OPT_CHUNKS)
def test_chunk_plan_properties(binaries, opt):
    """every n from 64 to 300 000 in odd steps (all residues mod 64 many times over), and 1e6, 1e7, 1e8"""
    step = 2405 if opt in (64, 128) else 65  # (one-tile chunks: thousands of starts per plan, so fewer of them; 125 > 64 sizes still)
    sizes = list(range(64, 300_001, step)) + [300_000, 10**6, 10**7, 10**8]
    assert len({n % 64 for n in sizes}) == 64
    asked = [(n, opt, prm) for n in sizes for prm in (8, 12)]
    lines = call(binaries["plain"], "plans", stdin="".join(f"{n} {o} {p}\n" for n, o, p in asked)).splitlines()
    assert len(lines) == len(asked)
    for line, (n, o, p) in zip(lines, asked):
        check_plan(line, n, o, p)


def test_default_plan_of_the_smallest_calls(binaries):
    """what the default options give just above host_tangent_min_points (the 70 003-point observation)"""
    chunk, nslots, _, start = plan(binaries["plain"], 70_003, 0, 8)
    assert (chunk, nslots, start.tolist()) == (65_536, 16, [0, 65_536, 70_003])
    assert plan(binaries["plain"], 65_536, 0, 8)[3].tolist() == [0, 65_536]
    assert plan(binaries["plain"], 10**7, 0, 8)[0] == 833_344


@pytest.mark.parametrize("threads", THREADS)
def test_tasks_of_a_chunk(binaries, threads):
    """ExpandPool::post: the tasks tile [0, np), start on tiles, and carry the parameters prm * a doubles and the ballots a / 64 words on"""
    for kind in (CONST, MISES, DRUCKER_PRAGER):
        prm = PRM.get(kind, 0)
        for np_ in sorted(set(NS + [1, 63, 4095, 4096, 4097, 8192, 16_384, 32_768, 98_304, 833_344, 1 << 20])):
            rows = [tuple(map(int, line.split())) for line in call(binaries["plain"], "parts", np_, threads, kind).splitlines()]
            what = f"kind={kind} np={np_} threads={threads}: {rows[:6]}"
            assert 1 <= len(rows) <= 4 * threads, what
            assert [r[:2] for r in rows] == U.parts(np_, threads, kind == CONST), what
            assert rows[0][0] == 0 and rows[-1][1] == np_, what
            for k, (a, b, src, mask) in enumerate(rows):
                assert a % 64 == 0 and a < b and (k == 0 or a == rows[k - 1][1]), what
                assert (src, mask) == ((-1, -1) if kind == CONST else (prm * a, a >> 6)), what
    assert len(call(binaries["plain"], "parts", 4467, threads, MISES).splitlines()) == 2
    assert len(call(binaries["plain"], "parts", 4095, threads, MISES).splitlines()) == 1
