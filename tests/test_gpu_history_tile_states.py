"""The sparse-history kernels over every tile state they branch on (tests/tile_state_util.py: the designs, the model of the state
machine, inputs whose ballots are the designed ones; tests/test_history_tile_states.py shows on the CPU that every leaf is taken).

An optimised ResidentState (sparse trial history, packed / split / 7-double rows, sparse tangent) goes through the script beside a
state with every shortcut off.  After every call: the arrays a caller can read are those of the reference state BIT FOR BIT, the
per-tile words (``_mask``, both EVER words) and the packed runs are what the model predicts, untouched tiles keep their trial slot,
and the reference state itself agrees with the float64 oracle within the STRICT bound of test_gpu_parity.py.  The slot rows
beyond every packed run are poisoned with a NaN payload after construction: it must never reach anything a caller can read.

The same designs then go, on a reduced script, through the other launch forms that share the tile code: ResidentProblemState
(fcamd_evaluate_batch, both register budgets, laws on submeshes with consecutive and with scattered parent rows) and the
per-point-field kernels with constant fields."""

import mmap

import numpy as np
import pytest
import tile_state_util as U
from golden_util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fenics_constitutive_amd as fc  # noqa: E402
from fenics_constitutive_amd import _capi  # noqa: E402
from fenics_constitutive_amd.device import pack_rows  # noqa: E402
from fenics_constitutive_amd.problem import ResidentProblemState  # noqa: E402
from fenics_constitutive_amd.resident import ResidentState  # noqa: E402
from test_gpu_parity import STRICT  # noqa: E402

C = U.Constants()
CASES = U.cases(C)
# the ragged tiles: each story behind two full tiles, one of each size alone (n < 64)
SMALL = [c for c in CASES[1:] if not c.name.endswith("/alone") or c.name.endswith("/new_rows/alone")]
POISON = 0x7FF8DEAD0000BEEF
REF_KW = dict(sparse_history=False, sparse_tangent=False, reuse_constant_tangent=False, placement="torch")
_inputs = {}


def inputs(kind, case, script=U.SCRIPT):
    key = (kind, case.name, script)
    if key not in _inputs:
        _inputs[key] = U.build_inputs(kind, case, script)
    return _inputs[key]


def make_law(kind, fields_n=None):
    p = U.PARAMS[kind]
    if kind == "von_mises_3d":
        return fc.VonMises3D(p if fields_n is None else {k: np.full(fields_n, v) for k, v in p.items()})
    cls = {"comfe_mises_plasticity": fc.MisesPlasticityLinearHardening3D, "drucker_prager": fc.DruckerPrager3D,
           "drucker_prager_hyperbolic": fc.DruckerPragerHyperbolic3D}[kind]
    return cls({k: np.array([v]) if fields_n is None else np.full(fields_n, v) for k, v in p.items()})


def own(k):
    return np.frombuffer(mmap.mmap(-1, max(8 * k, 8)), dtype=np.float64, count=k)


def i64(t):
    return t.contiguous().view(torch.int64)


def words(w, device):
    return torch.from_numpy(np.asarray(w, dtype=np.uint64).view(np.int64).copy()).to(device)


def same(a, b):
    return torch.equal(i64(a), i64(b))


@pytest.fixture
def ctx():
    c = _capi.get_context(_capi.default_device())
    saved = {k: c.get_option(k) for k in ("host_tangent_min_points", "bounce_max")}
    yield c
    for k, v in saved.items():
        c.set_option(k, v)
    c.set_option("host_tangent_threads", -1)
    c.set_option("masked_max", -1)


def valid_rows(ever, n):
    """bool per slot row: row r of tile t lies inside the run of popcount(ever[t]) rows"""
    pop = np.array([U.popcount(int(w)) for w in ever])
    return (np.arange(64)[None, :] < pop[:, None]).reshape(-1)[:n]


def poison(state):
    """the slot rows beyond each packed run, in both copies: undefined by contract, never to be read"""
    n = state.n
    for i in (0, 1):
        ever = state._ever[i].cpu().numpy().view(np.uint64)
        beyond = torch.from_numpy(~valid_rows(ever, n)).to(state.device)
        i64(state._hist[i][state._rows_key]).view(n, 6)[beyond] = POISON


def check_against_oracle(ref, call, what, tangent=True):
    tol = STRICT["pl"]
    got = {"stress_committed": ref.stress_committed, **{f"history_committed[{k}]": v for k, v in ref.history_committed.items()}}
    want = {"stress_committed": call.committed[0], **{f"history_committed[{k}]": v for k, v in call.committed[1].items()}}
    if call.op == "E":  # (after a commit the trial copies are the former committed ones until the next evaluate)
        got.update({"stress": ref.stress, **{f"history[{k}]": v for k, v in ref.history.items()}})
        want.update({"stress": call.trial[0], **{f"history[{k}]": v for k, v in call.trial[1].items()}})
    if tangent and call.op == "E":
        got["tangent"], want["tangent"] = ref.tangent, call.tangent
    for k in got:
        g = got[k].cpu().numpy()
        assert not np.isnan(g).any(), (what, k)
        err = rel_err(g, want[k])
        assert err <= tol, f"{what}: the reference state against the oracle, {k}: {err:.3e} > {tol:.0e}"


def run_script(ctx, kind, case, layout, masked_max, mode):
    """one optimised state and one reference state through the script; every check after every call"""
    family = U.LAYOUTS[kind][layout]
    what0 = f"{kind}/{layout}/masked_max={masked_max}/{mode}/{case.name}"
    s0, h0, trace = inputs(kind, case)
    n = case.n
    ctx.set_option("masked_max", -1 if masked_max is None else masked_max)
    ctx.set_option("host_tangent_min_points", 0)
    ctx.set_option("bounce_max", 0)
    ctx.set_option("host_tangent_threads", {"pageable_threads": 2}.get(mode, 0))
    law = make_law(kind)
    opt = ResidentState(law, n, stress0=s0, history0=h0, packed_history=layout == "packed", split_history=layout != "rows7", placement="torch")
    ref = ResidentState(law, n, stress0=s0, history0=h0, **REF_KW)
    assert opt._packed == (layout == "packed") and opt._split == (layout != "rows7" and kind != "von_mises_3d"), what0
    dev = opt.device
    if opt._packed:
        poison(opt)
    model = U.run_model(case, family, U.default_masked_max(family, C) if masked_max is None else masked_max, C, U.is_dp(kind))
    host = None
    if mode != "dev":
        alloc = own if mode == "pinned" else np.empty
        host = {"g": alloc(9 * n), "s": alloc(6 * n), "t": alloc(36 * n)}
        host["s"][:], host["t"][:] = np.nan, np.nan
        if mode == "pinned":
            for a in host.values():
                ctx.register_host_buffer(a)
    try:
        for i, (call, (op, labels, w)) in enumerate(zip(trace, model)):
            what = f"{what0} call {i} ({op})"
            if op == "E":
                # what the untouched tiles must keep: their trial slot of every history array
                before = {k: i64(v).clone() for k, v in opt._hist[1 - opt._c].items()}
                g = torch.from_numpy(call.grad).to(dev)
                ref.evaluate(0.0, 1.0, g)
                if mode == "dev":
                    opt.evaluate(0.0, 1.0, g)
                    torch.cuda.synchronize()
                    assert same(opt.tangent, ref.tangent), f"{what}: device tangent"
                else:
                    host["g"][:] = call.grad
                    opt.evaluate_into(0.0, 1.0, host["g"], host["s"], host["t"])
                    torch.cuda.synchronize()
                    assert np.array_equal(host["s"].view(np.uint64), ref.stress.cpu().numpy().view(np.uint64)), f"{what}: host stress"
                    bad = host["t"].view(np.uint64) != ref.tangent.cpu().numpy().view(np.uint64)
                    assert not bad.any(), f"{what}: host tangent, rows {np.unique(np.nonzero(bad)[0] // 36)[:8]}"
                untouched = torch.from_numpy(case.point_bits([U.ALL if "untouched" in lab else 0 for lab in labels])).to(dev)
                assert int(untouched.sum()) == sum(d.npts for d, lab in zip(case.designs, labels) if "untouched" in lab)
                for k, v in opt._hist[1 - opt._c].items():
                    width = v.numel() // n
                    assert torch.equal(i64(v).view(n, width)[untouched], before[k].view(n, width)[untouched]), f"{what}: untouched tiles, trial {k}"
            else:
                opt.update()
                ref.update()
            torch.cuda.synchronize()
            # the caller's view, bit for bit
            assert same(opt.stress, ref.stress), f"{what}: stress"
            assert same(opt.stress_committed, ref.stress_committed), f"{what}: stress_committed"
            oh, ohc, rh, rhc = opt.history, opt.history_committed, ref.history, ref.history_committed
            for k in rh:
                assert same(ohc[k], rhc[k]), f"{what}: history_committed[{k}]"
                if op == "E":  # (after a commit the trial copies are the former committed ones until the next evaluate)
                    bad = i64(oh[k]) != i64(rh[k])
                    assert not bool(bad.any()), f"{what}: history[{k}], points {torch.unique(torch.nonzero(bad)[:, 0] // (rh[k].numel() // n))[:8].tolist()}"
            # the words, against the model
            assert torch.equal(opt._mask, words(w[0], dev)), f"{what}: the ballot words"
            if opt._packed:
                assert torch.equal(opt._ever[opt._c], words(w[1], dev)), f"{what}: EVER of the committed run"
                assert torch.equal(opt._ever[1 - opt._c], words(w[2], dev)), f"{what}: EVER of the trial run"
                key = "eps_n" if kind == "von_mises_3d" else "history"
                for copy, ever, rows in ((opt._c, w[1], rhc[key]),) + (((1 - opt._c, w[2], rh[key]),) if op == "E" else ()):
                    if key == "history":
                        rows = rows.view(n, 7)[:, 1:].contiguous().view(-1)
                    packed, ever_ref = pack_rows(rows)
                    assert torch.equal(ever_ref, words(ever, dev)), f"{what}: the model's EVER word against the reference state's rows"
                    valid = torch.from_numpy(valid_rows(ever, n)).to(dev)
                    assert torch.equal(i64(opt._hist[copy][opt._rows_key]).view(n, 6)[valid], i64(packed).view(n, 6)[valid]), f"{what}: packed run of copy {copy}"
            if mode == "dev":  # the anchor: the all-shortcuts-off kernel on these inputs, against the float64 oracle
                check_against_oracle(ref, call, what)
    finally:
        if mode == "pinned":
            for a in host.values():
                ctx.unregister_host_buffer(a)


LAYOUT_PARAMS = [(k, lay) for k in U.KINDS for lay in U.LAYOUTS[k]]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind,layout", LAYOUT_PARAMS, ids=[f"{k}-{lay}" for k, lay in LAYOUT_PARAMS])
def test_every_tile_state(ctx, kind, layout):
    """the main state (every full design, a ragged last tile): every masked_max through the device entry and the zero-copy host
    entry, the pageable host entry with the tangent rebuilt by the kernel and by the host's threads"""
    for masked_max in (None, 0, 64):
        for mode in ("dev", "pinned"):
            run_script(ctx, kind, CASES[0], layout, masked_max, mode)
    for mode in ("pageable", "pageable_threads"):
        run_script(ctx, kind, CASES[0], layout, None, mode)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind,layout", LAYOUT_PARAMS, ids=[f"{k}-{lay}" for k, lay in LAYOUT_PARAMS])
def test_ragged_tiles(ctx, kind, layout):
    """a last tile of 1 / 17 / 63 points behind two full tiles, and alone (n < 64), through every ragged story"""
    assert {c.n % 64 for c in SMALL} == {1, 17, 63} and any(c.n < 64 for c in SMALL)
    for case in SMALL:
        run_script(ctx, kind, case, layout, None, "dev")
    for case in SMALL[::4]:
        run_script(ctx, kind, case, layout, None, "pinned")


# ---------------------------------------------------------------------------------------------------------------------
# the other launch forms, on the reduced script
# ---------------------------------------------------------------------------------------------------------------------
REDUCED = U.cases(C, seeds=(0,))[0]


def parent_rows(k, n_laws, n_k, n_parent_offset):
    """parent rows of law k: the first half of its tiles on consecutive parent rows, the second half interleaved with the other
    laws' (scattered, ascending)"""
    half = 64 * ((n_k // 64) // 2)
    block = n_parent_offset + k * half + np.arange(half)
    base = n_parent_offset + n_laws * half
    return np.concatenate([block, base + n_laws * np.arange(n_k - half) + k]).astype(np.int32)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("kinds", [("von_mises_3d", "comfe_mises_plasticity"),
                                   ("von_mises_3d", "comfe_mises_plasticity", "drucker_prager", "drucker_prager_hyperbolic")],
                         ids=["two_laws", "four_laws_three_wave_kernel"])
def test_problem_state(ctx, kinds, packed):
    """ResidentProblemState: one fcamd_evaluate_batch launch per evaluate (with a Drucker-Prager law: the three-wave kernel), every
    law on a submesh -- tiles of consecutive parent rows and tiles of scattered ones; VonMises3D packed (SPARSE 2) and not (1)"""
    case, n_k, L = REDUCED, REDUCED.n, len(kinds)
    n = L * n_k + 5  # five parent points belong to no law
    laws = [make_law(k) for k in kinds]
    rows = [parent_rows(k, L, n_k, 3) for k in range(L)]
    data = [inputs(k, case, U.SCRIPT_SHORT) for k in kinds]
    prob = ResidentProblemState(list(zip(laws, rows)), n, placement="torch", packed_history=packed)
    assert prob._laws[0].packed == packed
    s0 = np.zeros((n, 6))
    for r, (s, _, _) in zip(rows, data):
        s0[r] = s.reshape(-1, 6)
    prob.set_state(stress=s0.reshape(-1), history=[h for _, h, _ in data])
    refs = [ResidentState(law, n_k, stress0=s, history0=h, **REF_KW) for law, (s, h, _) in zip(laws, data)]
    dev = prob.device
    rows_d = [torch.from_numpy(r.astype(np.int64)).to(dev) for r in rows]
    models = [U.run_model(case, "vm_packed" if (k == "von_mises_3d" and packed) else ("vm_unpacked" if k == "von_mises_3d" else "rows7"),
                          C.max_vm if k == "von_mises_3d" else C.max_rows7, C, U.is_dp(k), U.SCRIPT_SHORT) for k in kinds]
    for i, op in enumerate(U.SCRIPT_SHORT):
        what = f"{kinds} packed={packed} call {i} ({op})"
        if op == "E":
            grads = [torch.from_numpy(d[2][i].grad).to(dev) for d in data]
            prob.evaluate(grads)
            for ref, g in zip(refs, grads):
                ref.evaluate(0.0, 1.0, g)
        else:
            prob.update()
            for ref in refs:
                ref.update()
        torch.cuda.synchronize()
        for k, (ref, r) in enumerate(zip(refs, rows_d)):
            assert torch.equal(i64(prob.stress_1).view(n, 6)[r], i64(ref.stress).view(n_k, 6)), f"{what}: stress of law {k}"
            assert torch.equal(i64(prob.stress_0).view(n, 6)[r], i64(ref.stress_committed).view(n_k, 6)), f"{what}: committed stress of law {k}"
            if op == "E":
                assert torch.equal(i64(prob.tangent).view(n, 36)[r], i64(ref.tangent).view(n_k, 36)), f"{what}: tangent of law {k}"
            for name, v in ref.history.items():
                if op == "E":
                    assert same(prob.history_of(k, committed=False)[name], v), f"{what}: history[{name}] of law {k}"
                assert same(prob.history_of(k, committed=True)[name], ref.history_committed[name]), f"{what}: committed history[{name}] of law {k}"
            w = models[k][i][2]
            assert torch.equal(prob._laws[k].mask, words(w[0], dev)), f"{what}: ballot words of law {k}"
            if prob._laws[k].packed:
                assert torch.equal(prob._laws[k].ever[prob._c], words(w[1], dev)) and torch.equal(prob._laws[k].ever[1 - prob._c], words(w[2], dev)), f"{what}: EVER words"
    unowned = torch.ones(n, dtype=torch.bool, device=dev)
    for r in rows_d:
        unowned[r] = False
    assert int(unowned.sum()) == 5 and not bool(prob.stress_1.view(n, 6)[unowned].any()) and not bool(prob.tangent.view(n, 36)[unowned].any())


@pytest.mark.timeout(600)
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("kind", ["von_mises_3d", "comfe_mises_plasticity"])
def test_field_kernels(ctx, kind, packed):
    """the per-point-parameter kernels (evaluate_fields_kernel) with constant fields: the optimised state against a state with every
    shortcut off, and that one against the oracle of the uniform law"""
    case, n = REDUCED, REDUCED.n
    s0, h0, trace = inputs(kind, case, U.SCRIPT_SHORT)
    law = make_law(kind, fields_n=n)
    assert law.field_points == n
    opt = ResidentState(law, n, stress0=s0, history0=h0, packed_history=packed, placement="torch")
    ref = ResidentState(law, n, stress0=s0, history0=h0, **REF_KW)
    family = U.LAYOUTS[kind]["packed" if packed else "unpacked"]
    model = U.run_model(case, family, C.max_vm, C, False, U.SCRIPT_SHORT)
    if opt._packed:
        poison(opt)
    for i, (call, (op, _, w)) in enumerate(zip(trace, model)):
        what = f"{kind} fields packed={packed} call {i} ({op})"
        if op == "E":
            g = torch.from_numpy(call.grad).to(opt.device)
            opt.evaluate(0.0, 1.0, g)
            ref.evaluate(0.0, 1.0, g)
            torch.cuda.synchronize()
            assert same(opt.tangent, ref.tangent), f"{what}: tangent"
        else:
            opt.update()
            ref.update()
        torch.cuda.synchronize()
        assert same(opt.stress, ref.stress) and same(opt.stress_committed, ref.stress_committed), f"{what}: stress"
        for k, v in ref.history.items():
            assert op != "E" or same(opt.history[k], v), f"{what}: history[{k}]"
            assert same(opt.history_committed[k], ref.history_committed[k]), f"{what}: history_committed[{k}]"
        assert torch.equal(opt._mask, words(w[0], opt.device)), f"{what}: ballot words"
        if opt._packed:
            assert torch.equal(opt._ever[opt._c], words(w[1], opt.device)) and torch.equal(opt._ever[1 - opt._c], words(w[2], opt.device)), f"{what}: EVER words"
        check_against_oracle(ref, call, what)


@pytest.mark.parametrize("kind", U.KINDS)
def test_in_place_call(ctx, kind):
    """the plain in-place call (the reference contract: no ballot word, rows of the plastic points alone) on the first evaluate of
    the designs, on both sides of masked_max and at its extremes: the bits of the all-shortcuts-off state"""
    case, n = CASES[0], CASES[0].n
    s0, h0, trace = inputs(kind, case)
    law = make_law(kind)
    ref = ResidentState(law, n, stress0=s0, history0=h0, **REF_KW)
    g = torch.from_numpy(trace[0].grad).to(ref.device)
    ref.evaluate(0.0, 1.0, g)
    for masked_max in (None, 0, 64):
        ctx.set_option("masked_max", -1 if masked_max is None else masked_max)
        s = torch.from_numpy(s0).to(ref.device)
        t = torch.full((36 * n,), float("nan"), dtype=torch.float64, device=ref.device)
        h = {k: torch.from_numpy(v).to(ref.device) for k, v in h0.items()}
        law.evaluate(0.0, 1.0, g, s, t, h)
        torch.cuda.synchronize()
        what = f"{kind} in place, masked_max={masked_max}"
        assert same(s, ref.stress) and same(t, ref.tangent), what
        for k, v in ref.history.items():
            assert same(h[k], v), f"{what}: history[{k}]"
