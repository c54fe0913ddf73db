"""The tile states of the sparse-history kernels: designs, a model of the per-tile state machine, inputs that realise the designs.

A 64-point tile of a device-resident state picks its memory path from four words -- the plastic ballot of this evaluate
(``mask``), the ballot of the previous one (``m_old`` = ``hmask[tile]``), the EVER word of the committed packed run (``ever_in``)
and of the trial run (``ever_trial``) -- and three constants (``masked_max``, ``kPackedRowsMinRun``, ``kPackedRowsDiv``).  The
conditions are those of ``tile_von_mises`` (csrc/kernels/law_von_mises.h), ``SplitRows`` / ``history7_store`` / ``sparse_record``
(history_rows.h) and the fully elastic branch of ``tile_comfe_dp`` (law_drucker_prager.h), restated here and nothing more.

No GPU is needed: ``tests/test_history_tile_states.py`` checks on the CPU that the designs reach every leaf and that the float64
oracle realises every designed ballot with a margin; ``tests/test_gpu_history_tile_states.py`` runs them on the kernels."""

from __future__ import annotations

import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenics-constitutive_amd", "csrc")
ALL = (1 << 64) - 1

# ---------------------------------------------------------------------------------------------------------------------
# constants, read from the sources: a retune moves the designs with it
# ---------------------------------------------------------------------------------------------------------------------
_CONSTANTS = {"kPackedRowsDiv": os.path.join("kernels", "history_rows.h"), "kPackedRowsMinRun": os.path.join("kernels", "history_rows.h"),
              "kRowGranule": os.path.join("kernels", "tile_io.h"), "kMaskedRowMaxVonMises": "fcamd_capi.cpp",
              "kMaskedRowMaxRows7": "fcamd_capi.cpp"}


def parse_constants() -> dict:
    """{name: int} of the constants the tiles branch on; an AssertionError names the one that does not parse"""
    out = {}
    for name, f in _CONSTANTS.items():
        with open(os.path.join(CSRC, f)) as fh:
            text = re.sub(r"//[^\n]*", " ", fh.read())
        m = re.findall(rf"\b{name}\s*=\s*(\d+)\s*[,;]", text)
        assert len(m) == 1, f"{name}: {len(m)} definitions found in csrc/{f}"
        out[name] = int(m[0])
    return out


class Constants:
    def __init__(self, c=None):
        c = parse_constants() if c is None else c
        self.div, self.min_run, self.granule = c["kPackedRowsDiv"], c["kPackedRowsMinRun"], c["kRowGranule"]
        self.max_vm, self.max_rows7 = c["kMaskedRowMaxVonMises"], c["kMaskedRowMaxRows7"]


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
#: layout families: VonMises3D packed / sparse unpacked / in place, the split laws packed / unpacked, 7-double rows
FAMILIES = ("vm_packed", "vm_unpacked", "vm_inplace", "split_packed", "split_unpacked", "rows7")
PACKED = ("vm_packed", "split_packed")
#: exactly one of these is in the label set of every evaluate of a tile
PRIMARY = {"vm_packed": ("untouched", "run_early", "run_late", "rows"),
           "split_packed": ("untouched", "run", "rows"),
           "vm_unpacked": ("untouched", "masked", "dense"), "split_unpacked": ("untouched", "masked", "dense"),
           "rows7": ("untouched", "masked", "dense"), "vm_inplace": ("untouched", "masked", "dense")}
#: the conditions of the rows-inside-a-run path, in the order of rows_conditions()
ROWS_CONDITIONS = ("layout", "run", "few", "nonew")


def popcount(x: int) -> int:
    return bin(x & ALL).count("1")


def lanes_of(x: int) -> list:
    return [i for i in range(64) if (x >> i) & 1]


def bits_of(lanes) -> int:
    x = 0
    for i in lanes:
        assert 0 <= i < 64
        x |= 1 << i
    return x


def default_masked_max(family: str, C: Constants) -> int:
    return C.max_rows7 if family == "rows7" else C.max_vm


class TileState:
    """the words a state keeps per tile"""

    def __init__(self, ever: int = 0):
        self.m_old, self.ever_c, self.ever_t = 0, ever, ever

    def words(self):
        return self.m_old, self.ever_c, self.ever_t


def rows_conditions(st: TileState, mask: int, C: Constants) -> tuple:
    """(layout, run, few, nonew): the four conditions of PackedRows::load_rows, all true on that path (of a full tile)"""
    need, run = mask | st.m_old, popcount(st.ever_c)
    return (st.ever_t == st.ever_c, run >= C.min_run, C.div * popcount(need) <= run, (mask & ~st.ever_c) == 0)


def evaluate(family: str, st: TileState, mask: int, full: bool, masked_max: int, C: Constants, drucker_prager: bool = False) -> set:
    """One evaluate of one tile with plastic ballot ``mask``: returns the labels of the path it takes (one PRIMARY label and
    tags) and moves ``st`` to the words the state must hold afterwards."""
    assert family in FAMILIES
    m_old = 0 if family == "vm_inplace" else st.m_old
    need = mask | m_old
    lab = set()
    if drucker_prager and mask == 0:  # tile_comfe_dp: the branch of the fully elastic tile
        lab.add("dp_elastic_stale" if need else "dp_elastic_clean")
    if need == 0:
        lab.add("untouched")
        return lab
    if mask == 0:
        lab.add("stale_only")
    if need == ALL:
        lab.add("need_all")
    if mask == ALL:
        lab.add("all_plastic")
    if family != "vm_inplace":
        if mask == m_old:
            lab.add("record_same")  # sparse_record: the word is not stored
        elif mask == 0:
            lab.add("record_clear")
    if family in PACKED:
        run = popcount(st.ever_c)
        cond = rows_conditions(st, mask, C)
        rows = full and all(cond)
        if family == "vm_packed":
            same_layout = full and cond[0] and cond[1]
            early = m_old != 0 and not (same_layout and C.div * popcount(m_old) <= run)
            lab.add("rows" if rows else ("run_early" if early else "run_late"))
            assert not (rows and early)
        else:
            lab.add("rows" if rows else "run")
        if not rows:
            if "run_early" not in lab:
                lab.add("late_new_rows" if mask & ~st.ever_c else "late_no_new_rows")
            if st.ever_c == 0:
                lab.add("virgin")
            if mask & ~st.ever_c:
                lab.add("new_rows")
            if full and sum(cond) == 3:  # a near miss of the rows path: one condition false
                if not cond[0]:
                    lab.add("miss_layout_grew" if (st.ever_t & ~st.ever_c) else "miss_layout_committed")
                if not cond[1]:
                    lab.add("miss_run_sharp" if run == C.min_run - 1 else "miss_run")
                if not cond[2]:
                    lab.add("miss_few_sharp" if C.div * popcount(need) == run + 1 else "miss_few")
                if not cond[3]:
                    lab.add("miss_new_sharp" if popcount(mask & ~st.ever_c) == 1 else "miss_new")
            if mask == 0 and (st.ever_t & ~st.ever_c):
                lab.add("stale_shrink")  # the trial run grew at the previous evaluate and shrinks back to ever_in
            if (st.ever_c | mask) == ALL:
                lab.add("run_64")
            if (st.ever_c | mask) == 0:
                lab.add("run_0")
            st.ever_t = st.ever_c | mask
        if not full:
            assert "rows" not in lab
            lab.add("ragged")
    else:
        if family == "rows7":
            masked = full and need != ALL and popcount(need) <= masked_max
        elif family == "split_unpacked":
            masked = full and need != ALL and popcount(need) <= masked_max
        else:  # tile_von_mises, sparse unpacked or in place
            masked = full and popcount(need) <= masked_max
        lab.add("masked" if masked else "dense")
        if mask == 0:
            lab.add("stale_masked_restore" if masked else "stale_dense_store")
        if popcount(need) == masked_max:
            lab.add("at_masked_max")
        if popcount(need) == masked_max + 1:
            lab.add("over_masked_max")
        if not full:
            assert "masked" not in lab
            lab.add("ragged")
    if family != "vm_inplace":
        st.m_old = mask
    return lab


def update(st: TileState) -> None:
    """the commit: the arrays and their EVER words swap, the ballot word stays"""
    st.ever_c, st.ever_t = st.ever_t, st.ever_c


# ---------------------------------------------------------------------------------------------------------------------
# designs
# ---------------------------------------------------------------------------------------------------------------------
#: the calls every tile goes through: evaluates take the design's next mask
SCRIPT = ("E", "E", "U", "E", "E", "E", "U", "E")
N_EVAL = SCRIPT.count("E")
#: the reduced script of the other launch forms
SCRIPT_SHORT = ("E", "E", "U", "E")


def placement(name: str, k: int = 8) -> list:
    """lanes of a bit placement: {0}, {63}, {31, 32}, every second lane (k of them, across lane 32), a block of k across lane 32"""
    if name == "l0":
        return [0]
    if name == "l63":
        return [63]
    if name == "l31_32":
        return [31, 32]
    if name == "alt":
        return [33 - k + 2 * j for j in range(k)]
    if name == "blk32":
        return [32 - k // 2 + j for j in range(k)]
    raise KeyError(name)


PLACEMENTS = ("l0", "l63", "l31_32", "alt", "blk32")


class Design:
    def __init__(self, name, ever, masks, npts=64, place=None):
        assert len(masks) == N_EVAL
        self.name, self.ever, self.masks, self.npts, self.place = name, ever, list(masks), npts, place
        live = ALL if npts == 64 else (1 << npts) - 1
        assert (ever & ~live) == 0 and all((m & ~live) == 0 for m in masks), name


def _ever_with(required, run, rng, exclude=(), top=64):
    """an EVER word of `run` rows that holds the lanes `required` and none of `exclude`"""
    req = set(required)
    pool = [i for i in range(top) if i not in req and i not in set(exclude)]
    assert len(req) <= run <= len(req) + len(pool), (run, len(req), len(pool))
    extra = rng.choice(pool, size=run - len(req), replace=False) if run > len(req) else []
    return bits_of(req | {int(i) for i in extra})


def _some(of, k, rng, exclude=0):
    pool = [i for i in lanes_of(of) if not (exclude >> i) & 1]
    assert k <= len(pool), (k, len(pool))
    return bits_of(int(i) for i in rng.choice(pool, size=k, replace=False)) if k else 0


def full_designs(C: Constants, seeds=(0, 1, 2)) -> list:
    """the designs of full tiles: stories aimed at the parsed constants, crossed with the bit placements, and the threshold sweep"""
    out = []
    long_run = max(C.min_run + 16, 3 * C.div * 4)  # a run in which the placements (<= 8 rows + 4) stay within a third
    long_run = min(long_run, 60)
    few = max(1, min(8, long_run // C.div - 4))
    for seed in seeds:
        rng = np.random.default_rng(1000 + seed)
        for pl in PLACEMENTS:
            P = bits_of(placement(pl, few))
            # rows inside the run: late, again with other rows, stale only, after a commit, the same ballot twice
            ever = _ever_with(lanes_of(P), long_run, rng)
            other = _some(ever, min(4, long_run // C.div - popcount(P)), rng, exclude=P)
            out.append(Design(f"rows/{pl}/{seed}", ever, [P, other, 0, P, P, 0], place=pl))
            # new rows late; the stale-only tile that shrinks back; new rows again; the trial layout grew: the whole run early
            ever = _ever_with([], long_run, rng, exclude=lanes_of(P))
            inside = _some(ever, 3, rng)
            out.append(Design(f"new_rows/{pl}/{seed}", ever, [P, 0, P, inside, 0, 0], place=pl))
            # ... and the grown layout with the placement in the rows touched after it
            grow = _some(ALL & ~ever & ~P, 1, rng)
            out.append(Design(f"grew/{pl}/{seed}", ever | P, [grow, P, grow, 0, P, P], place=pl))
            # ... and a new row that is COMMITTED: the trial run still has the older, shorter layout
            out.append(Design(f"committed/{pl}/{seed}", ever | P, [0, grow, P, P, 0, P], place=pl))
            # a virgin tile; its commit; more rows on the committed run
            more = _some(ALL & ~P, 5, rng)
            out.append(Design(f"virgin/{pl}/{seed}", 0, [P, P, P | more, 0, more, 0], place=pl))
            # a short run (whole run late, no new row), then early
            ever = _ever_with(lanes_of(P), max(popcount(P) + 4, C.min_run // 2), rng)
            out.append(Design(f"short_run/{pl}/{seed}", ever, [P, _some(ever, 2, rng), 0, P, 0, P], place=pl))
            # near miss: a run of MinRun - 1 rows
            ever = _ever_with(lanes_of(P), C.min_run - 1, rng)
            out.append(Design(f"miss_run/{pl}/{seed}", ever, [P, 0, P, P, 0, 0], place=pl))
            # near miss: Div * popcount(need) == run + 1
            run = next(r for r in range(max(C.min_run, C.div * popcount(P) - 1), 65) if (r + 1) % C.div == 0)
            ever = _ever_with(lanes_of(P), run, rng)
            need = P | _some(ever, (run + 1) // C.div - popcount(P), rng, exclude=P)
            half = _some(need, popcount(need) // 2, rng)
            out.append(Design(f"miss_few/{pl}/{seed}", ever, [need, 0, half, need & ~half, 0, need], place=pl))
            # near miss: one new row (the first lane of the placement), the others in the run
            lp = lanes_of(P)
            ever = _ever_with(lp[1:], long_run, rng, exclude=lp[:1])
            out.append(Design(f"miss_new/{pl}/{seed}", ever, [P, 0, 0, P, 0, 0], place=pl))
        # rows inside the run: rank-adjacent rows that share a 64-byte granule (one touched), rank 63 of a 64-row run, ranks on
        # both sides of 32 with the lanes on one side
        for r in (0, 1, 2, 3, 4, 5, 30, 31, 32, 33, 61, 62, 63):
            out.append(Design(f"rank/{r}/{seed}", ALL, [1 << r, 0, 1 << r, 1 << (r ^ 1), 0, 1 << r], place="rank"))
        top = bits_of(range(64 - max(C.min_run + 8, 48), 64))  # lanes 16 .. 63: rank = lane - 16
        lo_rank, hi_rank = [l for l in lanes_of(top) if l >= 32][:2], lanes_of(top)[-2:]
        out.append(Design(f"ranks_across_32/{seed}", top, [bits_of(lo_rank + hi_rank), bits_of(lo_rank), 0, bits_of(hi_rank), 0, 0], place="ranks_across_32"))
        # both sides of masked_max (either default), directly and as the union of two ballots; stale-only tiles of both sizes
        for mm in sorted({C.max_vm, C.max_rows7}):
            for c in (mm, mm + 1):
                if not 2 <= c <= 63:
                    continue
                m = _some(ALL, c, rng)
                a = _some(m, c // 2, rng)
                out.append(Design(f"masked_max/{c}/{seed}", ALL, [m, 0, a, m & ~a, 0, m], place=None))
        # need == ~0 with half the points plastic; all 64 plastic, twice, stale; a virgin tile that goes to 64 rows and back to 0
        even, odd = bits_of(range(0, 64, 2)), bits_of(range(1, 64, 2))
        out.append(Design(f"need_all/{seed}", ALL, [even, odd, ALL, ALL, 0, 0]))
        out.append(Design(f"all_virgin/{seed}", 0, [ALL, 0, ALL, ALL, even, odd]))
        part = _ever_with([], 40, rng)
        out.append(Design(f"all_from_part/{seed}", part, [ALL, 0, ALL & ~part, ALL, 0, ALL]))
        # untouched throughout
        out.append(Design(f"untouched/{seed}", _ever_with([], 40, rng), [0] * N_EVAL))
        out.append(Design(f"untouched_virgin/{seed}", 0, [0] * N_EVAL))
    # threshold independence: every run length, 0 / 1 / 2 / run // Div / run // Div + 1 / run touched rows
    rng = np.random.default_rng(77)
    for run in range(65):
        ever = _ever_with([], run, rng)
        for t in sorted({0, 1, 2, run // C.div, run // C.div + 1, run}):
            if t > run:
                continue
            a, b = _some(ever, t, rng), _some(ever, t, rng)
            out.append(Design(f"sweep/{run}/{t}", ever, [a, 0, b, b, 0, a], place="sweep"))
    return out


def ragged_designs(npts: int, C: Constants) -> list:
    """the stories of a ragged last tile of ``npts`` points (FULL == false: neither the masked nor the rows-inside-a-run path)"""
    rng = np.random.default_rng(500 + npts)
    live = (1 << npts) - 1
    out = []
    k = max(1, npts // 3)
    ever = _some(live, max(1, (2 * npts) // 3), rng)
    a = _some(ever, max(1, min(k, popcount(ever)) // 2), rng)
    new = _some(live & ~ever, min(2, popcount(live & ~ever)), rng) if live & ~ever else 0
    out.append(Design(f"ragged{npts}/inside", ever, [a, a, 0, a, 0, 0], npts=npts))
    out.append(Design(f"ragged{npts}/new_rows", ever, [new or a, 0, new or a, a, 0, a], npts=npts))
    out.append(Design(f"ragged{npts}/virgin", 0, [a, 0, live, live, 0, a], npts=npts))
    out.append(Design(f"ragged{npts}/all", ever, [live, live, 0, live & ~ever or live, a, 0], npts=npts))
    out.append(Design(f"ragged{npts}/untouched", ever, [0] * N_EVAL, npts=npts))
    if npts > 2 * C.min_run - 10 and npts >= C.min_run + 3:  # a long run with few touched rows: still the whole run
        ever = _some(live, npts - 1, rng)
        a = _some(ever, 2, rng)
        out.append(Design(f"ragged{npts}/long_run", ever, [a, 0, a, a, 0, 0], npts=npts))
    return out


class Case:
    """a state: full tiles and, possibly, one ragged last tile"""

    def __init__(self, name, designs):
        assert all(d.npts == 64 for d in designs[:-1])
        self.name, self.designs = name, designs
        self.tiles = len(designs)
        self.n = 64 * (len(designs) - 1) + designs[-1].npts

    def words(self, which) -> np.ndarray:
        """ever words (which = 'ever') or the masks of evaluate ``which`` as uint64"""
        return np.array([d.ever if which == "ever" else d.masks[which] for d in self.designs], dtype=np.uint64)

    def point_bits(self, words) -> np.ndarray:
        """bool per point from one word per tile"""
        w = np.asarray(words, dtype=np.uint64)
        b = ((w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        return b.reshape(-1)[: self.n]


def cases(C: Constants = None, seeds=(0, 1, 2)) -> list:
    """the main state (every full design, a ragged last tile of 17) and the small ones: a ragged tile of 1 / 17 / 63 points behind
    two full tiles, and alone (n < 64)"""
    C = Constants() if C is None else C
    full = full_designs(C, seeds)
    out = [Case("main", full + [ragged_designs(17, C)[1]])]
    fill = [d for d in full if d.name.startswith(("rows/alt/0", "new_rows/blk32/0"))]
    assert len(fill) == 2
    for npts in (1, 17, 63):
        for d in ragged_designs(npts, C):
            out.append(Case(d.name, fill + [d]))
            out.append(Case(d.name + "/alone", [d]))
    return out


def run_model(case: Case, family: str, masked_max: int, C: Constants, drucker_prager: bool = False, script=SCRIPT):
    """The model through ``script``: per call, (op, labels per tile or None, the words per tile AFTER the call as three uint64
    arrays (hmask, ever committed, ever trial))."""
    states = [TileState(d.ever) for d in case.designs]
    out, e = [], 0
    for op in script:
        labels = None
        if op == "E":
            labels = [evaluate(family, st, d.masks[e], d.npts == 64, masked_max, C, drucker_prager) for st, d in zip(states, case.designs)]
            e += 1
        else:
            for st in states:
                update(st)
        words = tuple(np.array([st.words()[i] for st in states], dtype=np.uint64) for i in range(3))
        out.append((op, labels, words))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs: gradients that realise the designed ballots with a margin, and the float64 oracle's trace
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("von_mises_3d", "comfe_mises_plasticity", "drucker_prager", "drucker_prager_hyperbolic")
PARAMS = {"von_mises_3d": {"p_ka": 175000.0, "p_mu": 80769.0, "p_y0": 1200.0, "p_y00": 2500.0, "p_w": 200.0},
          "comfe_mises_plasticity": {"mu": 80769.0, "kappa": 175000.0, "y_0": 1200.0, "h": 200.0},
          "drucker_prager": {"mu": 80769.0, "kappa": 175000.0, "a": 100.0, "b": 0.05, "b_flow": 0.02},
          "drucker_prager_hyperbolic": {"mu": 80769.0, "kappa": 175000.0, "a": 100.0, "b": 0.05, "d": 40.0, "b_flow": 0.02}}
#: which layout families a law has under ResidentState: (packed_history, split_history) -> family
LAYOUTS = {"von_mises_3d": {"packed": "vm_packed", "unpacked": "vm_unpacked"},
           **{k: {"packed": "split_packed", "unpacked": "split_unpacked", "rows7": "rows7"} for k in KINDS[1:]}}


def is_dp(kind):
    return kind.startswith("drucker_prager")


def mu_of(kind):
    return PARAMS[kind]["p_mu" if kind == "von_mises_3d" else "mu"]


def oracle_call(kind, g, s, t, h):
    """the float64 oracle, in place (C oracle: the reference's point loop)"""
    from oracle import c_oracle as CO

    p = PARAMS[kind]
    if kind == "von_mises_3d":
        CO.von_mises_3d(p, 0.0, 1.0, g, s, t, h)
    elif kind == "comfe_mises_plasticity":
        CO.comfe_mises_plasticity(p, 0.0, 1.0, g, s, t, h)
    else:
        CO.comfe_drucker_prager(p, 0.0, 1.0, g, s, t, h, hyperbolic=kind.endswith("hyperbolic"))  # raises if a point does not converge


def _dev(s):
    d = s.copy()
    d[:, :3] -= (s[:, :3].sum(axis=1) / 3.0)[:, None]
    return d


def yield_radius(kind, s, h):
    """norm of the deviatoric trial stress (6-vector) at which a point of committed state (s, h) yields under an isochoric step"""
    p = PARAMS[kind]
    if kind == "von_mises_3d":
        return math.sqrt(2.0 / 3.0) * (p["p_y0"] + (p["p_y00"] - p["p_y0"]) * (1.0 - np.exp(-p["p_w"] * h["alpha"])))
    if kind == "comfe_mises_plasticity":
        return (p["y_0"] + p["h"] * h["history"].reshape(-1, 7)[:, 0]) / math.sqrt(1.5)
    i1 = s.reshape(-1, 6)[:, :3].sum(axis=1)
    r = p["a"] - p["b"] * i1
    assert (r > 0).all()
    return math.sqrt(2.0) * (np.sqrt(r * r - p["d"] ** 2) if "d" in p else r)


def yield_value(kind, g, s, h):
    """(value of the yield function of the trial state, its scale), per point: phitr and the yield radius for the Mises laws, f
    and ``a`` for Drucker-Prager.  Written from the laws' definitions, independently of how the gradients were chosen."""
    from oracle import numpy_oracle as O

    p, mu = PARAMS[kind], mu_of(kind)
    e = O.strain_from_grad_u_full(g, O.F_PY if kind == "von_mises_3d" else O.F_RS).reshape(-1, 6)
    sv = s.reshape(-1, 6)
    tr = e[:, :3].sum(axis=1)
    nrm = np.linalg.norm(_dev(sv) + 2.0 * mu * _dev(e), axis=1)
    if not is_dp(kind):
        r = yield_radius(kind, s, h)
        return nrm - r, r
    i1 = sv[:, :3].sum(axis=1) + 3.0 * p["kappa"] * tr
    j2 = 0.5 * nrm * nrm
    return np.sqrt(j2 + p.get("d", 0.0) ** 2) + p["b"] * i1 - p["a"], np.full(nrm.shape, p["a"])


def initial_state(kind, case: Case, seed=0):
    """(stress0, history0, unit deviatoric direction per point): eps_p rows are non-zero exactly where the design's EVER bit is set"""
    rng = np.random.default_rng(seed)
    n = case.n
    d = rng.normal(size=(n, 6))
    d[:, :3] -= d[:, :3].mean(axis=1)[:, None]
    d /= np.linalg.norm(d, axis=1)[:, None]
    ever = case.point_bits(case.words("ever"))
    rows = np.where(ever[:, None], rng.normal(scale=1e-3, size=(n, 6)), 0.0)  # +0.0 rows, bit for bit, elsewhere
    if kind == "von_mises_3d":
        h = {"eps_n": rows.reshape(-1).copy(), "alpha": rng.uniform(0.0, 0.02, size=n)}
    else:
        hh = np.zeros((n, 7))
        hh[:, 1:] = rows
        hh[:, 0] = 0.0 if is_dp(kind) else rng.uniform(0.0, 0.02, size=n)
        h = {"history": hh.reshape(-1).copy()}
    s = np.zeros((n, 6))
    s[:, :3] = (-1000.0 if is_dp(kind) else 0.0) + rng.normal(scale=30.0, size=n)[:, None]
    s += (rng.uniform(0.0, 0.5, size=n) * yield_radius(kind, s.reshape(-1), h))[:, None] * d
    return s.reshape(-1).copy(), h, d


def gradient_for(kind, plastic, s, h, d, rng):
    """Gradients along the point's own deviatoric direction ``d``: the trial stress of a plastic point lands at 1.2 .. 1.6 yield
    radii, that of an elastic one at 0.3 .. 0.7 -- for a point on the yield surface (it yielded at the last commit) that is a
    reversed step, so that the sign of the yield function is not left to rounding.  The Mises laws get a volumetric part too."""
    from oracle import numpy_oracle as O

    n = d.shape[0]
    r = yield_radius(kind, s, h)
    c = np.einsum("ij,ij->i", _dev(s.reshape(-1, 6)), d)
    u = rng.uniform(size=n)
    target = np.where(plastic, 1.2 + 0.4 * u, 0.3 + 0.4 * u) * r
    a = (target - c) / (2.0 * mu_of(kind))
    f = 2.0 * (O.F_PY if kind == "von_mises_3d" else O.F_RS)
    g = np.zeros((n, 9))
    g[:, 0], g[:, 4], g[:, 8] = d[:, 0], d[:, 1], d[:, 2]
    g[:, 1] = g[:, 3] = d[:, 3] / f
    g[:, 2] = g[:, 6] = d[:, 4] / f
    g[:, 5] = g[:, 7] = d[:, 5] / f
    g *= a[:, None]
    if not is_dp(kind):
        g[:, [0, 4, 8]] += rng.normal(scale=1e-4, size=n)[:, None]
    return g.reshape(-1).copy()


def history_rows(kind, h):
    return (h["eps_n"] if kind == "von_mises_3d" else h["history"].reshape(-1, 7)[:, 1:]).reshape(-1, 6)


def realised_mask(kind, h_in, h_out):
    """the oracle's plastic points: alpha_out > alpha_in (VonMises3D), a changed eps_p row (the comfe-rs laws)"""
    if kind == "von_mises_3d":
        return h_out["alpha"] > h_in["alpha"]
    return (history_rows(kind, h_out).view(np.uint64) != history_rows(kind, h_in).view(np.uint64)).any(axis=1)


class Call:
    """one call of the trace: the gradient (evaluates), committed and trial stress / history and the trial tangent AFTER the call"""

    def __init__(self, op, grad, committed, trial, tangent, value, scale):
        self.op, self.grad, self.committed, self.trial, self.tangent, self.value, self.scale = op, grad, committed, trial, tangent, value, scale


def _copy(state):
    s, h = state
    return s.copy(), {k: v.copy() for k, v in h.items()}


def build_inputs(kind, case: Case, script=SCRIPT, seed=0):
    """(stress0, history0, trace): the oracle through ``script`` on gradients that realise the case's masks.  trace[i] is the Call
    of script[i]; after an update the trial state of the trace is the committed one (nothing evaluated yet)."""
    s0, h0, d = initial_state(kind, case, seed)
    rng = np.random.default_rng(seed + 1)
    committed, trial, tangent = (s0, h0), None, None
    trace, e = [], 0
    for op in script:
        if op == "E":
            plastic = case.point_bits(case.words(e))
            g = gradient_for(kind, plastic, committed[0], committed[1], d, rng)
            value, scale = yield_value(kind, g, committed[0], committed[1])
            trial = _copy(committed)
            tangent = np.full(36 * case.n, np.nan)
            oracle_call(kind, g, trial[0], tangent, trial[1])
            trace.append(Call(op, g, committed, trial, tangent, value, scale))
            e += 1
        else:
            assert trial is not None
            committed, trial = trial, None
            trace.append(Call(op, None, committed, committed, tangent, None, None))
    return s0, h0, trace
