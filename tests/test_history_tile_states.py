"""The conditions that keep tests/test_gpu_history_tile_states.py from passing for the wrong reason, checked without a GPU: the
constants parse, the designs reach every leaf of the tile state machine in every layout family (full and ragged tiles, every
bit placement), and the float64 oracle realises every designed ballot exactly and with a margin, for every law."""

import collections

import numpy as np
import pytest
import tile_state_util as U

C = U.Constants()
CASES = U.cases(C)
MAIN = CASES[0]

#: leaves every layout family must take (full tiles)
COMMON = ("untouched", "stale_only", "need_all", "all_plastic", "record_same", "record_clear")
PACKED_LEAVES = ("rows", "late_new_rows", "late_no_new_rows", "virgin", "miss_layout_grew", "miss_layout_committed", "miss_run_sharp",
                 "miss_few_sharp", "miss_new_sharp", "stale_shrink", "run_64", "run_0")
UNPACKED_LEAVES = ("masked", "dense", "stale_masked_restore", "stale_dense_store", "at_masked_max", "over_masked_max")
LEAVES = {"vm_packed": COMMON + PACKED_LEAVES + ("run_early", "run_late"), "split_packed": COMMON + PACKED_LEAVES + ("run",),
          "vm_unpacked": COMMON + UNPACKED_LEAVES, "split_unpacked": COMMON + UNPACKED_LEAVES, "rows7": COMMON + UNPACKED_LEAVES,
          "vm_inplace": ("untouched", "masked", "dense", "all_plastic", "at_masked_max", "over_masked_max")}
#: ... and their ragged counterparts (a ragged tile has fewer than 64 live lanes: no full ballot; FULL == false: neither the
#: masked path nor the rows inside a run, and no near miss of the latter)
RAGGED_LEAVES = {"vm_packed": ("untouched", "stale_only", "record_same", "record_clear", "run_early", "run_late", "late_new_rows",
                               "late_no_new_rows", "virgin", "stale_shrink", "run_0"),
                 "split_packed": ("untouched", "stale_only", "record_same", "record_clear", "run", "late_new_rows", "late_no_new_rows",
                                  "virgin", "stale_shrink", "run_0"),
                 **{f: ("untouched", "stale_only", "record_same", "record_clear", "dense", "stale_dense_store")
                    for f in ("vm_unpacked", "split_unpacked", "rows7")},
                 "vm_inplace": ("untouched", "dense")}
DP_LEAVES = ("dp_elastic_stale", "dp_elastic_clean")
#: leaves 3 to 6 of the packed families, under which every bit placement must occur
PLACED = ("late_new_rows", "late_no_new_rows", "rows", "miss_layout_grew", "miss_run_sharp", "miss_few_sharp", "miss_new_sharp", "stale_shrink")


def coverage(family, masked_max=None, drucker_prager=False):
    """(full-tile counts, ragged-tile counts, {leaf: placements}) over every case"""
    mm = U.default_masked_max(family, C) if masked_max is None else masked_max
    full, ragged, placed = collections.Counter(), collections.Counter(), collections.defaultdict(set)
    for case in CASES:
        for op, labels, _ in U.run_model(case, family, mm, C, drucker_prager):
            if labels is None:
                continue
            for d, lab in zip(case.designs, labels):
                assert len(lab & set(U.PRIMARY[family])) == 1, (family, d.name, lab)
                (full if d.npts == 64 else ragged).update(lab)
                for leaf in lab:
                    placed[leaf].add(d.place)
    return full, ragged, placed


def test_constants_parse():
    c = U.parse_constants()
    assert set(c) == {"kPackedRowsDiv", "kPackedRowsMinRun", "kRowGranule", "kMaskedRowMaxVonMises", "kMaskedRowMaxRows7"}
    assert all(isinstance(v, int) for v in c.values())
    assert 1 <= c["kPackedRowsDiv"] <= 8 and 8 <= c["kPackedRowsMinRun"] <= 56, c  # the designs need room on both sides
    assert 2 <= c["kMaskedRowMaxRows7"] <= 62 and 2 <= c["kMaskedRowMaxVonMises"] <= 62, c
    assert c["kRowGranule"] == 4, "the granule of PackedRows::load_rows meets two rows only at 4 chunks"


@pytest.mark.parametrize("family", U.FAMILIES)
def test_every_leaf_is_taken(family):
    full, ragged, _ = coverage(family, drucker_prager=family in ("split_packed", "split_unpacked", "rows7"))
    leaves = LEAVES[family] + (DP_LEAVES if family in ("split_packed", "split_unpacked", "rows7") else ())
    report = f"{family}: full tiles " + ", ".join(f"{k}={full[k]}" for k in leaves)
    print(report)
    assert all(full[k] >= 3 for k in leaves), report
    rag = RAGGED_LEAVES[family] + (DP_LEAVES if family in ("split_packed", "split_unpacked", "rows7") else ())
    report = f"{family}: ragged tiles " + ", ".join(f"{k}={ragged[k]}" for k in rag)
    print(report)
    assert all(ragged[k] >= 1 for k in rag), report
    # FULL == false disables the masked access and the rows inside a run: pinned
    assert ragged["rows"] == 0 and ragged["masked"] == 0 and not any(k.startswith("miss_") for k in ragged), dict(ragged)


@pytest.mark.parametrize("masked_max", [0, 64])
@pytest.mark.parametrize("family", ["vm_unpacked", "split_unpacked", "rows7", "vm_inplace"])
def test_masked_max_extremes(family, masked_max):
    """masked_max = 0: no touched tile is masked; 64: every full one is, but for need == ~0 where the layout says so"""
    full, ragged, _ = coverage(family, masked_max)
    if masked_max == 0:
        assert full["masked"] == 0 and full["dense"] >= 3
    else:
        assert full["masked"] >= 3 and ragged["masked"] == 0 and ragged["dense"] >= 1
        assert (full["dense"] == 0) == family.startswith("vm_"), (family, full["dense"])  # tile_von_mises masks a full need as well


@pytest.mark.parametrize("family", U.PACKED)
def test_every_placement_under_leaves_3_to_6(family):
    _, _, placed = coverage(family)
    for leaf in PLACED:
        missing = set(U.PLACEMENTS) - placed[leaf]
        assert not missing, f"{family}: {leaf} never with placement {sorted(missing)} (has {sorted(map(str, placed[leaf]))})"
    assert {"rank", "ranks_across_32", "sweep"} <= placed["rows"], placed["rows"]


def test_near_misses_differ_in_one_condition():
    """a near miss has exactly one of the four conditions false, the one it is named after; the rows leaf has none"""
    which = {"miss_layout_grew": 0, "miss_layout_committed": 0, "miss_run_sharp": 1, "miss_run": 1, "miss_few_sharp": 2, "miss_few": 2,
             "miss_new_sharp": 3, "miss_new": 3}
    seen = collections.Counter()
    for family in U.PACKED:
        for case in CASES:
            states = [U.TileState(d.ever) for d in case.designs]
            e = 0
            for op in U.SCRIPT:
                for st, d in zip(states, case.designs):
                    if op == "U":
                        U.update(st)
                        continue
                    cond = U.rows_conditions(st, d.masks[e], C)
                    before = st.words()
                    lab = U.evaluate(family, st, d.masks[e], d.npts == 64, 0, C)
                    if "rows" in lab:
                        assert all(cond) and d.npts == 64 and st.words()[1:] == before[1:], d.name
                    for k, i in which.items():
                        if k in lab:
                            assert [j for j in range(4) if not cond[j]] == [i], (d.name, k, cond)
                            seen[k] += 1
                    if "miss_run_sharp" in lab:
                        assert U.popcount(before[1]) == C.min_run - 1
                    if "miss_few_sharp" in lab:
                        assert C.div * U.popcount(d.masks[e] | before[0]) == U.popcount(before[1]) + 1
                    if "miss_new_sharp" in lab:
                        assert U.popcount(d.masks[e] & ~before[1]) == 1
                    if "miss_layout_grew" in lab:
                        assert before[2] & ~before[1], "the trial run grew at the previous evaluate of this increment"
                e += op == "E"
    assert all(seen[k] >= 6 for k in ("miss_layout_grew", "miss_layout_committed", "miss_run_sharp", "miss_few_sharp", "miss_new_sharp")), seen


def test_load_rows_granule_designs():
    """the placements of the rows path that a wrong rank or granule would hide behind: a touched row whose neighbour in the run is
    not (both orders: the granule that meets two rows), rank 63 of a 64-row run, ranks on both sides of 32 with lanes on one"""
    first, second, rank63, across = 0, 0, 0, 0
    for d in MAIN.designs:
        st = U.TileState(d.ever)
        if "rows" not in U.evaluate("vm_packed", st, d.masks[0], True, 0, C):
            continue
        run_lanes = U.lanes_of(d.ever)
        ranks = sorted(run_lanes.index(l) for l in U.lanes_of(d.masks[0]))
        for r in ranks:
            g_lo, g_hi = (3 * r) // C.granule, (3 * r + 2) // C.granule  # the granules of the row's three chunks
            if g_lo != g_hi:  # the row shares its first granule with row r - 1 and its last with row r + 1
                first += (r - 1) not in ranks and r >= 1
                second += (r + 1) not in ranks and r + 1 < len(run_lanes)
        rank63 += len(run_lanes) == 64 and 63 in ranks
        lanes = U.lanes_of(d.masks[0])
        across += min(ranks) < 32 <= max(ranks) and (min(lanes) >= 32 or max(lanes) < 32)
    assert first >= 3 and second >= 3 and rank63 >= 3 and across >= 3, (first, second, rank63, across)


def test_sweep_covers_every_run_length():
    runs = collections.defaultdict(set)
    sides = collections.Counter()
    for d in MAIN.designs:
        if d.place == "sweep":
            run, t = U.popcount(d.ever), U.popcount(d.masks[0])
            runs[run].add(t)
            if t:
                st = U.TileState(d.ever)
                sides[(run >= C.min_run, "rows" in U.evaluate("vm_packed", st, d.masks[0], True, 0, C))] += 1
    assert sorted(runs) == list(range(65))
    for run, ts in runs.items():
        assert ts == {t for t in (0, 1, 2, run // C.div, run // C.div + 1, run) if t <= run}, (run, ts)
    assert sides[(True, True)] >= 3 and sides[(True, False)] >= 3 and sides[(False, False)] >= 3 and sides[(False, True)] == 0, sides


def test_no_design_left_out():
    names = [d.name for c in CASES for d in c.designs]
    assert len(MAIN.designs) == len({d.name for d in MAIN.designs}), "design names are unique within the main state"
    assert MAIN.n % 64 == 17 and MAIN.tiles >= 500
    assert {c.designs[-1].npts for c in CASES} == {1, 17, 63}
    assert any(c.n < 64 for c in CASES) and any(c.n > 64 and c.n % 64 == r for c in CASES for r in (1, 17, 63))
    assert len(names) >= MAIN.tiles + 3 * 5


@pytest.mark.parametrize("kind", U.KINDS)
def test_oracle_realises_every_design(kind):
    """every case, every evaluate: the oracle's plastic points ARE the designed ballot (no design is skipped: a case that cannot be
    realised fails here), every point is at least 1e-3 of its yield radius (Drucker-Prager: of `a`) away from the yield surface,
    and no Drucker-Prager point fails to converge (the oracle raises)"""
    worst = np.inf
    for case in CASES:
        _, _, trace = U.build_inputs(kind, case)
        e = 0
        for call in trace:
            if call.op != "E":
                continue
            want = case.point_bits(case.words(e))
            got = U.realised_mask(kind, call.committed[1], call.trial[1])
            assert np.array_equal(got, want), f"{kind} {case.name} evaluate {e}: {int((got != want).sum())} points differ from the design"
            assert np.array_equal(call.value > 0.0, want), (kind, case.name, e)
            margin = float(np.min(np.abs(call.value) / call.scale))
            worst = min(worst, margin)
            assert margin >= 1e-3, (kind, case.name, e, margin)
            assert not np.isnan(call.tangent).any() and np.isfinite(call.trial[0]).all()
            # the plastic strain only accumulates: a row, once non-zero, stays so (the EVER word of the model)
            rows_in, rows_out = U.history_rows(kind, call.committed[1]), U.history_rows(kind, call.trial[1])
            assert ((rows_out != 0).any(axis=1) >= (rows_in != 0).any(axis=1)).all()
            e += 1
        assert e == U.N_EVAL
        # the model's EVER words are those of the oracle's rows after every call
        model = U.run_model(case, "vm_packed", 0, C)
        for call, (op, _, words) in zip(trace, model):
            for state, w in ((call.committed, words[1]),) + (((call.trial, words[2]),) if op == "E" else ()):
                nz = (U.history_rows(kind, state[1]).view(np.uint64) != 0).any(axis=1)
                assert np.array_equal(nz, case.point_bits(w)), (kind, case.name, op)
    print(f"{kind}: smallest |yield function| / scale over all designed points: {worst:.3f}")
