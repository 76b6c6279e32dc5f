"""The expectation of tests/test_gpu_polish_encoder_cases.py pinned on the CPU: on every hand-built pileup and span of
tests/polish_encoder_cases.py the restatement (oracle/pileup_oracle.cpp) equals the reference's own SummaryGenerator
(oracle/_ref/libref_polish_encoder.so) -- spans that differ from the region, reads over the edges, N / P as gaps included, which
tests/test_encoder_oracle.py does not reach --, a committed golden holds what that build gave (the check that still runs where
the build is absent), and three small pileups have their rows written out by hand.  The module also pins what the catalogue
promises (which operation is operation 64 and on which row, which sizes outgrow the first guess), so that the GPU module
cannot pass by missing an edge.  CPU only; exact integer parity."""
import importlib.util
import os

import numpy as np
import pytest

import pileup_utils as pu
import polish_encoder_cases as pc
from conftest import need_reference_build

GOLDEN_NAME = "encoder_polish_cases.npz"


@pytest.fixture(scope="module")
def oracle():
    return pu.load_restatement()


@pytest.fixture(scope="module")
def families():
    return {name: fn() for name, fn in pc.FAMILIES.items()}


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_restatement_equals_reference_build_on_the_catalogue(oracle, families, family):
    ref = pu.load_reference_polish_encoder()
    if ref is None:
        need_reference_build("oracle/_ref")
    for name, case in families[family].items():
        pile = pc.pileup(case)
        for start, end in case[4]:
            img_o, pos_o = pu.run_polish_oracle(oracle, pile, start, end)
            img_r, pos_r = pu.run_polish_reference(ref, pile, start, end)
            assert img_o.shape == img_r.shape and img_o.shape[0] >= end - start + 1, (name, start, end)
            assert np.array_equal(pos_o, pos_r), (name, start, end)
            assert np.array_equal(img_o, img_r), (name, start, end)


def test_restatement_against_the_committed_golden(oracle, families, golden_dir):
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    seen = 0
    for family in pc.GOLDEN_FAMILIES:
        for name, case in families[family].items():
            pile = pc.pileup(case)
            for k, (start, end) in enumerate(case[4]):
                img, pos = pu.run_polish_oracle(oracle, pile, start, end)
                assert np.array_equal(img, g["%s__%s__%d__image" % (family, name, k)]), (family, name, k)
                assert np.array_equal(pos, g["%s__%s__%d__positions" % (family, name, k)]), (family, name, k)
                seen += 1
    assert 2 * seen == len(g.files)


def test_golden_reproduces_from_its_script_and_stays_small(golden_dir):
    """What tests/golden/make_golden_polish_cases.py would write today is what is committed; data only, smaller than the
    largest file beside it."""
    ref = pu.load_reference_polish_encoder()
    if ref is None:
        need_reference_build("oracle/_ref")
    spec = importlib.util.spec_from_file_location("make_golden_polish_cases", os.path.join(golden_dir, "make_golden_polish_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = mod.golden_arrays(ref)
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    assert sorted(g.files) == sorted(want)
    for key, value in want.items():
        assert g[key].dtype == value.dtype and np.array_equal(g[key], value), key
    others = [os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if f != GOLDEN_NAME]
    assert os.path.getsize(os.path.join(golden_dir, GOLDEN_NAME)) < max(others)


# ---- rows worked out by hand ---------------------------------------------------------------------------------------------------
# features: 0 .. 3 = A C G T reverse, 4 .. 7 = A C G T forward, 8 = gap / other reverse, 9 = gap / other forward
# pixel = uint8(int64(count / max(1, coverage) * 254) & 0xff)

def _rows(lib, case, run=pu.run_polish_oracle):
    img, pos = run(lib, pc.pileup(case), *case[4][0])
    return {(int(p) - case[0], int(i)): row.tolist() for (p, i), row in zip(pos, img)}


def _both(oracle):
    out = [(oracle, pu.run_polish_oracle)]
    ref = pu.load_reference_polish_encoder()
    if ref is not None:
        out.append((ref, pu.run_polish_reference))
    return out


def test_by_hand_deletion_only_column(oracle, families):
    """Rows 7 .. 13 lie inside all three deletions and no deletion starts there: nothing is credited to their coverage, so the
    divisor is max(1, 0) = 1.  Forward gaps: 2 -> 2 * 254 = 508 -> 508 & 0xff = 252 (the cast wraps).  Reverse gaps: 1 -> 254.
    Row 6 has the same counts but is the third deletion's first row: coverage 10 -> 2 / 10 * 254 = 50.8 -> 50, 1 / 10 * 254 ->
    25.  Row 5 is inside the first deletion and the first row of the second: coverage 10 (the second deletion's ten positions)
    + 1 (the third read's C, reverse -> feature 1) = 11; forward gaps 2 -> 2 / 11 * 254 = 46.18 -> 46; C: 1 / 11 * 254 = 23.09
    -> 23."""
    case = families["by_hand"]["deletion_only"]
    for lib, run in _both(oracle):
        rows = _rows(lib, case, run)
        for r in range(7, 14):
            assert rows[r, 0] == [0, 0, 0, 0, 0, 0, 0, 0, 254, 252], r
        assert rows[6, 0] == [0, 0, 0, 0, 0, 0, 0, 0, 25, 50]
        assert rows[5, 0] == [0, 23, 0, 0, 0, 0, 0, 0, 0, 46]
        assert len(rows) == 30
    # the same quirk in the catalogue's three-tile pileup
    gaps = families["tile_edges"]["gaps"]
    rows = _rows(oracle, gaps)
    for r in pc.DELETION_ONLY_ROWS:
        assert rows[r, 0] == [0, 0, 0, 0, 0, 0, 0, 0, 254, 252], r
    for r in pc.MAPQ0_ROWS:
        assert rows[r, 0] == [0] * 10, r


def test_by_hand_insert_on_a_deletion_start(oracle, families):
    """Row 2: the forward read's G (feature 6) and, from the reverse read, the first position of a deletion of 4: the deletion
    credits its 4 positions to row 2, so coverage(2) = 1 + 4 = 5.  Base row: G forward 1 / 5 * 254 = 50.8 -> 50, reverse gap
    1 / 5 * 254 -> 50.  The insert AC anchored on row 2 is normalised by that same 5: A forward (feature 4) -> 50 in insert row 1,
    C forward (feature 5) -> 50 in insert row 2.  Row 3: T forward with coverage 1 -> 254, reverse gap 1 / 1 * 254 -> 254 (the
    deletion's credit went to row 2, not here)."""
    case = families["by_hand"]["insert_on_deletion_start"]
    for lib, run in _both(oracle):
        rows = _rows(lib, case, run)
        assert rows[2, 0] == [0, 0, 0, 0, 0, 0, 50, 0, 50, 0]
        assert rows[2, 1] == [0, 0, 0, 0, 50, 0, 0, 0, 0, 0]
        assert rows[2, 2] == [0, 0, 0, 0, 0, 50, 0, 0, 0, 0]
        assert rows[3, 0] == [0, 0, 0, 0, 0, 0, 0, 254, 254, 0]
        assert rows[1, 0] == [0, 127, 0, 0, 0, 0, 127, 0, 0, 0]     # C reverse and G forward, coverage 2: 1 / 2 * 254 = 127
        assert len(rows) == 12 and (2, 3) not in rows


def test_by_hand_staircase_column(oracle, families):
    """Row 6 is under reads 0 .. 6: coverage 7.  A (even reads 0, 2, 4, 6): reverse for 0 and 6 (k % 3 == 0) -> feature 0 = 2,
    forward for 2 and 4 -> feature 4 = 2.  C (odd reads 1, 3, 5): reverse for 3 -> feature 1 = 1, forward for 1 and 5 ->
    feature 5 = 2.  2 / 7 * 254 = 72.57 -> 72; 1 / 7 * 254 = 36.28 -> 36.  Row 39 and beyond: coverage 40, 20 A and 20 C; reverse
    reads 0, 3, .., 39: 14 of them, the even ones (0, 6, .., 36: 7) are A: A rev 7, A fwd 13, C rev 7, C fwd 13: 7 / 40 * 254 =
    44.45 -> 44, 13 / 40 * 254 = 82.55 -> 82."""
    case = families["staircase"]["staircase"]
    for lib, run in _both(oracle):
        rows = _rows(lib, case, run)
        assert rows[6, 0] == [72, 36, 0, 0, 72, 72, 0, 0, 0, 0]
        assert rows[0, 0] == [254, 0, 0, 0, 0, 0, 0, 0, 0, 0]
        assert rows[39, 0] == rows[63, 0] == [44, 44, 0, 0, 82, 82, 0, 0, 0, 0]


# ---- what the catalogue promises -----------------------------------------------------------------------------------------------
def _walk(read_, region_start):
    """(index, op, first row, rows) of every operation."""
    row, out = read_["pos"] - region_start, []
    for i, (op, n) in enumerate(read_["cigar"]):
        adv = n if op in (pc.M, pc.EQ, pc.X, pc.D, pc.N, pc.P) else 0
        out.append((i, op, row, adv))
        row += adv
    return out


def test_catalogue_puts_operation_64_where_it_says(families):
    mo = families["many_operations"]
    for name, kind, check in (("op64_insert_on_511", pc.I, lambda first, n: first - 1 == 511),
                              ("op64_deletion_from_512", pc.D, lambda first, n: first == 512),
                              ("op64_match_over_1023", pc.M, lambda first, n: first <= 1023 < 1024 <= first + n - 1)):
        reads = mo[name][3]
        assert sorted(len(r["cigar"]) for r in reads) == list(pc.OP_COUNTS)
        for r in reads:
            ops = _walk(r, mo[name][0])
            i, op, first, n = ops[64] if len(ops) > 64 else [o for o in ops if o[1] == kind and (kind != pc.M or o[3] == 3)][-1]
            assert op == kind and check(first, n), (name, len(ops), i, first)
            assert len(ops) <= 64 or i == 64
    for r in mo["third_tile_record"][3]:
        owner = [o for o in _walk(r, pc.R0) if o[3] > 0 and o[2] <= 1024 <= o[2] + o[3] - 1]
        assert len(r["cigar"]) == 200 and len(owner) == 1 and owner[0][0] >= 64 and owner[0][2] < 1024


def test_catalogue_shapes(families):
    te = families["tile_edges"]
    for case in te.values():
        assert case[0] == pc.R0 > 0 and case[1] - case[0] + 1 == 1537 and case[4] == [(case[0], case[1])]
    starts = {(r["pos"] - pc.R0, r["cigar"][0]) for r in te["first_m"][3]}
    assert starts == {(row, (pc.M, n)) for row in pc.EDGE_ROWS for n in (1, 600)}
    lead = {(r["pos"] - pc.R0, tuple(op for op, _ in r["cigar"])) for r in te["leading_inserts"][3]}
    assert lead == {(row, ops) for row in pc.EDGE_ROWS for ops in ((pc.I, pc.M), (pc.S, pc.I, pc.M), (pc.H, pc.S, pc.I, pc.M))} | \
        {(pc.L0, (pc.I, pc.M)), (pc.L0, (pc.S, pc.I, pc.M))}
    assert {r["pos"] - pc.R0 for r in te["gaps"][3]} >= {-1, -600} and any(r["mapq"] == 0 for r in te["gaps"][3])
    assert all({True, False} == {r["reverse"] for r in case[3]} for case in te.values())
    assert len(te["all"][3]) == sum(len(c[3]) for n, c in te.items() if n != "all")
    assert len(families["spans"]["all"][4]) == 8
    assert [c[1] - c[0] + 1 for c in families["scan_edges"].values()] == list(pc.SCAN_LENGTHS)
    mr = families["many_regions"]
    assert len(mr) == 1100 and {c[1] - c[0] + 1 for c in mr.values()} == {1, 2, 3} and {len(c[3]) for c in mr.values()} >= {0, 1, 2, 3}
    # capacity: more insert slots than 2 * rows + 4096; more tile records than bases / 512 + 2 * reads + 1024
    a, b = families["capacity"]["long_inserts"], families["capacity"]["many_records"]
    assert sum(sorted(n for r in a[3] for op, n in r["cigar"] if op == pc.I)[-2:]) == 6000 > 2 * 200 + 4096
    crossings = sum(1 for r in b[3] for i, op, first, n in _walk(r, b[0]) if n > 0 and (first + n - 1) // 512 > max(first, 0) // 512)
    assert crossings > sum(len(r["seq"]) for r in b[3]) // 512 + 2 * len(b[3]) + 1024
