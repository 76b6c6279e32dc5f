"""min_quality polish on the host (pepper_amd/polish/Stitch.py gate_numpy, through create_consensus_sequence and perform_stitch):
only the edits whose winning prediction has phred >= Q are applied, the draft's letter stands elsewhere.  One small case is written
out by hand -- sequence, qualities, applied and withheld records -- so the twin is not only held to itself; larger tables are held
to the rule's invariants: the applied records are the ungated ones filtered by the rule, and replaying them over the draft gives
the gated sequence."""
import os

import numpy as np
import pytest

import polish_edits_cases as cases
from pepper_amd.polish import Edits, Stitch
from pepper_amd.polish.DataStorePredict import DataStore
from pepper_amd.polish.Stitch import create_consensus_sequence
from pepper_amd.polish.perform_stitch import perform_stitch

A, C, G, T = (ord(c) for c in "ACGT")
N = ord("N")
SUFFIXES = ("_pepper_polished.fa", "_pepper_polished.fastq", "_pepper_polished.edits.tsv", "_pepper_polished.withheld.tsv")

# ---- the case written out by hand: Q = 20 ----
HAND_DRAFT = "ACGTNACgTACnA"
HAND_TABLE = {
    (0, 0): (1, 40),        # A on A: untouched, keeps its phred
    (1, 0): (3, 19),        # G on C, 19: SUB withheld -> C, '!'
    (2, 0): (4, 20),        # T on G, 20: SUB applied
    (3, 0): (0, 19),        # gap on T, 19: DEL withheld -> T, '!'
    (3, 1): (1, 19),        # INS A, 19: withheld -> nothing
    (3, 2): (2, 20),        # INS C, 20: applied
    (4, 0): (2, 5),         # C on N, 5: the draft letter is no base, the model's decision stands
    (5, 0): (0, 20),        # gap on A, 20: DEL applied
    (6, 1): (3, 50),        # INS G, 50: applied; (6, 0) has no writer: a DEL with phred 0, withheld -> C, '!'
    (7, 0): (3, 7),         # G on g: equal after upper-casing, untouched whatever its phred
    (8, 0): (1, 3),         # A on T, 3: SUB withheld -> T, '!'
    #  9: no slot at all: dropped as ever (a GAP pair)
    (10, 0): (2, 30),       # C on C
    (11, 0): (0, 1),        # gap on n, 1: the draft letter is no base, the DEL stands
    (12, 0): (1, 40),       # A on A
}
HAND_SEQUENCE = "ACTTCCCGGTCA"
HAND_QUALITY = "I!5!5&!S(!?I"
#               position, offset, index, piece, kind, draft, letter, phred
HAND_APPLIED = [(2, 2, 0, 0, 1, G, T, 20), (3, 4, 2, 0, 3, 0, C, 20), (4, 5, 0, 0, 1, N, C, 5), (5, 6, 0, 0, 2, A, 0, 20),
                (6, 7, 1, 0, 3, 0, G, 50), (9, 10, 0, 0, 4, A, 0, 0), (9, 10, 0, 0, 5, A, 0, 0), (11, 11, 0, 0, 2, N, 0, 1)]
HAND_WITHHELD = [(1, 1, 0, 0, 1, C, G, 19), (3, 3, 0, 0, 2, T, 0, 19), (3, 4, 1, 0, 3, 0, A, 19), (6, 6, 0, 0, 2, C, 0, 0),
                 (8, 9, 0, 0, 1, T, A, 3)]
HAND_TSV = ("#contig\tdraft_position\tinsert_index\tkind\tdraft\tmodel\tphred\tpolished_offset\n"
            "ctg\t1\t0\tsub\tC\tG\t19\t1\nctg\t3\t0\tdel\tT\t-\t19\t3\nctg\t3\t1\tins\t-\tA\t19\t4\nctg\t6\t0\tdel\tC\t-\t0\t6\n"
            "ctg\t8\t0\tsub\tT\tA\t3\t9\n")


def _arrays(table):
    keys = sorted(table)
    return (np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
            np.array([table[k][0] for k in keys], np.int64), np.array([table[k][1] for k in keys], np.int64))


def _write_table(pred, contig, table, chunk=5):
    os.makedirs(str(pred), exist_ok=True)
    with DataStore(str(pred / "p.hdf"), "w") as store:
        cases.write_region(store, contig, 0, 100, _arrays(table), chunk=chunk)


def _gate(table, draft, q, filled=False):
    """The numpy gate on a table -> (positions, indices, labels, phred, withheld)."""
    positions, indices, labels, phred = Stitch.with_empty_slots(*_arrays(table))
    labels, phred, withheld = Stitch.gate_numpy(positions, indices, labels, phred, draft, q, filled=filled)
    return positions, indices, labels, phred, withheld


def test_the_case_written_out_by_hand(tmp_path):
    positions, indices, labels, phred, withheld = _gate(HAND_TABLE, HAND_DRAFT, 20)
    letters = Stitch._DECODE[labels]
    assert letters[letters != 0].tobytes().decode() == HAND_SEQUENCE
    assert (33 + np.minimum(phred[letters != 0], 93)).astype(np.uint8).tobytes().decode() == HAND_QUALITY
    assert cases.as_tuples(withheld) == HAND_WITHHELD
    applied = Edits.records_numpy(positions, indices, labels, phred, HAND_DRAFT)
    assert cases.as_tuples(applied) == HAND_APPLIED
    assert Edits.apply(HAND_DRAFT, applied, [(0, 12, 12)]) == HAND_SEQUENCE
    # through the files: one region, chunks of 5 rows
    _write_table(tmp_path / "pred", "ctg", HAND_TABLE)
    draft_fa = cases.write_draft(tmp_path / "draft.fa", {"ctg": HAND_DRAFT})
    keys = cases.contig_keys(tmp_path / "pred", "ctg")
    sequence, quality, records, pieces, held = create_consensus_sequence("ctg", keys, 1, qualities=True, edits=draft_fa, min_quality=20,
                                                                         draft=draft_fa)
    assert (sequence, quality, pieces) == (HAND_SEQUENCE, HAND_QUALITY, [(0, 12, 12)])
    assert cases.as_tuples(records) == HAND_APPLIED and cases.as_tuples(held) == HAND_WITHHELD
    assert create_consensus_sequence("ctg", keys, 1, min_quality=20, draft=draft_fa)[0] == HAND_SEQUENCE
    perform_stitch(str(tmp_path / "pred"), str(tmp_path / "out" / "asm"), 1, qualities=True, edits=draft_fa, min_quality=20, draft=draft_fa)
    fasta, fastq, tsv, withheld_tsv = (open(str(tmp_path / "out" / "asm") + suffix).read() for suffix in SUFFIXES)
    assert fasta == ">ctg\n" + HAND_SEQUENCE + "\n" and fastq == "@ctg\n" + HAND_SEQUENCE + "\n+\n" + HAND_QUALITY + "\n"
    assert withheld_tsv == HAND_TSV
    assert tsv.splitlines()[-1].split("\t")[-1] == "withheld=5"


def test_the_hand_case_filled(tmp_path):
    """With fill the one uncovered position (9) gives the draft's letter, and every offset behind it counts it."""
    positions, indices, labels, phred, withheld = _gate(HAND_TABLE, HAND_DRAFT, 20, filled=True)
    assert cases.as_tuples(withheld) == HAND_WITHHELD                # (all of them lie in front of position 9)
    _write_table(tmp_path / "pred", "ctg", HAND_TABLE)
    draft_fa = cases.write_draft(tmp_path / "draft.fa", {"ctg": HAND_DRAFT})
    sequence, quality, records, pieces, held = create_consensus_sequence("ctg", cases.contig_keys(tmp_path / "pred", "ctg"), 3,
                                                                         qualities=True, edits=draft_fa, fill=draft_fa, min_quality=20,
                                                                         draft=draft_fa)
    assert sequence == HAND_SEQUENCE[:10] + "A" + HAND_SEQUENCE[10:] and quality == HAND_QUALITY[:10] + "!" + HAND_QUALITY[10:]
    assert pieces == [(0, 12, 13)] and cases.as_tuples(held) == HAND_WITHHELD
    assert Edits.apply_filled(HAND_DRAFT, records, pieces) == sequence
    assert [int(o) for o in records["offset"][-1:]] == [12]          # the DEL at 11 lies behind the filled letter


def _applied_by_the_rule(ungated, q):
    """The ungated records the rule keeps: the GAP kinds, SUB / DEL / INS with phred >= q, SUB / DEL on a draft letter outside ACGT."""
    kind, phred, draft = ungated["kind"], ungated["phred"], ungated["draft"]
    no_base = ~np.isin(draft, np.frombuffer(b"ACGT", np.uint8))
    return ungated[(kind >= Edits.GAP_OPEN) | (phred >= q) | ((kind != Edits.INS) & no_base)]


def _without_offset(records):
    records = records.copy()
    records["offset"] = 0
    return records.tobytes()


def _big_table(rng, draft, a, b):
    """Every kind of edit at every phred around the thresholds, an empty (p, 0) beside insert slots, 300 insert slots at one
    position, uncovered runs."""
    table = {(p, 0): (cases.CODE.get(draft[p].upper(), 1), int(rng.integers(0, 256))) for p in range(a, b)}
    for k, p in enumerate(range(a + 3, b - 3, 5)):
        phred = (0, 1, 19, 20, 21, 254, 255)[k % 7]
        if k % 3 == 0:
            table[(p, 0)] = (cases.other(draft[p], 1 + k % 3), phred)
        elif k % 3 == 1:
            table[(p, 0)] = (0, phred)
        else:
            table[(p, 1 + k % 2)] = (1 + k % 4, phred)
    mid = (a + b) // 2
    for i in range(1, 301):
        if i % 7:
            table[(mid, i)] = (int(rng.integers(0, 5)), i % 256)
    del table[(mid + 11, 0)]
    table[(mid + 11, 2)] = (2, 200)                                  # (p, 0) and (p, 1) have no writer
    for p in range(mid + 20, mid + 31):
        table.pop((p, 0), None)
        table.pop((p, 1), None)
        table.pop((p, 2), None)
    return table


def _marked_draft(rng, n):
    draft = list(cases.random_draft(rng, n))
    for p in rng.integers(0, n, n // 5).tolist():
        draft[p] = draft[p].lower()
    for p in rng.integers(0, n, n // 12 + 1).tolist():
        draft[p] = "N" if p % 2 else "n"
    return ''.join(draft)


@pytest.mark.parametrize("q", [1, 19, 20, 21, 255])
def test_the_rule_on_a_large_table(q):
    rng = np.random.default_rng(q)
    draft = _marked_draft(rng, 900)
    table = _big_table(rng, draft, 20, 880)
    positions, indices, labels, phred, withheld = _gate(table, draft, q)
    ungated = Edits.records_numpy(*_arrays(table), draft)
    applied = Edits.records_numpy(positions, indices, labels, phred, draft)
    want = _applied_by_the_rule(ungated, q)
    for kind in range(1, 6):
        assert _without_offset(applied[applied["kind"] == kind]) == _without_offset(want[want["kind"] == kind])
    # what is withheld is the rest of the ungated records: kind, key, letters and phred
    rest = ungated[(ungated["kind"] < Edits.GAP_OPEN) & ~((ungated["phred"] >= q) | ((ungated["kind"] != Edits.INS) &
                   ~np.isin(ungated["draft"], np.frombuffer(b"ACGT", np.uint8))))]
    assert _without_offset(withheld) == _without_offset(rest) and (len(withheld) > 50 or q == 1)
    letters = Stitch._DECODE[labels]
    sequence = letters[letters != 0].tobytes().decode()
    assert Edits.apply(draft, applied, [(20, 879, len(sequence))]) == sequence
    # a withheld SUB or DEL stands on its kept draft letter, a withheld INS in front of the next letter
    upper = draft.upper()
    for r in withheld[withheld["kind"] != Edits.INS]:
        assert sequence[int(r["offset"])] == upper[int(r["position"])] == chr(r["draft"])
    for r in withheld[withheld["kind"] == Edits.INS]:                # (sorted keys: offsets never go down)
        assert 0 <= int(r["offset"]) <= len(sequence)
    assert np.all(np.diff(withheld["offset"].astype(np.int64)) >= 0)
    if q == 1:                                                       # only the slots without a writer lie below phred 1 ...
        assert set(withheld["phred"].tolist()) <= {0}
    if q == 255:                                                     # ... and at 255 only phred 255 itself is applied
        gateable = applied[(applied["kind"] < Edits.GAP_OPEN) & np.isin(applied["draft"], np.frombuffer(b"ACGT\0", np.uint8))]
        assert len(gateable) > 0 and set(gateable["phred"].tolist()) == {255}


def _files(where):
    return tuple(open(str(where) + suffix).read() if os.path.exists(str(where) + suffix) else None for suffix in SUFFIXES)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gate_planted")
    drafts = cases.write_planted(tmp / "pred")
    return tmp, cases.write_draft(tmp / "draft.fa", drafts), drafts


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("threads", [1, 3])
def test_perform_stitch_on_the_planted_files(planted, fill, threads):
    tmp, draft_fa, drafts = planted
    pred, draft = tmp / "pred", drafts["ctg"]
    tag = "f%d_t%d" % (fill, threads)
    kw = dict(fill=draft_fa) if fill else {}
    perform_stitch(str(pred), str(tmp / tag / "asm"), threads, qualities=True, edits=draft_fa, min_quality=20, draft=draft_fa, **kw)
    fasta, fastq, tsv, withheld_tsv = _files(tmp / tag / "asm")
    sequence, quality, records, pieces, held = create_consensus_sequence("ctg", cases.contig_keys(pred, "ctg"), threads, qualities=True,
                                                                         edits=draft_fa, min_quality=20, draft=draft_fa, **kw)
    assert fasta == ">ctg\n" + sequence + "\n" and fastq == "@ctg\n" + sequence + "\n+\n" + quality + "\n"
    replay = Edits.apply_filled if fill else Edits.apply
    assert replay(draft, records, pieces) == sequence
    # the planted edits below 20: SUB at 20 (phred 0), SUB INS INS SUB at 50 / 51 (11, 12, 13, 9), DEL at 300 (5), and the empty
    # (90, 0) under a filled (90, 1) (phred 0); piece 0 begins at position 10, so without fill the offset of position 20 is 10
    lines = withheld_tsv.splitlines()
    d = draft.upper()
    assert lines[0] + "\n" == Edits.WITHHELD_HEADER
    assert lines[1] == "ctg\t20\t0\tsub\t%s\t%s\t0\t%d" % (d[20], "ACGT"[cases.other(draft[20]) - 1], 20 if fill else 10)
    assert [(line.split("\t")[1], line.split("\t")[3]) for line in lines[1:]] == [
        ("20", "sub"), ("50", "sub"), ("50", "ins"), ("50", "ins"), ("51", "sub"), ("90", "del"), ("300", "del")]
    assert len(held) == 7 and (sequence[int(held[5]["offset"])], sequence[int(held[6]["offset"])]) == (d[90], d[300])
    summary = tsv.splitlines()[-1]
    assert summary.startswith("##contig=ctg\t") and summary.split("\t")[-1] == "withheld=7"
    # the other files of the run do not depend on which of them were asked for
    perform_stitch(str(pred), str(tmp / (tag + "_bare") / "asm"), threads, min_quality=20, draft=draft_fa, **kw)
    assert _files(tmp / (tag + "_bare") / "asm") == (fasta, None, None, withheld_tsv)
    perform_stitch(str(pred), str(tmp / (tag + "_q") / "asm"), threads, qualities=True, min_quality=20, draft=draft_fa, **kw)
    assert _files(tmp / (tag + "_q") / "asm") == (fasta, fastq, None, withheld_tsv)
    # the lowest gate: only phred 0 lies below it -- the SUB at 20, which was written with phred 0, and the empty slot (90, 0)
    perform_stitch(str(pred), str(tmp / (tag + "_q1") / "asm"), threads, qualities=True, edits=draft_fa, min_quality=1, draft=draft_fa, **kw)
    assert [line.split("\t")[1] for line in _files(tmp / (tag + "_q1") / "asm")[3].splitlines()[1:]] == ["20", "90"]


@pytest.mark.parametrize("off", [0, None])
def test_off_is_byte_identical_and_writes_no_withheld_file(planted, off):
    tmp, draft_fa, _ = planted
    for k, kw in enumerate((dict(), dict(qualities=True, edits=draft_fa), dict(qualities=True, edits=draft_fa, fill=draft_fa))):
        plain, gated = tmp / ("plain%d_%s" % (k, off)) / "asm", tmp / ("off%d_%s" % (k, off)) / "asm"
        perform_stitch(str(tmp / "pred"), str(plain), 3, **kw)
        perform_stitch(str(tmp / "pred"), str(gated), 3, min_quality=off, draft=draft_fa, **kw)
        assert _files(plain) == _files(gated) and _files(gated)[3] is None and _files(gated)[0]


@pytest.mark.parametrize("bad", [-1, 256, 3.5])
def test_values_outside_the_range_are_refused(planted, bad):
    tmp, draft_fa, _ = planted
    with pytest.raises(ValueError):
        perform_stitch(str(tmp / "pred"), str(tmp / "bad" / "asm"), 1, min_quality=bad, draft=draft_fa)
    with pytest.raises(ValueError):
        create_consensus_sequence("ctg", cases.contig_keys(tmp / "pred", "ctg"), 1, min_quality=bad, draft=draft_fa)


def test_a_gate_needs_its_draft(planted):
    tmp, draft_fa, _ = planted
    with pytest.raises(ValueError):
        perform_stitch(str(tmp / "pred"), str(tmp / "nodraft" / "asm"), 1, min_quality=20)
