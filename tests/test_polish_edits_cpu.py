"""perform_stitch(..., edits=<draft FASTA>): the records of the numpy twin (pepper_amd/polish/Edits.records_numpy) against a literal
restatement -- polish_edits_cases.dict_records, a dictionary loop over the keys -- the hunks and the text made from them, and the
round trip that needs no twin: Edits.apply(draft, records, pieces) is the consensus perform_stitch writes.  No GPU."""
import inspect
import os

import numpy as np
import pytest

import polish_edits_cases as cases
import test_polish_qualities_cpu as qcases
from pepper_amd import _lib
from pepper_amd.polish import Edits
from pepper_amd.polish.perform_stitch import perform_stitch


def _lines(tsv, contig="ctg"):
    """The hunk lines of one contig as tuples of columns (without the contig), and its summary line as a dict."""
    assert tsv.startswith(Edits.HEADER)
    hunks, summary = [], None
    for line in tsv[len(Edits.HEADER):].splitlines():
        cols = line.split("\t")
        if cols[0] == "##contig=" + contig:
            summary = dict(c.split("=") for c in cols[1:])
        elif cols[0] == contig:
            hunks.append(tuple(cols[1:]))
    return hunks, summary


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("edits_planted")
    drafts = cases.write_planted(tmp / "pred")
    return tmp / "pred", cases.write_draft(tmp / "draft.fa", drafts), drafts["ctg"], tmp


@pytest.mark.parametrize("threads", [1, 3])
def test_planted_records_and_round_trip(planted, threads):
    pred, draft_fa, draft, tmp = planted
    fasta, tsv = cases.host_texts(pred, draft_fa, tmp / ("o%d" % threads) / "asm", threads)
    sequence, records, pieces = cases.check_contig(pred, draft_fa, draft, "ctg", threads, cases.fasta_sequences(fasta)["ctg"])
    assert pieces == ([(10, 350, len(sequence))] if threads == 1 else [(10, 180, pieces[0][2]), (170, 350, pieces[1][2])])
    kinds = records["kind"].tolist()
    assert {1, 2, 3, 4, 5} <= set(kinds) and kinds.count(4) == kinds.count(5) == 2
    assert {0, 100, 255} <= set(records["phred"].tolist())
    by_key = {(int(r["position"]), int(r["index"]), int(r["kind"])): r for r in records if r["piece"] == 0}
    assert chr(by_key[(72, 0, 1)]["draft"]) == draft[72].upper() != draft[72]              # a lower-case draft letter
    assert all((p, 0, 1) not in by_key for p in (70, 71, 73, 74, 75))                      # ... that matches gives nothing
    assert chr(by_key[(80, 0, 1)]["draft"]) == "N" and (81, 0, 2) in by_key and chr(by_key[(83, 0, 1)]["draft"]) == "N"
    assert by_key[(90, 0, 2)]["phred"] == 0 and (90, 1, 3) in by_key                       # the empty slot under a filled one
    assert not any(k[0] in (95, 96) for k in by_key if k[2] != 3) and (96, 2, 3) in by_key and (95, 1, 3) not in by_key
    assert (120, 0, 4) in by_key and (120, 0, 5) in by_key                                 # a one-position gap: both records
    assert by_key[(120, 0, 4)]["offset"] == by_key[(120, 0, 5)]["offset"]


def test_planted_hunks_and_text(planted):
    pred, draft_fa, draft, tmp = planted
    _, tsv1 = cases.host_texts(pred, draft_fa, tmp / "h1" / "asm", 1)
    _, tsv3 = cases.host_texts(pred, draft_fa, tmp / "h3" / "asm", 3)
    sequence, records, pieces = cases.host_records(pred, draft_fa, "ctg", 1)
    hunks, summary = _lines(tsv1)
    by_start = {(int(h[0]), h[4]): h for h in hunks}
    letters = lambda a, b: sequence[int(a):int(b)] or "."
    for h in hunks:                                                  # every line's columns are what its coordinates name
        if h[4] not in ("uncovered", "duplicated"):
            assert h[5] == (draft[int(h[0]):int(h[1])].upper() or ".") and h[6] == letters(h[2], h[3]), h
        else:
            assert h[5:] == (".", ".", ".") and h[2] == h[3]
    assert by_start[(0, "uncovered")][:2] == ("0", "10") and by_start[(351, "uncovered")][:2] == ("351", "400")
    assert by_start[(120, "uncovered")][:2] == ("120", "121") and by_start[(261, "uncovered")][:2] == ("261", "280")
    assert by_start[(50, "complex")][:2] == ("50", "52") and len(by_start[(50, "complex")][6]) == 4 and by_start[(50, "complex")][7] == "9"
    assert by_start[(60, "del")][:2] == ("60", "61") and by_start[(62, "del")][:2] == ("62", "63")          # a match between: two hunks
    assert by_start[(130, "sub")][:2] == ("130", "133") and by_start[(130, "sub")][7] == "40"
    assert by_start[(141, "ins")][:2] == ("141", "141") and by_start[(141, "ins")][6] == "ACG" and by_start[(141, "ins")][7] == "70"
    assert by_start[(150, "del")][:2] == ("150", "152") and by_start[(150, "del")][5] == draft[150:152]
    assert by_start[(20, "sub")][7] == "0" and by_start[(30, "del")][7] == "100" and by_start[(41, "ins")][7] == "255"
    # DEL (90, 0) + INS (90, 1): one hunk, and equal lengths make it a `sub`; the empty slot's phred is 0
    assert by_start[(90, "sub")][:2] == ("90", "91") and by_start[(90, "sub")][6:] == ("T", "0")
    assert not any(h[4] == "duplicated" for h in hunks)
    assert int(summary["draft_length"]) == 400 and int(summary["polished_length"]) == len(sequence)
    assert int(summary["uncovered"]) == 10 + 1 + 19 + 49 and int(summary["duplicated"]) == 0
    # threads 3: the same draft, two pieces that overlap in [170, 181)
    hunks3, summary3 = _lines(tsv3)
    dup = [h for h in hunks3 if h[4] == "duplicated"]
    _, _, pieces3 = cases.host_records(pred, draft_fa, "ctg", 3)
    assert dup == [("170", "181", str(pieces3[0][2]), str(pieces3[0][2]), "duplicated", ".", ".", ".")]
    assert int(summary3["duplicated"]) == 11 and int(summary3["polished_length"]) == pieces3[0][2] + pieces3[1][2]
    assert [h for h in hunks3 if int(h[1]) <= 170] == [h for h in hunks if int(h[1]) <= 170]


def test_pieces_apart(tmp_path):
    """The second piece starts at 190: (180, 190) is an inter-piece `uncovered` hunk with threads 3, a gap inside the one piece
    with threads 1 -- the same line either way."""
    drafts = cases.write_planted(tmp_path / "pred", second_from=190)
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    found = []
    for threads in (1, 3):
        fasta, tsv = cases.host_texts(tmp_path / "pred", draft_fa, tmp_path / ("o%d" % threads) / "asm", threads)
        _, records, pieces = cases.check_contig(tmp_path / "pred", draft_fa, drafts["ctg"], "ctg", threads, cases.fasta_sequences(fasta)["ctg"])
        found.append((_lines(tsv), len(pieces), int((records["kind"] == 4).sum())))
    assert found[0][0] == found[1][0] and ("181", "190") in [h[:2] for h in found[0][0][0] if h[4] == "uncovered"]
    assert (found[0][1], found[0][2]) == (1, 3) and (found[1][1], found[1][2]) == (2, 2)


def test_hunks_without_qualities_and_apply_alone():
    """Records written by hand: min_phred is '.' for a contig without qualities; apply needs nothing but the records."""
    draft = "acgtNACGTAC"
    records = np.array([(1, 1, 0, 0, 1, ord("C"), ord("T"), 0), (1, 2, 1, 0, 3, 0, ord("G"), 0), (3, 4, 0, 0, 2, ord("T"), 0, 0),
                        (5, 5, 0, 0, 4, ord("A"), 0, 0), (5, 5, 0, 0, 5, ord("A"), 0, 0), (8, 7, 0, 1, 1, ord("T"), ord("A"), 0)],
                       Edits.EDIT_DTYPE)
    pieces = [(0, 6, 6), (7, 9, 3)]
    assert Edits.apply(draft, records, pieces) == "ATGG" + "N" + "C" + "GAA"
    assert Edits.hunks(records, pieces, len(draft), False) == [
        (1, 2, 1, 3, "complex", "C", "TG", "."), (3, 4, 4, 4, "del", "T", ".", "."), (5, 6, 5, 5, "uncovered", ".", ".", "."),
        (8, 9, 7, 8, "sub", "T", "A", "."), (10, 11, 9, 9, "uncovered", ".", ".", ".")]
    assert Edits.hunks(records, pieces, len(draft), True)[0][7] == "0"
    assert Edits.hunks(np.zeros(0, Edits.EDIT_DTYPE), [], 5, True) == [(0, 5, 0, 0, "uncovered", ".", ".", ".")]


def test_golden_inputs(golden_dir, tmp_path):
    """The reference's golden stitch inputs against a draft derived from the golden consensus: the FASTA's bytes do not change."""
    pred = tmp_path / "pred"
    qcases.write_golden(golden_dir, pred)
    want = open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read()
    drafts = cases.golden_draft(golden_dir)
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    for threads in (1, 2):
        fasta, tsv = cases.host_texts(pred, draft_fa, tmp_path / ("o%d" % threads) / "asm", threads)
        assert fasta == want
        sequences = cases.fasta_sequences(fasta)
        assert [line.split("\t")[0][9:] for line in tsv.splitlines() if line.startswith("##contig=")] == list(sequences)
        for contig, sequence in sequences.items():
            _, records, _ = cases.check_contig(pred, draft_fa, drafts[contig], contig, threads, sequence)
            assert len(records) > 10


def test_off_changes_nothing(planted):
    pred, draft_fa, _, tmp = planted
    fasta, _ = cases.host_texts(pred, draft_fa, tmp / "on" / "asm", 3)
    assert sorted(os.listdir(str(tmp / "on"))) == ["asm_pepper_polished.edits.tsv", "asm_pepper_polished.fa"]
    for name, kw in (("off", {}), ("off2", {"edits": None})):
        out = perform_stitch(str(pred), str(tmp / name / "asm"), 3, **kw)
        assert open(out).read() == fasta and os.listdir(os.path.dirname(out)) == ["asm_pepper_polished.fa"]
    out = perform_stitch(str(pred), str(tmp / "both" / "asm"), 3, qualities=True, edits=draft_fa)
    assert open(out).read() == fasta
    assert open(str(tmp / "both" / "asm") + "_pepper_polished.edits.tsv").read() == open(str(tmp / "on" / "asm") + "_pepper_polished.edits.tsv").read()
    assert open(str(tmp / "both" / "asm") + "_pepper_polished.fastq").read() == \
        qcases.host_texts(pred, tmp / "q" / "asm", 3)[1]


def test_short_draft_is_refused(planted):
    pred, _, draft, tmp = planted
    short = cases.write_draft(tmp / "short.fa", {"ctg": draft[:350]})
    with pytest.raises(ValueError, match="no letter at position 350"):
        perform_stitch(str(pred), str(tmp / "short" / "asm"), 1, edits=short)
    other = cases.write_draft(tmp / "other.fa", {"another": draft})
    with pytest.raises(KeyError):
        perform_stitch(str(pred), str(tmp / "other" / "asm"), 1, edits=other)


def test_signatures_and_switch(monkeypatch):
    from pepper_amd.polish import Stitch
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
    from pepper_amd.polish.polish import polish
    for fn in (polish, perform_stitch, Stitch.small_chunk_stitch, Stitch.small_chunk_stitch_numpy, Stitch.create_consensus_sequence,
               stitch_directory, DeviceStitcher.write_fasta, DeviceStitcher.write_fastq):
        assert inspect.signature(fn).parameters["edits"].default is None, fn
    assert list(inspect.signature(DeviceStitcher.edits).parameters) == ["self", "draft_sequence"]
    assert list(inspect.signature(Edits.hunks).parameters) == ["records", "pieces", "draft_length", "has_qualities"]
    assert list(inspect.signature(Edits.apply).parameters) == ["draft_sequence", "records", "pieces"]
    assert Edits.EDIT_DTYPE.itemsize == 16 and Edits.EDIT_DTYPE.names == ("position", "offset", "index", "piece", "kind", "draft",
                                                                          "letter", "phred")
    assert [Edits.EDIT_DTYPE.fields[n][1] for n in Edits.EDIT_DTYPE.names] == [0, 4, 8, 10, 12, 13, 14, 15]
    monkeypatch.delenv("PEPPER_AMD_POLISH_EDITS", raising=False)
    assert _lib.polish_edits() is False
    monkeypatch.setenv("PEPPER_AMD_POLISH_EDITS", "1")
    assert _lib.polish_edits() is True
    monkeypatch.setenv("PEPPER_AMD_POLISH_EDITS", "yes")
    assert _lib.polish_edits() is False
    assert _lib.POLISH_EDITS_ENV == "PEPPER_AMD_POLISH_EDITS"
    assert {"pa_stitcher_edits", "pa_stitcher_take_edits"} <= {name for name, _, _ in _lib.SYMBOLS}


def test_new_symbols_load_and_refuse_a_null_handle():
    from pepper_amd import build
    build.build()
    lib = _lib.load()
    assert lib.pa_stitcher_edits(None, None, 0, None, None) == _lib.PA_ERR_INVALID
    assert lib.pa_stitcher_take_edits(None, None, 0) == _lib.PA_ERR_INVALID
