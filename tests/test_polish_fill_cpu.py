"""perform_stitch(..., fill=<draft FASTA>): the filled consensus of the host form, held to properties that need no twin -- with
its filled runs cut out it is the threads=1 consensus of today, it does not depend on `threads`, Edits.apply_filled(draft, records,
pieces) gives it back, and its length is what the summary line adds up to.  No GPU."""
import inspect
import io
import os

import numpy as np
import pytest

import polish_edits_cases as cases
import test_polish_qualities_cpu as qcases
from pepper_amd import _lib
from pepper_amd.polish import Edits
from pepper_amd.polish.Stitch import create_consensus_sequence
from pepper_amd.polish.perform_stitch import perform_stitch

SUFFIXES = ("_pepper_polished.fa", "_pepper_polished.fastq", "_pepper_polished.edits.tsv")


def fill_texts(pred, draft_fa, where, threads, **kw):
    """(FASTA, FASTQ, .edits.tsv) of perform_stitch with everything on."""
    kw = dict(dict(qualities=True, edits=str(draft_fa), fill=str(draft_fa)), **kw)
    perform_stitch(str(pred), str(where), threads, **kw)
    return tuple(open(str(where) + suffix).read() for suffix in SUFFIXES)


def tsv_lines(tsv, contig):
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


def fastq_records(text):
    lines = text.splitlines()
    assert all(line == "+" for line in lines[2::4])
    return {name[1:]: (sequence, quality) for name, sequence, quality in zip(lines[0::4], lines[1::4], lines[3::4])}


def cut_runs(sequence, hunks):
    """The sequence without the polished intervals of its `filled` hunks."""
    out, at = [], 0
    for h in hunks:
        if h[4] == "filled":
            assert int(h[3]) - int(h[2]) == int(h[1]) - int(h[0]) > 0 and h[5:] == (".", ".", ".")
            out.append(sequence[at:int(h[2])])
            at = int(h[3])
    return ''.join(out) + sequence[at:]


def check_filled_contig(pred, draft_fa, draft, contig, texts, unfilled):
    """Invariants (a), (c), (d) and the letters, qualities and offsets of one contig of a filled run.  unfilled: the threads=1
    consensus of today (None: the contig has no prediction)."""
    fasta, fastq, tsv = texts
    sequence = cases.fasta_sequences(fasta)[contig]
    assert fastq_records(fastq)[contig][0] == sequence
    quality = fastq_records(fastq)[contig][1]
    hunks, summary = tsv_lines(tsv, contig)
    assert not any(h[4] in ("uncovered", "duplicated") for h in hunks)
    assert int(summary["uncovered"]) == int(summary["duplicated"]) == 0 and list(summary)[-1] == "filled"
    # (a) the runs cut out: today's threads=1 consensus
    assert cut_runs(sequence, hunks) == (unfilled or "")
    # the filled letters are the draft's as stored, their qualities '!'
    filled = 0
    for h in hunks:
        if h[4] == "filled":
            d0, d1, o0, o1 = (int(v) for v in h[:4])
            assert sequence[o0:o1] == draft[d0:d1] and quality[o0:o1] == "!" * (o1 - o0)
            filled += d1 - d0
        else:                                                        # the columns are what the coordinates name
            assert h[5] == (draft[int(h[0]):int(h[1])].upper() or ".") and h[6] == (sequence[int(h[2]):int(h[3])] or ".")
    assert int(summary["filled"]) == filled
    # (d) the length
    assert len(sequence) == int(summary["polished_length"]) == int(summary["draft_length"]) - int(summary["del"]) - \
        int(summary["complex_draft"]) + int(summary["ins"]) + int(summary["complex_polished"])
    assert int(summary["draft_length"]) == len(draft)
    # (c) the records give it back, and name their own letters
    if unfilled is None:
        assert sequence == draft and Edits.apply_filled(draft, np.zeros(0, Edits.EDIT_DTYPE), []) == draft
        return sequence
    got, got_quality, records, pieces = create_consensus_sequence(contig, cases.contig_keys(pred, contig), 5, qualities=True,
                                                                  edits=str(draft_fa), fill=str(draft_fa))
    assert (got, got_quality) == (sequence, quality) and len(pieces) == 1 and pieces[0][2] == len(sequence)
    assert Edits.apply_filled(draft, records, pieces) == sequence
    own = (records["kind"] == Edits.SUB) | (records["kind"] == Edits.INS)
    assert [sequence[o] for o in records["offset"][own].tolist()] == [chr(c) for c in records["letter"][own].tolist()]
    text = io.StringIO()
    Edits.write_contig(text, contig, records, pieces, len(draft), True, filled=True)
    assert Edits.HEADER + text.getvalue() == ''.join(line + "\n" for line in tsv.splitlines()
                                                     if line.startswith(("#contig", contig + "\t", "##contig=" + contig + "\t")))
    assert Edits.filled_hunks(records, pieces, len(draft), True) == [
        tuple(int(v) for v in h[:4]) + h[4:] for h in hunks]
    return sequence


def planted_with_marks(pred, second_from=170):
    """cases.write_planted with lower-case letters and Ns where no row covers the draft: 0..9, 261..279, 351..399 (and 120)."""
    draft = list(cases.write_planted(pred, second_from)["ctg"])
    for p in (0, 3, 9, 120, 261, 270, 279, 351, 399):
        draft[p] = draft[p].lower()
    for p in (5, 265, 360):
        draft[p] = 'N'
    draft[266] = 'n'
    return {"ctg": ''.join(draft)}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fill_planted")
    drafts = planted_with_marks(tmp / "pred")
    return tmp / "pred", cases.write_draft(tmp / "draft.fa", drafts), drafts["ctg"], tmp


@pytest.mark.parametrize("second_from", [170, 190])
def test_planted_runs_cut_out_apply_and_length(tmp_path, second_from):
    """(a), (c), (d), (f) on the planted case: a leading run, a run of one position, one of 19 (and one of 9 with pieces apart),
    a trailing run."""
    drafts = planted_with_marks(tmp_path / "pred", second_from)
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    unfilled = cases.fasta_sequences(open(perform_stitch(str(tmp_path / "pred"), str(tmp_path / "u" / "asm"), 1)).read())["ctg"]
    texts = fill_texts(tmp_path / "pred", draft_fa, tmp_path / "f" / "asm", 3)
    sequence = check_filled_contig(tmp_path / "pred", draft_fa, drafts["ctg"], "ctg", texts, unfilled)
    hunks, summary = tsv_lines(texts[2], "ctg")
    runs = [(h[0], h[1]) for h in hunks if h[4] == "filled"]
    assert runs == [("0", "10"), ("120", "121")] + ([("181", "190")] if second_from == 190 else []) + [("261", "280"), ("351", "400")]
    assert int(summary["filled"]) == 10 + 1 + 19 + 49 + (9 if second_from == 190 else 0)
    # (f) lower case and N survive in the runs, and only there
    draft = drafts["ctg"]
    assert sequence[:10] == draft[:10] and sequence[:10] != draft[:10].upper() and sequence[5] == "N"
    assert sequence[-49:] == draft[351:] and sequence[-40] == "N" and sequence[-1].islower()
    run = int([h for h in hunks if h[0] == "261"][0][2])
    assert sequence[run:run + 19] == draft[261:280] and sequence[run + 4:run + 6] == "Nn"
    covered = cut_runs(sequence, hunks)
    assert covered == covered.upper() and "N" not in covered


def test_threads_do_not_shape_the_filled_files(planted):
    """(b) regions that overlap: today's files differ between thread counts and show a `duplicated` hunk; the filled ones do not."""
    pred, draft_fa, _, tmp = planted
    today = {t: fill_texts(pred, draft_fa, tmp / ("today%d" % t) / "asm", t, fill=None) for t in (1, 3)}
    assert today[1][0] != today[3][0] and today[1][2] != today[3][2]
    assert any(h[4] == "duplicated" for h in tsv_lines(today[3][2], "ctg")[0])
    filled = [fill_texts(pred, draft_fa, tmp / ("filled%d" % t) / "asm", t) for t in (1, 2, 3, 8)]
    assert filled[0] == filled[1] == filled[2] == filled[3]
    assert "filled" in filled[0][2] and "duplicated\t" not in filled[0][2]


def test_golden_inputs(golden_dir, tmp_path):
    """(a), (c), (d) on the reference's golden stitch inputs, every contig of them."""
    pred = tmp_path / "pred"
    qcases.write_golden(golden_dir, pred)
    drafts = {name: draft[:len(draft) // 2] + draft[len(draft) // 2:].lower() + "acgtn" for name, draft in cases.golden_draft(golden_dir).items()}
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    unfilled = cases.fasta_sequences(open(perform_stitch(str(pred), str(tmp_path / "u" / "asm"), 1)).read())
    assert unfilled == cases.fasta_sequences(open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read())
    texts = [fill_texts(pred, draft_fa, tmp_path / ("f%d" % t) / "asm", t) for t in (1, 2)]
    assert texts[0] == texts[1]
    assert list(cases.fasta_sequences(texts[0][0])) == list(unfilled)
    for contig in unfilled:
        sequence = check_filled_contig(pred, draft_fa, drafts[contig], contig, texts[0], unfilled[contig])
        assert sequence.endswith("acgtn")


def test_full_coverage_is_todays_output(tmp_path):
    """(e) every position of the draft has a key: the bytes of the threads=1 files of today, and no `filled` hunk."""
    rng = np.random.default_rng(12)
    draft = cases.random_draft(rng, 300)
    draft = draft[:100] + draft[100:140].lower() + draft[140:]
    pred = tmp_path / "pred"
    pred.mkdir()
    with cases.DataStore(str(pred / "p.hdf"), "w") as s:
        cases.write_region(s, "ctg", 0, 160, cases.rows(draft, 0, 160, {(20, 0): (cases.other(draft[20]), 7), (30, 1): (2, 8), (0, 0): (0, 9)}))
        cases.write_region(s, "ctg", 0, 300, cases.rows(draft, 150, 300, {(299, 0): (cases.other(draft[299]), 3), (200, 0): None, (200, 2): (1, 4)}))
    draft_fa = cases.write_draft(tmp_path / "draft.fa", {"ctg": draft})
    today = fill_texts(pred, draft_fa, tmp_path / "today" / "asm", 1, fill=None)
    for threads in (1, 3):
        filled = fill_texts(pred, draft_fa, tmp_path / ("filled%d" % threads) / "asm", threads)
        assert filled[:2] == today[:2]
        assert filled[2] == today[2].rstrip("\n") + "\tfilled=0\n" and "\tfilled\t" not in filled[2]
    assert fill_texts(pred, draft_fa, tmp_path / "all" / "asm", 1, unpolished_contigs=True) == filled


def test_unpolished_contigs(tmp_path):
    """(g) a contig without a prediction appears only with unpolished_contigs=True, unchanged, in natural order."""
    drafts = planted_with_marks(tmp_path / "pred")
    drafts = {"b1": "acgtNNacgtTTGGaa" * 9, "ctg": drafts["ctg"], "ctg10": "G" * 70, "ctg2": "ttAAccNn"}
    draft_fa = cases.write_draft(tmp_path / "draft.fa", drafts)
    only = fill_texts(tmp_path / "pred", draft_fa, tmp_path / "only" / "asm", 2)
    assert list(cases.fasta_sequences(only[0])) == ["ctg"] and "b1" not in only[2]
    every = fill_texts(tmp_path / "pred", draft_fa, tmp_path / "every" / "asm", 2, unpolished_contigs=True)
    sequences = cases.fasta_sequences(every[0])
    assert list(sequences) == ["b1", "ctg", "ctg2", "ctg10"] == list(fastq_records(every[1]))
    assert sequences["ctg"] == cases.fasta_sequences(only[0])["ctg"]
    unfilled = cases.fasta_sequences(open(perform_stitch(str(tmp_path / "pred"), str(tmp_path / "u" / "asm"), 1)).read())
    for contig in sequences:
        check_filled_contig(tmp_path / "pred", draft_fa, drafts[contig], contig, every, unfilled.get(contig))
    for contig in ("b1", "ctg2", "ctg10"):
        assert sequences[contig] == drafts[contig] and fastq_records(every[1])[contig][1] == "!" * len(drafts[contig])
        assert tsv_lines(every[2], contig)[0] == [("0", str(len(drafts[contig])), "0", str(len(drafts[contig])), "filled", ".", ".", ".")]
    assert [line.split("\t")[0][9:] for line in every[2].splitlines() if line.startswith("##contig=")] == ["b1", "ctg", "ctg2", "ctg10"]
    # without the FASTQ and the edits: the same FASTA
    out = perform_stitch(str(tmp_path / "pred"), str(tmp_path / "plain" / "asm"), 4, fill=draft_fa, unpolished_contigs=True)
    assert open(out).read() == every[0] and os.listdir(os.path.dirname(out)) == ["asm_pepper_polished.fa"]


def test_errors(planted):
    """(h) a contig with predictions that the draft lacks; a kept position the draft does not reach; arguments that do not go
    together."""
    pred, draft_fa, draft, tmp = planted
    short = cases.write_draft(tmp / "short.fa", {"ctg": draft[:350]})
    for kw in (dict(fill=short), dict(fill=short, edits=short, qualities=True)):
        with pytest.raises(ValueError, match="no letter at position 350"):
            perform_stitch(str(pred), str(tmp / "short" / "asm"), 1, **kw)
    fasta, _, _ = fill_texts(pred, cases.write_draft(tmp / "just.fa", {"ctg": draft[:351]}), tmp / "just" / "asm", 1)
    assert cases.fasta_sequences(fasta)["ctg"] == cases.fasta_sequences(fill_texts(pred, draft_fa, tmp / "whole" / "asm", 1)[0])["ctg"][:-49]
    other = cases.write_draft(tmp / "other.fa", {"another": draft})
    for kw in (dict(fill=other), dict(fill=other, unpolished_contigs=True), dict(fill=other, edits=other)):
        with pytest.raises(KeyError):
            perform_stitch(str(pred), str(tmp / "other" / "asm"), 1, **kw)
    with pytest.raises(ValueError, match="needs fill"):
        perform_stitch(str(pred), str(tmp / "bad" / "asm"), 1, unpolished_contigs=True)
    with pytest.raises(ValueError, match="against the draft that fills"):
        perform_stitch(str(pred), str(tmp / "bad" / "asm"), 1, fill=draft_fa, edits=short)


def test_off_is_off(planted):
    """(i) with fill unset the files are those written without the argument."""
    pred, draft_fa, _, tmp = planted
    for threads in (1, 3):
        perform_stitch(str(pred), str(tmp / ("bare%d" % threads) / "asm"), threads, qualities=True, edits=draft_fa)
        bare = tuple(open(str(tmp / ("bare%d" % threads) / "asm") + suffix).read() for suffix in SUFFIXES)
        assert fill_texts(pred, draft_fa, tmp / ("off%d" % threads) / "asm", threads, fill=None, unpolished_contigs=False) == bare
        assert "filled" not in bare[2]
    out = perform_stitch(str(pred), str(tmp / "plain" / "asm"), 3, fill=None)
    assert open(out).read() == bare[0] and os.listdir(os.path.dirname(out)) == ["asm_pepper_polished.fa"]


def test_hunks_written_by_hand():
    """Filled records by hand: a run is a `filled` hunk between its neighbours, the ends come from the piece."""
    draft = "acGTNACgtAC"
    records = np.array([(3, 3, 0, 0, 1, ord("T"), ord("A"), 0), (3, 4, 1, 0, 3, 0, ord("G"), 0), (5, 6, 0, 0, 2, ord("A"), 0, 0),
                        (7, 7, 0, 0, 4, ord("G"), 0, 0), (8, 7, 0, 0, 5, ord("T"), 0, 0)], Edits.EDIT_DTYPE)
    pieces = [(2, 9, 11)]
    assert Edits.apply_filled(draft, records, pieces) == "ac" + "GAG" + "N" + "C" + "gt" + "A" + "C"
    assert Edits.filled_hunks(records, pieces, len(draft), False) == [
        (0, 2, 0, 2, "filled", ".", ".", "."), (3, 4, 3, 5, "complex", "T", "AG", "."), (5, 6, 6, 6, "del", "A", ".", "."),
        (7, 9, 7, 9, "filled", ".", ".", "."), (10, 11, 10, 11, "filled", ".", ".", ".")]
    assert Edits.filled_hunks(np.zeros(0, Edits.EDIT_DTYPE), [], 5, True) == [(0, 5, 0, 5, "filled", ".", ".", ".")]
    assert Edits.summary(Edits.filled_hunks(records, pieces, len(draft), False), filled=True)["filled"] == 5
    with pytest.raises(ValueError, match="one piece"):
        Edits.filled_hunks(records, [(2, 5, 4), (6, 9, 4)], len(draft), False)


def test_signatures_and_switch(monkeypatch):
    from pepper_amd.polish import Stitch
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
    from pepper_amd.polish.polish import polish
    for fn in (polish, perform_stitch, Stitch.small_chunk_stitch, Stitch.small_chunk_stitch_numpy, Stitch.create_consensus_sequence,
               stitch_directory, DeviceStitcher.finish, DeviceStitcher.write_fasta, DeviceStitcher.write_fastq):
        assert inspect.signature(fn).parameters["fill"].default is None, fn
    for fn in (perform_stitch, stitch_directory, DeviceStitcher.write_fasta, DeviceStitcher.write_fastq):
        assert inspect.signature(fn).parameters["unpolished_contigs"].default is False, fn
    assert inspect.signature(Edits.write_contig).parameters["filled"].default is False
    monkeypatch.delenv("PEPPER_AMD_POLISH_FILL", raising=False)
    assert _lib.polish_fill() is False
    monkeypatch.setenv("PEPPER_AMD_POLISH_FILL", "1")
    assert _lib.polish_fill() is True
    monkeypatch.setenv("PEPPER_AMD_POLISH_FILL", "yes")
    assert _lib.polish_fill() is False
    assert _lib.POLISH_FILL_ENV == "PEPPER_AMD_POLISH_FILL"
    assert "pa_stitcher_fill" in {name for name, _, _ in _lib.SYMBOLS}


def test_new_symbol_loads_and_refuses_a_null_handle():
    from pepper_amd import build
    build.build()
    assert _lib.load().pa_stitcher_fill(None, None, 0, None, None) == _lib.PA_ERR_INVALID
