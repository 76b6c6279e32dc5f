"""polish(..., vcf=True): the rule of pepper_amd/polish/Variants.py on the host -- the numpy twin against a per-hunk restatement
on strings over random small contigs and the properties a VCF reader relies on, exact lines and the written file for a contig
written by hand, and perform_stitch(..., fill=, vcf=) on planted predictions.  No GPU."""
import contextlib
import inspect

import numpy as np
import pytest

import polish_edits_cases as cases
import polish_vcf_cases as vcases
import test_polish_fill_cpu as fcases
from pepper_amd import _lib
from pepper_amd.polish import Edits, Variants
from pepper_amd.polish.perform_stitch import perform_stitch
from pepper_amd.variant.bgzf import parse_tbi, read_bgzf


def twin_calls(records, draft, consensus):
    return [(pos, ref, alt, int(q), int(k)) for (pos, ref, alt), q, k in
            zip(Variants.alleles(records, draft, consensus), records["phred"], records["shift"])]


def check_case(draft, keys, phred):
    edit_records, pieces, consensus = vcases.filled(draft, keys, phred)
    want, want_counts = vcases.restated(edit_records, pieces, draft, consensus)
    records, counts = Variants.records_numpy(edit_records, draft, consensus, True)
    assert twin_calls(records, draft, consensus) == [w[:5] for w in want], (draft, consensus)
    assert counts == want_counts
    D, at = draft.upper(), 0
    for (pos, ref, alt, _q, k, bound), r in zip(want, records):
        assert ref and alt and ref != alt
        assert pos - 1 >= at                                         # POS ascending, REF spans disjoint
        at = pos - 1 + len(ref)
        assert at <= len(D) and D[pos - 1:at] == ref
        if r["kind"] in (Variants.KIND_INS, Variants.KIND_DEL) and not r["tail"]:      # it cannot move one further
            assert pos - 1 == bound or D[pos - 1] != (D[at - 1] if r["kind"] == Variants.KIND_DEL else alt[-1])
            assert ref[0] == alt[0] and (len(ref) == 1 or len(alt) == 1)
    calls = [w[:3] for w in want]
    assert counts[2] <= 1
    if counts[2] == 0:
        assert Variants.replay(draft, calls) == consensus.upper()
    else:                                   # the one hunk without an anchor is the contig's last: replay leaves it as the draft has it
        d0, d1, o0, o1 = [h for h in Edits.filled_hunks(edit_records, pieces, len(draft), True) if h[4] != "filled"][-1][:4]
        assert d1 == len(draft) and Variants.replay(draft, calls) == (consensus[:o0] + draft[d0:d1] + consensus[o1:]).upper()
    # the text in columns is the text record by record
    _, _, text = Variants.lines("c", records, draft, consensus, True)
    assert [t.decode() for t in text] == ["c\t%d\t.\t%s\t%s\t%d\tPASS\t.\tGT:GQ\t1:%d\n" % (p, r, a, q, q) for p, r, a, q, _ in
                                          twin_calls(records, draft, consensus)]
    return counts


def test_twin_against_the_restatement_on_random_contigs():
    rng = np.random.default_rng(20260)
    total = np.zeros(5, np.int64)
    longest = 0
    for _ in range(20000):
        draft, keys, phred = vcases.random_case(rng)
        counts = check_case(draft, keys, phred)
        total += counts
        longest = max(longest, counts[4])
    assert total[0] > 20000 and total[1] > 0 and total[2] > 0 and total[3] > 1000 and longest >= 10      # every branch was taken


HAND = "ACAAAAGTTCACACACGgnAAT"
#       0123456789012345678901


def hand_records():
    """A SNV at 1, a deletion at the right end of AAAA (5 -> anchored on C at 2), an inserted T behind TT (9), a deleted AC at the
    right end of the ACACAC run (14..15 -> anchored on C at 9), a complex hunk at 17 (g -> TT: no letter in common), an insertion
    behind the last letter."""
    changes = {(1, 0): 3, (5, 0): 0, (8, 1): 4, (14, 0): 0, (15, 0): 0, (17, 0): 4, (17, 1): 4, (21, 1): 2}
    keys = vcases.keys_of(HAND, changes, holes=(18,))
    return vcases.filled(HAND, keys, np.arange(10, 10 + keys[0].size))


def test_exact_lines_header_and_file(tmp_path):
    edit_records, pieces, consensus = hand_records()
    assert consensus == "AGAAAGTTTCACACGTTnAATC"
    records, counts = Variants.records_numpy(edit_records, HAND, consensus, True)
    assert counts == [6, 0, 0, 3, 2 + 2 + 4]
    _, _, text = Variants.lines("ctg", records, HAND, consensus, True)
    # (the deletion in AAAA stops at 3: anchored at 2 it would lie inside the SNV in front of it, its bound)
    want = ["ctg\t2\t.\tC\tG\t11\tPASS\t.\tGT:GQ\t1:11\n",
            "ctg\t3\t.\tAA\tA\t15\tPASS\t.\tGT:GQ\t1:15\n",
            "ctg\t7\t.\tG\tGT\t19\tPASS\t.\tGT:GQ\t1:19\n",
            "ctg\t10\t.\tCAC\tC\t25\tPASS\t.\tGT:GQ\t1:25\n",
            "ctg\t18\t.\tG\tTT\t28\tPASS\t.\tGT:GQ\t1:28\n",
            "ctg\t22\t.\tT\tTC\t33\tPASS\t.\tGT:GQ\t1:33\n"]
    assert [t.decode() for t in text] == want
    assert Variants.replay(HAND, Variants.parse("".join(want))["ctg"]) == consensus.upper()
    _, _, plain = Variants.lines("ctg", records, HAND, consensus, False)
    assert plain[0].decode() == "ctg\t2\t.\tC\tG\t.\tPASS\t.\tGT\t1\n"
    head = Variants.header([("ctg", len(HAND)), ("other", 7)])
    assert head == ("##fileformat=VCFv4.2\n##source=pepper_amd polish\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
                    "##contig=<ID=ctg,length=22>\n##contig=<ID=other,length=7>\n"
                    "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
                    "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n"
                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
    with contextlib.ExitStack() as files:
        out = Variants.VcfOutput(files, str(tmp_path / "x"), {"ctg": len(HAND), "other": 7})
        out.contig("ctg", records, counts, HAND, consensus, True)
    assert out.path == str(tmp_path / "x_pepper_polished.vcf.gz")
    assert read_bgzf(out.path).decode() == head + "".join(want)
    index = parse_tbi(out.path + ".tbi")
    assert index["names"] == ["ctg"] and index["format"] == 2 and len(index["refs"]) == 1


def test_a_long_allele_is_written_like_a_short_one():
    draft = "G" + "AC" * 40 + "T"
    keys = vcases.keys_of(draft, {(p, 0): 0 for p in range(21, 81)})
    edit_records, pieces, consensus = vcases.filled(draft, keys)
    records, counts = Variants.records_numpy(edit_records, draft, consensus, True)
    assert counts == [1, 0, 0, 1, 20] and int(records["ref_len"][0]) == 61
    _, _, text = Variants.lines("c", records, draft, consensus, True)
    assert text[0].decode() == "c\t1\t.\tG" + "AC" * 30 + "\tG\t40\tPASS\t.\tGT:GQ\t1:40\n"
    assert Variants.replay(draft, Variants.parse(text[0])["c"]) == consensus


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vcf_planted")
    drafts = fcases.planted_with_marks(tmp / "pred")
    drafts["zz_untouched"] = "ACGTTGCA"
    return tmp / "pred", cases.write_draft(tmp / "draft.fa", drafts), drafts, tmp


def vcf_text(prefix):
    return read_bgzf(str(prefix) + "_pepper_polished.vcf.gz").decode()


@pytest.mark.parametrize("extra", [dict(), dict(qualities=True, edits=True), dict(min_quality=20), dict(min_quality=50, edits=True)])
def test_perform_stitch_vcf_replays_to_the_fasta(planted, extra):
    pred, draft_fa, drafts, tmp = planted
    kw = dict(extra)
    if kw.pop("edits", False):
        kw["edits"] = draft_fa
    if "min_quality" in kw:
        kw["draft"] = draft_fa
    where = tmp / ("out_" + "_".join(sorted(extra)) + str(extra.get("min_quality", "")))
    perform_stitch(str(pred), str(where), 2, fill=draft_fa, unpolished_contigs=True, vcf=draft_fa, **kw)
    text = vcf_text(where)
    assert text.startswith(Variants.header([(name, len(seq)) for name, seq in drafts.items()]))
    calls = Variants.parse(text)
    # (whatever the gate: the planted hunks at 30, 40, 130, 132, 140 and 150 carry phred 50 and more)
    assert list(calls) == ["ctg"] and len(calls["ctg"]) >= 6
    fasta = cases.fasta_sequences(open(str(where) + "_pepper_polished.fa").read())
    for name, draft in drafts.items():
        assert Variants.replay(draft, calls.get(name, [])) == fasta[name].upper()
    assert parse_tbi(str(where) + "_pepper_polished.vcf.gz.tbi") is not None
    if "min_quality" in extra:                                       # the gate takes records away, and the plain run has them all
        plain = Variants.parse(vcf_text(tmp / "out_"))["ctg"] if (tmp / "out__pepper_polished.vcf.gz").exists() else None
        assert plain is None or len(calls["ctg"]) < len(plain)


def test_no_prediction_gives_the_header_alone(planted, tmp_path):
    """What polish() falls back to when no chunk was predicted: the draft as it is, and a VCF without a record."""
    _, draft_fa, drafts, _ = planted
    (tmp_path / "empty").mkdir()
    perform_stitch(str(tmp_path / "empty"), str(tmp_path / "o"), 1, fill=draft_fa, unpolished_contigs=True, vcf=draft_fa)
    assert vcf_text(tmp_path / "o") == Variants.header([(name, len(seq)) for name, seq in drafts.items()])
    assert parse_tbi(str(tmp_path / "o") + "_pepper_polished.vcf.gz.tbi")["names"] == []
    assert cases.fasta_sequences(open(str(tmp_path / "o") + "_pepper_polished.fa").read()) == drafts


def test_vcf_without_fill_raises_and_defaults(planted, tmp_path, monkeypatch):
    pred, draft_fa, _, _ = planted
    with pytest.raises(ValueError, match="vcf needs fill"):
        perform_stitch(str(pred), str(tmp_path / "o"), 1, vcf=draft_fa)
    with pytest.raises(ValueError, match="the one that fills"):
        perform_stitch(str(pred), str(tmp_path / "o"), 1, fill=draft_fa, vcf=str(tmp_path / "other.fa"))
    assert not list(tmp_path.iterdir())
    assert inspect.signature(perform_stitch).parameters["vcf"].default is None
    from pepper_amd.polish.DeviceStitch import DeviceStitcher, stitch_directory
    from pepper_amd.polish.polish import polish
    for function in (stitch_directory, DeviceStitcher.write_fasta, DeviceStitcher.write_fastq, polish):
        assert inspect.signature(function).parameters["vcf"].default is None
    monkeypatch.delenv(_lib.POLISH_VCF_ENV, raising=False)
    assert _lib.polish_vcf() is False
    for value, want in (("1", True), ("0", False), ("true", False), ("", False)):
        monkeypatch.setenv(_lib.POLISH_VCF_ENV, value)
        assert _lib.polish_vcf() is want
