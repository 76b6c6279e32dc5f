"""options.haploid_contigs / options.par_regions_bed through the candidate finder's three host forms (the I/O library, the numpy
columns with PEPPER_AMD_CANDIDATES_PYTHON=1, the reference-shaped tuples with PEPPER_AMD_CANDIDATES_TUPLES=1) and the site merge.

The hand-built job: two contigs of "ACGT" repeated (no homopolymer: REP is 0 everywhere; the reference base of position p is
"ACGT"[p % 4]), chrA diploid and chrH haploid with a PAR on 100 - 200.  Every probability is a binary fraction, so a primed triple
(pepper_amd/variant/Ploidy.py) is exact in float32 and every expectation below was worked out by hand:
QUAL = max(1, int(-10 log10(1 - gq))), gq = the called class's probability, or max(p1, p2) at a hom-ref call."""
import os
import types

import numpy as np
import pytest

import select_utils as su
from haploid_utils import host_select_ploidy
from pepper_amd.variant import FastCandidates, Ploidy, bgzf
from pepper_amd.variant.DataStorePredict import DataStore
from pepper_amd.variant.FindCandidates import process_candidates

VCFS = ("PEPPER_VARIANT_FULL", "PEPPER_VARIANT_OUTPUT_PEPPER", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING",
        "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_SNPs", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_INDEL")
F = "GT:AP:GQ:DP:AD:VAF:REP"
HET = [0.125, 0.5, 0.375]            # diploid: het, gq 0.5 -> QUAL 3, AP 0.5.  primed: (0.25, 0, 0.75) -> "1", QUAL 6, AP 0.75

RECORDS = [
    # ---- chrA, diploid
    ("chrA", 12, 40, "1C", 20, HET),
    ("chrA", 24, 40, "1C", 20, HET),                                     # a two-allele site: 1/2
    ("chrA", 24, 40, "1G", 16, [0.0625, 0.5, 0.4375]),
    ("chrA", 36, 40, "1T", 38, [0.0009765625, 0.5, 0.4990234375]),
    ("chrA", 48, 32, "1C", 8, [0.25, 0.5, 0.25]),
    ("chrA", 52, 40, "3ACG", 10, [0.75, 0.25, 0.0]),                     # a deletion admitted by probability: swapped
    # ---- chrH, haploid outside 100 - 200
    ("chrH", 0, 40, "1C", 20, HET),                                      # position 0
    ("chrH", 10, 40, "1A", 20, HET),                                     # het -> 1
    ("chrH", 20, 32, "1C", 8, [0.25, 0.5, 0.25]),                        # (0.5, 0, 0.5): a tie, the first maximum -> 0, refCall
    ("chrH", 30, 40, "1T", 6, [0.875, 0.125, 0.0]),                      # (1, 0, 0): non_alt 0 < 0.1, dropped (diploid: kept, 0/0)
    ("chrH", 40, 50, "1G", 48, [0.0009765625, 0.5, 0.4990234375]),       # (2^-9, 0, 1 - 2^-9): 1, QUAL 27 -> the PEPPER file
    # a deletion admitted by probability only AFTER priming: non_alt 0.234375 < 0.25 raw (kept by frequency, unswapped),
    # 0.1875 / 0.75 = 0.25 >= 0.25 primed (swapped)
    ("chrH", 50, 40, "3GTA", 10, [0.5625, 0.234375, 0.1875]),
    # ... and one only BEFORE: non_alt 0.25 raw (swapped), (1, 0, 0) primed (kept by frequency, unswapped)
    ("chrH", 60, 40, "3ACG", 10, [0.75, 0.25, 0.0]),
    # a two-allele site where both alleles prime to genotype 2: (0.25, 0, 0.75) and (0.125, 0, 0.875)
    ("chrH", 70, 40, "1A", 16, HET),
    ("chrH", 70, 40, "1C", 20, [0.0625, 0.5, 0.4375]),
    # ... and one where none does: (0.75, 0, 0.25) and (0.875, 0, 0.125)
    ("chrH", 80, 40, "1C", 10, [0.375, 0.5, 0.125]),
    ("chrH", 80, 40, "1G", 12, [0.4375, 0.5, 0.0625]),
    # het rows on both sides of both PAR edges
    ("chrH", 99, 40, "1A", 20, HET),
    ("chrH", 100, 40, "1C", 20, HET),
    ("chrH", 150, 40, "1T", 20, HET),                                    # a two-allele site inside the PAR: 1/2 as ever
    ("chrH", 150, 40, "1A", 16, [0.0625, 0.5, 0.4375]),
    ("chrH", 199, 40, "1A", 20, HET),
    ("chrH", 200, 40, "1C", 20, HET),
]

# the FULL file's chrH lines with the feature on
WANT_CHRH = [
    ["chrH", "1", ".", "A", "C", "6", "PASS", ".", F, "1:0.75:6:40:20:0.5:0"],
    ["chrH", "11", ".", "G", "A", "6", "PASS", ".", F, "1:0.75:6:40:20:0.5:0"],
    ["chrH", "21", ".", "A", "C", "3", "refCall", ".", F, "0:0.5:3:32:8:0.25:0"],
    ["chrH", "41", ".", "A", "G", "27", "PASS", ".", F, "1:0.998047:27:50:48:0.96:0"],
    ["chrH", "51", ".", "GTA", "G", "1", "refCall", ".", F, "0:0.25:1:40:10:0.25:0"],
    ["chrH", "61", ".", "A", "ACG", "1", "refCall", ".", F, "0:0:1:40:10:0.25:0"],
    # sorted by (genotype, probability) descending: C (0.875) then A (0.75); the called allele is the first of genotype 2 -> 1;
    # QUAL from the weaker call (0.75 -> 6)
    ["chrH", "71", ".", "G", "C,A", "6", "PASS", ".", F, "1:0.875,0.75:6:40:20,16:0.5,0.4:0"],
    # both hom-ref: G (0.875) then C (0.75); gq = max(p1', p2') of the first = 0.125 -> QUAL 1
    ["chrH", "81", ".", "A", "G,C", "1", "refCall", ".", F, "0:0.125,0.25:1:40:12,10:0.3,0.25:0"],
    ["chrH", "100", ".", "T", "A", "6", "PASS", ".", F, "1:0.75:6:40:20:0.5:0"],
    ["chrH", "101", ".", "A", "C", "3", "PASS", ".", F, "0/1:0.5:3:40:20:0.5:0"],
    ["chrH", "151", ".", "G", "T,A", "3", "PASS", ".", F, "1/2:0.5,0.5:3:40:20,16:0.5,0.4:0"],
    ["chrH", "200", ".", "T", "A", "3", "PASS", ".", F, "0/1:0.5:3:40:20:0.5:0"],
    ["chrH", "201", ".", "A", "C", "6", "PASS", ".", F, "1:0.75:6:40:20:0.5:0"],
]
# ... and where each lands: QUAL 27 > 20 stays with PEPPER; refCalls and low QUALs go to re-genotyping, split by SNP / indel
WANT_PEPPER = ["41"]
WANT_SNPS = ["1", "11", "21", "71", "81", "100", "101", "151", "200", "201"]
WANT_INDEL = ["51", "61"]


def options(**kw):
    o = types.SimpleNamespace(
        fasta=None, sample_name="SAMPLE", threads=1, allowed_multiallelics=4,
        snp_p_value=0.1, insert_p_value=0.25, delete_p_value=0.25,
        snp_p_value_in_lc=0.1, insert_p_value_in_lc=0.3, delete_p_value_in_lc=0.3,
        snp_q_cutoff=20, indel_q_cutoff=15, snp_q_cutoff_in_lc=20, indel_q_cutoff_in_lc=10,
        report_snp_above_freq=0, report_indel_above_freq=0.2)
    o.__dict__.update(kw)
    return o


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("haploid_candidates")
    fa = str(tmp / "ref.fa")
    with open(fa, "w") as fh:
        for name in ("chrA", "chrH"):
            fh.write(">" + name + "\n" + "\n".join(["ACGT" * 10] * 10) + "\n")
    par = str(tmp / "par.bed")
    with open(par, "w") as fh:
        fh.write("chrH\t100\t200\nchrA\t0\t50\n")
    pred = tmp / "pred"
    pred.mkdir()
    with DataStore(str(pred / "pepper_prediction_0.hdf"), "w") as store:
        b = 0
        for contig in ("chrA", "chrH"):                      # batches of one contig, as the pipeline writes them
            rows = [r for r in RECORDS if r[0] == contig]
            for i in range(0, len(rows), 6):
                part = rows[i:i + 6]
                store.write_prediction(b, [r[0] for r in part], [r[1] for r in part], [r[2] for r in part],
                                       np.array([[r[3]] for r in part], dtype=object), np.array([[r[4]] for r in part], dtype=np.uint8),
                                       np.array([r[5] for r in part], dtype=np.float32))
                b += 1
    return types.SimpleNamespace(tmp=tmp, fasta=fa, par=par, pred=str(pred))


def _run(job, form, tag, monkeypatch, **over):
    for key in ("PEPPER_AMD_CANDIDATES_PYTHON", "PEPPER_AMD_CANDIDATES_TUPLES", Ploidy.ENV_CONTIGS, Ploidy.ENV_PAR):
        monkeypatch.delenv(key, raising=False)
    if form != "native":
        monkeypatch.setenv("PEPPER_AMD_CANDIDATES_" + form.upper(), "1")
    out = str(job.tmp / (tag + "_" + form))
    totals = process_candidates(options(fasta=job.fasta, **over), job.pred, out)
    files = {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() for name in VCFS}
    index = {name: bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz.tbi")) for name in VCFS}
    return files, index, totals


def _data(lines, contig=None):
    rows = [line.split("\t") for line in lines if not line.startswith("#")]
    return [r for r in rows if contig is None or r[0] == contig]


@pytest.fixture()
def runs(job, monkeypatch):
    on = {form: _run(job, form, "on", monkeypatch, haploid_contigs="chrH", par_regions_bed=job.par)
          for form in ("native", "python", "tuples")}
    off = _run(job, "native", "off", monkeypatch)
    return on, off


def test_the_three_host_forms_write_the_same_files(runs):
    on, _ = runs
    files, index, totals = on["native"]
    assert totals[0] == len(_data(files["PEPPER_VARIANT_FULL"])) >= 17
    for form in ("python", "tuples"):
        other_files, other_index, other_totals = on[form]
        assert tuple(other_totals) == tuple(totals), form
        for name in VCFS:
            assert other_files[name] == files[name], (form, name)
            assert other_index[name] == index[name], (form, name)


def test_hand_derived_records_and_routing(runs):
    on, _ = runs
    files = on["native"][0]
    assert _data(files["PEPPER_VARIANT_FULL"], "chrH") == WANT_CHRH
    assert [r[1] for r in _data(files["PEPPER_VARIANT_OUTPUT_PEPPER"], "chrH")] == WANT_PEPPER
    assert [r[1] for r in _data(files["PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_SNPs"], "chrH")] == WANT_SNPS
    assert [r[1] for r in _data(files["PEPPER_VARIANT_OUTPUT_VARIANT_CALLING_INDEL"], "chrH")] == WANT_INDEL
    assert [r[1] for r in _data(files["PEPPER_VARIANT_OUTPUT_VARIANT_CALLING"], "chrH")] == \
        sorted(WANT_SNPS + WANT_INDEL, key=int)
    for name in VCFS:
        assert all(r in _data(files["PEPPER_VARIANT_FULL"]) for r in _data(files[name]))


def test_no_diploid_genotype_outside_the_par_and_nothing_else_changes(runs):
    on, off = runs
    files, off_files = on["native"][0], off[0]
    for name in VCFS:
        outside = [r for r in _data(files[name], "chrH") if not 100 <= int(r[1]) - 1 < 200]
        assert all("/" not in r[9].split(":")[0] for r in outside), name
        unchanged = lambda rows: [r for r in rows if r[0] == "chrA" or 100 <= int(r[1]) - 1 < 200]      # noqa: E731
        assert unchanged(_data(files[name])) == unchanged(_data(off_files[name])), name
    full, off_full = _data(files["PEPPER_VARIANT_FULL"]), _data(off_files["PEPPER_VARIANT_FULL"])
    assert len([r for r in full if r[0] == "chrA"]) == 5 and any(r[9].startswith("1/2:") for r in full if r[0] == "chrA")
    # the feature-off run calls the same rows diploid: het records outside the PAR, the row priming drops, both swaps the other way
    off_h = {r[1]: r for r in off_full if r[0] == "chrH"}
    assert sum(r[9].startswith("0/1:") for r in off_h.values() if not 100 <= int(r[1]) - 1 < 200) >= 5
    assert off_h["31"][9].startswith("0/0:") and "31" not in [r[1] for r in full if r[0] == "chrH"]
    assert (off_h["51"][3], off_h["51"][4]) == ("G", "GTA") and (off_h["61"][3], off_h["61"][4]) == ("ACG", "A")
    assert off_h["71"][9].startswith("1/2:") and off_h["81"][9].startswith("1/2:")


def test_the_header_says_what_was_asked_for(runs, job, monkeypatch):
    on, off = runs
    line = "##pepper_amd_haploid_contigs=chrH;par_regions_bed=par.bed"
    for name in VCFS:
        head = [h for h in on["native"][0][name] if h.startswith("#")]
        off_head = [h for h in off[0][name] if h.startswith("#")]
        assert head[5].startswith("##FILTER=") and head[6] == line and head[7].startswith("##FORMAT=")
        assert head[:6] + head[7:] == off_head and not any("haploid" in h for h in off_head)
    star = _run(job, "native", "star", monkeypatch, haploid_contigs="*")[0]["PEPPER_VARIANT_FULL"]
    assert "##pepper_amd_haploid_contigs=*" in star
    assert all("/" not in r[9].split(":")[0] for r in _data(star))


def test_an_unknown_contig_or_a_par_alone_stops_the_run(job, monkeypatch):
    with pytest.raises(ValueError, match="chrQ"):
        _run(job, "native", "typo", monkeypatch, haploid_contigs="chrH,chrQ")
    with pytest.raises(ValueError, match="needs haploid_contigs"):
        _run(job, "native", "par_alone", monkeypatch, par_regions_bed=job.par)


def test_the_environment_switches_it_on(job, runs, monkeypatch):
    on, _ = runs
    for key in ("PEPPER_AMD_CANDIDATES_PYTHON", "PEPPER_AMD_CANDIDATES_TUPLES"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv(Ploidy.ENV_CONTIGS, "chrH")
    monkeypatch.setenv(Ploidy.ENV_PAR, job.par)
    out = str(job.tmp / "env")
    process_candidates(options(fasta=job.fasta), job.pred, out)
    for name in VCFS:
        assert bgzf.read_bgzf(os.path.join(out, name + ".vcf.gz")).decode().splitlines() == on["native"][0][name]


def _format_ploidy(case, rule, haploid):
    """pa_candidates_select_format_ploidy over a select_utils.Case -> (rows, flags, ref_len, lines) or None for -2."""
    got = host_select_ploidy(case, rule, haploid)
    return None if got is None else (got["row"], got["full_flags"], got["ref_len"], got["lines"])


def test_a_null_mask_gives_the_old_functions_bytes():
    """With the options absent native_batch_arrays hands the new entry point NULL: byte for byte pa_candidates_select_format, and
    so is a mask of zeros; a mask of ones is not."""
    case, rule = su.random_case(1500, 11), su.rules()
    want = su.host_select(case, rule)
    assert len(want["row"]) > 300
    for mask in (None, np.zeros(case.n, np.uint8)):
        row, flags, ref_len, lines = _format_ploidy(case, rule, mask)
        assert np.array_equal(row, want["row"]) and np.array_equal(flags, want["full_flags"]) and not (flags & 8).any()
        assert np.array_equal(ref_len, want["ref_len"]) and lines == want["lines"]
    row, flags, _, lines = _format_ploidy(case, rule, np.ones(case.n, np.uint8))
    assert (flags & 8).all() and not ((flags >> 4) == 1).any() and lines != want["lines"]
    assert all(b"/" not in line.split(b"\t")[9].split(b":")[0] for line in lines)


def test_a_nan_is_still_handed_to_the_python_path():
    case, rule = su.random_case(64, 3), su.rules()
    kept = su.host_select(case, rule)["row"]
    case.prediction[int(kept[0]), 1] = np.nan
    assert _format_ploidy(case, rule, np.ones(case.n, np.uint8)) is None
    case.prediction[int(kept[0])] = [np.nan, 0.5, 0.25]
    assert _format_ploidy(case, rule, np.ones(case.n, np.uint8)) is None


def test_random_batches_the_library_against_the_python_loops(tmp_path):
    """One contig with a PAR through it, 3 000 random rows (sites with several allele records among them), Dirichlet and tied
    probabilities: pa_candidates_select_format_ploidy against _select_batch + _format_single, and the records of the merge."""
    from pepper_amd.variant.CandidateFinder import _fasta
    rng = np.random.default_rng(21)
    ref = "".join("ACGT"[int(k)] * int(r) for k, r in zip(rng.integers(0, 4, 6000), rng.choice([1, 1, 2, 6], 6000)))
    fa = str(tmp_path / "r.fa")
    with open(fa, "w") as fh:
        fh.write(">c1\n" + ref + "\n")
    par = str(tmp_path / "par.bed")
    with open(par, "w") as fh:
        fh.write("c1\t2000\t3000\nc1\t7000\t7001\n")
    n = 3000
    pos = np.sort(rng.choice(np.arange(20, len(ref) - 20), n, replace=True)).astype(np.int32)
    depth = rng.choice([1, 2, 8, 16, 32, 64, 90], n).astype(np.uint8)
    support = rng.integers(0, 60, (n, 1)).astype(np.uint8)
    cands = [[("1" + "ACGT"[int(rng.integers(4))], "2" + ref[int(p)] + "ACG"[: int(rng.integers(1, 4))], "3" + ref[int(p):int(p) + int(rng.integers(2, 6))])
              [int(rng.integers(3))]] for p in pos]
    probs = rng.dirichlet([0.5, 0.5, 0.5], n).astype(np.float32)
    probs[rng.random(n) < 0.1] = [0.25, 0.5, 0.25]
    probs[rng.random(n) < 0.05] = [0.0, 1.0, 0.0]
    probs[rng.random(n) < 0.05] = [0.0, 0.0, 1.0]
    pred = str(tmp_path / "p.hdf")
    with DataStore(pred, "w") as store:
        store.write_prediction(0, ["c1"] * n, pos, depth, np.array(cands, dtype=object), support, probs)
    opts = options(fasta=fa, haploid_contigs="c1", par_regions_bed=par, report_snp_above_freq=0.15, report_indel_above_freq=0.15)
    handler = _fasta(opts)
    seg = FastCandidates._native_batch(opts, FastCandidates._rules(opts), handler, pred, "batch_0")
    left = []
    want = FastCandidates._python_batch(opts, handler, pred, "batch_0", left)
    assert seg is not None and seg.raw is not None and not left and len(seg) == len(want) > 1000
    assert seg.lines == want.lines and np.array_equal(seg.pos, want.pos) and np.array_equal(seg.ref_len, want.ref_len)
    assert np.array_equal(seg.snp, want.snp) and np.array_equal(seg.sel, want.sel)
    haploid = Ploidy.of(opts).is_haploid("c1", seg.pos)
    assert haploid.sum() > 500 and (~haploid).sum() > 100
    assert np.array_equal((seg.raw[1] & 8) != 0, haploid)
    for k in range(0, len(seg), 7):
        assert seg.record(k) == want.record(k) and seg.pair(k) == want.pair(k)
        assert len(seg.record(k)[5]) == (1 if haploid[k] else 2)
