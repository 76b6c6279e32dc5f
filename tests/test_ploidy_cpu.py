"""pepper_amd/variant/Ploidy.py: options.haploid_contigs / options.par_regions_bed read into a Ploidy, `is_haploid` at the edges
of a PAR interval, and the priming of a haploid row's triple on values whose result is exact in float32 and derived by hand."""
import pickle
import types

import numpy as np
import pytest

from pepper_amd.variant import Ploidy

LENGTHS = {"chr1": 1000, "chrX": 5000, "chrY": 800, "chrM": 160}


def _bed(tmp_path, text, name="par.bed"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_a_list_a_star_and_an_unknown_name(tmp_path):
    p = Ploidy.parse("chrX,chrY", None, LENGTHS)
    assert p.contigs == {"chrX", "chrY"} and p.given == "chrX,chrY" and p.par == {} and p.par_name is None
    assert p.header_line() == "##pepper_amd_haploid_contigs=chrX,chrY"
    assert Ploidy.parse(" chrX , chrM ", None, LENGTHS).contigs == {"chrX", "chrM"}
    star = Ploidy.parse("*", None, LENGTHS)
    assert star.contigs == set(LENGTHS) and star.header_line() == "##pepper_amd_haploid_contigs=*"
    with pytest.raises(ValueError, match="chrZ"):
        Ploidy.parse("chrX,chrZ", None, LENGTHS)
    assert Ploidy.parse(None, None, LENGTHS) is None and Ploidy.parse("", None, LENGTHS) is None


def test_par_without_haploid_contigs_is_an_error(tmp_path):
    bed = _bed(tmp_path, "chrX\t10\t20\n")
    with pytest.raises(ValueError, match="needs haploid_contigs"):
        Ploidy.parse(None, bed, LENGTHS)
    with pytest.raises(ValueError, match="needs haploid_contigs"):
        Ploidy.of(types.SimpleNamespace(par_regions_bed=bed))


def test_par_intervals_merge_clamp_and_ignore(tmp_path):
    # touching (100-200, 200-260) and overlapping (250-300) intervals merge; the end beyond the contig is clamped; the interval on
    # the diploid chr1 and the one on a contig the FASTA does not have are ignored with one line that counts them
    bed = _bed(tmp_path, "# PAR\nchrX\t200\t260\nchrX\t100\t200\nchrX 250 300 name\nchrX\t4900\t9000\nchr1\t0\t50\nchrUn\t5\t9\n"
                         "chrX\t700\t700\n")
    said = []
    p = Ploidy.parse("chrX,chrY", bed, LENGTHS, log=said.append)
    assert set(p.par) == {"chrX"}
    assert p.par["chrX"][0].tolist() == [100, 4900] and p.par["chrX"][1].tolist() == [300, 5000]
    assert p.par["chrX"][0].dtype == np.int64
    assert len(said) == 1 and " 2 INTERVALS" in said[0]
    assert p.header_line() == "##pepper_amd_haploid_contigs=chrX,chrY;par_regions_bed=par.bed"
    assert p.boundaries("chrX") == [100, 300, 4900, 5000] and p.boundaries("chrY") == [] and p.boundaries("chr1") == []
    # Targets.read_bed's messages for a malformed line
    with pytest.raises(ValueError, match=r"line 2: end before start"):
        Ploidy.parse("chrX", _bed(tmp_path, "chrX\t1\t2\nchrX\t9\t3\n", "bad.bed"), LENGTHS)
    with pytest.raises(ValueError, match=r"line 1: a BED line needs contig, start and end"):
        Ploidy.parse("chrX", _bed(tmp_path, "chrX\t1\n", "short.bed"), LENGTHS)
    # a file that leaves no interval is not an error here
    empty = Ploidy.parse("chrY", _bed(tmp_path, "chrX\t1\t2\n", "other.bed"), LENGTHS)
    assert empty.par == {} and empty.is_haploid("chrY", [0, 799]).all()


def test_is_haploid_at_the_edges(tmp_path):
    p = Ploidy.parse("chrX", _bed(tmp_path, "chrX\t100\t300\nchrX\t4900\t5000\n"), LENGTHS)
    positions = [0, 99, 100, 299, 300, 4899, 4900, 4999]
    assert p.is_haploid("chrX", positions).tolist() == [True, True, False, False, True, True, False, False]
    assert p.is_haploid("chrX", np.array(positions)).dtype == bool
    assert not p.is_haploid("chr1", positions).any() and not p.is_haploid("nowhere", [0]).any()
    assert p.is_haploid("chrX", []).shape == (0,)
    whole = Ploidy.parse("chrX", None, LENGTHS)
    assert whole.is_haploid("chrX", positions).all()
    haploid, starts, ends = p.table("chrX")
    assert haploid and starts.tolist() == [100, 4900] and ends.tolist() == [300, 5000]
    assert p.table("chr1")[0] is False and len(p.table("chr1")[1]) == 0


def test_the_object_pickles(tmp_path):
    p = Ploidy.parse("chrX", _bed(tmp_path, "chrX\t100\t300\n"), LENGTHS)
    q = pickle.loads(pickle.dumps(p))
    assert q.contigs == p.contigs and q.given == p.given and q.par_name == p.par_name
    assert q.is_haploid("chrX", [99, 100]).tolist() == [True, False]


def test_options_and_environment(tmp_path, monkeypatch):
    class Fasta(object):
        def get_chromosome_names(self):
            return list(LENGTHS)

        def get_chromosome_sequence_length(self, name):
            return LENGTHS[name]
    monkeypatch.delenv(Ploidy.ENV_CONTIGS, raising=False)
    monkeypatch.delenv(Ploidy.ENV_PAR, raising=False)
    assert Ploidy.of(types.SimpleNamespace()) is None                       # absent attributes, unset variables: nothing
    o = types.SimpleNamespace(haploid_contigs="chrM", fasta="x.fa")
    p = Ploidy.of(o, Fasta())
    assert p.contigs == {"chrM"} and Ploidy.of(o) is p                      # (read once per options object)
    assert Ploidy.of(types.SimpleNamespace(ploidy=p)) is p                  # what _plain_options hands a worker
    monkeypatch.setenv(Ploidy.ENV_CONTIGS, "chrY")
    monkeypatch.setenv(Ploidy.ENV_PAR, _bed(tmp_path, "chrY\t10\t20\n"))
    q = Ploidy.of(types.SimpleNamespace(fasta="x.fa"), Fasta())
    assert q.contigs == {"chrY"} and q.par["chrY"][0].tolist() == [10]
    with pytest.raises(ValueError, match="chrQ"):
        Ploidy.of(types.SimpleNamespace(haploid_contigs="chrQ", fasta="x.fa"), Fasta())


def _genotype(t):
    return int(np.argmax(t))


def test_priming_on_hand_derived_triples():
    # (0.25, 0.5, 0.25): s = 0.5, 0.25 / 0.5 = 0.5 on both sides -- a tie, the first maximum is 0
    t = Ploidy.prime(np.array([[0.25, 0.5, 0.25]], np.float32))
    assert t.dtype == np.float32 and t.tolist() == [[0.5, 0.0, 0.5]] and _genotype(t[0]) == 0
    # (0.125, 0.5, 0.375): s = 0.5, 0.125 / 0.5 = 0.25, 0.375 / 0.5 = 0.75 -- genotype 2
    t = Ploidy.prime(np.array([[0.125, 0.5, 0.375]], np.float32))
    assert t.tolist() == [[0.25, 0.0, 0.75]] and _genotype(t[0]) == 2
    # non_alt = max(p1', p2') = 0.75 widened to double: admitted at a threshold of exactly 0.75, not at the next double above
    non_alt = float(max(t[0, 1], t[0, 2]))
    assert non_alt >= 0.75 and not non_alt >= float(np.nextafter(0.75, 1.0))
    # (0, 1, 0): s == 0
    t = Ploidy.prime(np.array([[0.0, 1.0, 0.0]], np.float32))
    assert t.tolist() == [[0.5, 0.0, 0.5]] and _genotype(t[0]) == 0
    # (0.6, 0.3, 0.1): against the formula in float64
    raw = np.array([0.6, 0.3, 0.1], np.float32)
    s = float(raw[0]) + float(raw[2])
    t = Ploidy.prime(raw.reshape(1, 3))
    assert t[0, 0] == np.float32(float(raw[0]) / s) and t[0, 1] == 0 and t[0, 2] == np.float32(float(raw[2]) / s)
    assert _genotype(t[0]) == 0
    # several rows at once are the rows one by one
    rows = np.array([[0.25, 0.5, 0.25], [0.125, 0.5, 0.375], [0, 1, 0], [0.6, 0.3, 0.1]], np.float32)
    assert np.array_equal(Ploidy.prime(rows), np.concatenate([Ploidy.prime(r.reshape(1, 3)) for r in rows]))


def test_prime_batch_touches_only_the_haploid_rows(tmp_path):
    p = Ploidy.parse("chrX", _bed(tmp_path, "chrX\t100\t300\n"), LENGTHS)
    raw = np.array([[0.125, 0.5, 0.375]] * 4, np.float32)
    primed, mask = Ploidy.prime_batch(p, "chrX", [99, 100, 299, 300], raw)
    assert mask.tolist() == [True, False, False, True]
    assert primed.tolist() == [[0.25, 0.0, 0.75], [0.125, 0.5, 0.375], [0.125, 0.5, 0.375], [0.25, 0.0, 0.75]]
    assert raw.tolist() == [[0.125, 0.5, 0.375]] * 4                         # the caller's array is left alone
    primed, mask = Ploidy.prime_batch(p, ["chr1", "chrX", "chrX", "chr1"], [5, 5, 150, 150], raw)
    assert mask.tolist() == [False, True, False, False] and primed[1].tolist() == [0.25, 0.0, 0.75]
    same, mask = Ploidy.prime_batch(None, "chrX", [1, 2, 3, 4], raw)
    assert same is raw and not mask.any()
    assert not Ploidy.prime_batch(p, "chr1", [1, 2, 3, 4], raw)[1].any()
