"""options.region_bed on the host (pepper_amd/variant/Targets.py): the BED reader, the rule `start <= p < end` in numpy, and the
planner's step behind split_intervals -- an interval (contig, s, e) is kept iff a target position lies in [s, e]."""
import numpy as np
import pytest

from pepper_amd.variant import Targets
from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils

LENGTHS = {"ctg": 12000, "other": 500}


def _bed(tmp_path, text, name="targets.bed"):
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def _table(bed, contig="ctg"):
    starts, ends = bed[contig]
    assert starts.dtype == np.int64 and ends.dtype == np.int64
    return list(zip(starts.tolist(), ends.tolist()))


def test_unsorted_overlapping_touching_and_duplicate_lines_merge(tmp_path):
    bed = Targets.read_bed(_bed(tmp_path, "ctg\t900\t1000\nctg\t100\t200\nctg\t150\t300\nctg\t300\t310\nctg\t100\t200\n"
                                          "ctg\t5000\t5001\nother\t10\t20\nctg\t120\t130\nctg\t311\t320\n"), LENGTHS)
    assert _table(bed) == [(100, 310), (311, 320), (900, 1000), (5000, 5001)]       # 310 / 311: a gap of one base stays
    assert _table(bed, "other") == [(10, 20)]


def test_header_and_blank_lines_mixed_whitespace_and_extra_fields(tmp_path):
    text = ("# a comment\ntrack name=panel description=\"ctg 1 2\"\nbrowser position ctg:1-100\n\n   \n"
            "ctg \t 10   20\tname\t0\t+\n  ctg\t30 \t 40  \n#ctg\t50\t60\n")
    assert _table(Targets.read_bed(_bed(tmp_path, text), LENGTHS)) == [(10, 20), (30, 40)]


def test_ends_clamped_unknown_contigs_and_empty_intervals_ignored(tmp_path):
    lines = []
    text = "ctg\t11990\t13000\nnowhere\t0\t100\nelsewhere\t5\t6\nctg\t700\t700\nctg\t12000\t12500\nother\t0\t0\n"
    bed = Targets.read_bed(_bed(tmp_path, text), LENGTHS, log=lines.append)
    assert sorted(bed) == ["ctg"] and _table(bed) == [(11990, 12000)]               # (12000 .. clamps to nothing; `other` keeps none)
    assert len(lines) == 1 and " 2 " in lines[0]


@pytest.mark.parametrize("bad", ["ctg\t10", "ctg", "ctg\tten\t20", "ctg\t10\t2e3", "ctg\t10\t0x20", "ctg\t1_0\t20", "ctg\t-5\t20",
                                 "ctg\t30\t20", "ctg\t10.0\t20", "nowhere\t5\tx"])
def test_malformed_lines_raise_with_their_line_number(tmp_path, bad):
    path = _bed(tmp_path, "# header\nctg\t1\t2\n\n" + bad + "\nctg\t5\t6\n")
    with pytest.raises(ValueError) as err:
        Targets.read_bed(path, LENGTHS)
    assert path in str(err.value) and "line 4" in str(err.value)


def test_a_bed_that_leaves_nothing_raises(tmp_path):
    for text in ("", "# nothing\n", "nowhere\t0\t10\n", "ctg\t5\t5\nctg\t12000\t12010\n"):
        path = _bed(tmp_path, text)
        with pytest.raises(ValueError, match="no target"):
            Targets.read_bed(path, LENGTHS)


def test_contains_at_the_edges_and_on_an_empty_table():
    starts, ends = np.array([100, 311, 5000], np.int64), np.array([310, 320, 5001], np.int64)
    probe = [99, 100, 309, 310, 311, 319, 320, 4999, 5000, 5001, 0, 10**12]
    assert Targets.contains(starts, ends, probe).tolist() == [False, True, True, False, True, True, False, False, True, False,
                                                               False, False]
    none = np.zeros(0, np.int64)
    assert Targets.contains(none, none, probe).tolist() == [False] * len(probe)
    assert Targets.contains(starts, ends, np.zeros(0, np.int64)).shape == (0,)
    # the rule itself, position by position, over a random table
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(3000, 80, replace=False)).astype(np.int64)
    s, e = cuts[0::2], cuts[1::2]                       # disjoint, ascending; touching pairs do not occur (distinct cuts, s < e < next s)
    inside = np.zeros(3100, bool)
    for a, b in zip(s, e):
        inside[a:b] = True
    assert np.array_equal(Targets.contains(s, e, np.arange(3100)), inside)


def test_overlaps_is_closed_at_both_ends():
    starts, ends = np.array([100, 4000], np.int64), np.array([110, 4001], np.int64)
    assert [Targets.overlaps(starts, ends, s, e) for s, e in ((0, 99), (0, 100), (109, 200), (110, 200), (2000, 4000), (4000, 6000),
                                                               (4001, 6000), (0, 10**9))] == [False, True, True, False, True, True, False, True]


class _Fasta(object):
    def __init__(self, lengths):
        self.lengths = lengths

    def get_chromosome_sequence_length(self, name):
        return self.lengths[name]


def _plan(tmp_path, text, region=None, lengths=LENGTHS, region_size=2000):
    chr_list = ImageGenerationUtils.get_chromosome_list(region, None, None) if region else [(c, None) for c in lengths]
    intervals, _ = ImageGenerationUtils.split_intervals(chr_list, _Fasta(lengths), region_size)
    return intervals, Targets.filter_intervals(intervals, Targets.read_bed(_bed(tmp_path, text), lengths))


def test_planner_keeps_exactly_the_intervals_that_hold_a_target(tmp_path):
    intervals, (kept, dropped, dropped_bases) = _plan(tmp_path, "ctg\t2500\t2600\nctg\t7999\t8000\nctg\t11999\t12000\n", lengths={"ctg": 12000})
    assert intervals == [("ctg", 0, 2000), ("ctg", 2000, 4000), ("ctg", 4000, 6000), ("ctg", 6000, 8000), ("ctg", 8000, 10000),
                         ("ctg", 10000, 11999)]
    # 7999 lies in [6000, 8000] alone; 11999 is the last base of the contig and of the last interval
    assert kept == [("ctg", 2000, 4000), ("ctg", 6000, 8000), ("ctg", 10000, 11999)]
    assert dropped == 3 and dropped_bases == 6000
    # the same by the rule, position by position
    bed = Targets.read_bed(_bed(tmp_path, "ctg\t2500\t2600\nctg\t7999\t8000\nctg\t11999\t12000\n"), {"ctg": 12000})
    for contig, s, e in intervals:
        assert ((contig, s, e) in kept) == bool(Targets.contains(*bed[contig], np.arange(s, e + 1)).any())


def test_one_base_on_a_shared_boundary_keeps_both_neighbours(tmp_path):
    _, (kept, dropped, _) = _plan(tmp_path, "ctg\t4000\t4001\n", lengths={"ctg": 12000})
    assert kept == [("ctg", 2000, 4000), ("ctg", 4000, 6000)] and dropped == 4


def test_region_and_bed_intersect(tmp_path):
    text = "ctg\t100\t200\nctg\t3000\t3001\nctg\t5500\t5600\nctg\t9000\t9100\nother\t0\t500\n"
    intervals, (kept, dropped, _) = _plan(tmp_path, text, region="ctg:2500-6500")
    assert intervals == [("ctg", 2500, 4500), ("ctg", 4500, 6500)] and kept == intervals and dropped == 0
    _, (kept, dropped, dropped_bases) = _plan(tmp_path, text, region="ctg:0-6500")
    assert kept == [("ctg", 0, 2000), ("ctg", 2000, 4000), ("ctg", 4000, 6000)] and (dropped, dropped_bases) == (1, 500)
    with pytest.raises(ValueError, match="no target position"):          # targets on the contig, none inside the span
        _plan(tmp_path, text, region="ctg:3001-5499")
    with pytest.raises(ValueError, match="no target position"):          # targets in the file, none on the contig of the run
        _plan(tmp_path, "other\t0\t500\n", region="ctg")
