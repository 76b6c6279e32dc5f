"""pepper_amd/variant/RefConfidence.py and Gvcf.py on the CPU: the table, the bands, the numpy block rule, the track and the
composition of the gVCF on hand-written blocks and records.  Expected values are written out here or worked out in the test
from the rule's statement; none comes from the functions under test."""
import gzip
import math

import numpy as np
import pytest

from pepper_amd.variant import Gvcf, RefConfidence, bgzf
from pepper_amd.variant.RefConfidence import BlockTrack, OFF_TARGET

# (n_ref, n_alt) -> GQ at p = 0.001, max_gq 50, computed in f64
FIXED = {(0, 0): 0, (1, 0): 4, (2, 0): 6, (3, 0): 9, (4, 0): 12, (5, 0): 15, (8, 0): 24, (10, 0): 30, (16, 0): 48, (17, 0): 50,
         (19, 1): 30, (18, 2): 3, (17, 3): 0}


def _gq_by_subtraction(n_ref, n_alt, p, max_gq):
    """The model written the plain way (probabilities, not logs): good where nothing underflows, which holds for small counts."""
    like = [(1 - p) ** n_ref * p ** n_alt, 0.5 ** (n_ref + n_alt), p ** n_ref * (1 - p) ** n_alt]
    return int(math.floor(min(max_gq, -10 * math.log10((like[1] + like[2]) / sum(like)))))


def test_the_table_at_its_fixed_points():
    table = RefConfidence.build_table()
    assert table.shape == (101, 101) and table.dtype == np.uint8
    for (r, a), gq in FIXED.items():
        assert table[r, a] == gq == RefConfidence.gq_value(r, a), (r, a)
    assert table.max() == 50 and table[100, 0] == 50 and table[0, 100] == 0 and table[50, 50] == 0


@pytest.mark.parametrize("p,max_gq", [(0.001, 50), (0.01, 40), (0.1, 99)])
def test_the_table_is_the_model(p, max_gq):
    table = RefConfidence.build_table(p, max_gq)
    for r in range(0, 13):
        for a in range(0, 7):
            if r or a:
                assert table[r, a] == _gq_by_subtraction(r, a, p, max_gq), (r, a)
    steps = table.astype(int)
    assert (np.diff(steps, axis=0) >= 0).all() and (np.diff(steps, axis=1) <= 0).all() and table[0, 0] == 0
    if p != 0.001:
        assert not np.array_equal(table, RefConfidence.build_table())


def test_a_table_needs_a_rate_inside_its_range():
    for p in (0.0, 0.5, -1.0, 1.0):
        with pytest.raises(ValueError):
            RefConfidence.build_table(p)
    with pytest.raises(ValueError):
        RefConfidence.build_table(0.001, 256)


def test_the_rescale_rule():
    # n = 100 is left alone; 101 and 1000 are brought to 100 with n_ref rounded up, in 64-bit products
    assert [v.tolist() for v in RefConfidence.rescale([100, 60, 0], [0, 40, 100])] == [[100, 60, 0], [0, 40, 100]]
    assert [v.tolist() for v in RefConfidence.rescale([101, 100, 1, 0], [0, 1, 100, 101])] == [[100, 100, 1, 0], [0, 0, 99, 100]]
    assert [v.tolist() for v in RefConfidence.rescale([1000, 999, 500, 1], [0, 1, 500, 999])] == [[100, 100, 50, 1], [0, 0, 50, 99]]
    big = 3_000_000_000
    assert [v.tolist() for v in RefConfidence.rescale([big], [big])] == [[50], [50]]
    # 130 identical reads: (100, 0), the cap
    table = RefConfidence.build_table()
    assert RefConfidence.gq_numpy([130], [130], [0], [0], [True], table).tolist() == [50]


def test_the_evidence():
    # cov 20 of which 19 show the reference letter: (19, 1); an insert anchor among three reads: (2, 1); a deleted base
    # beside two reads: (2, 1); a letter column above the coverage never goes negative; a reference N is GQ 0
    n_ref, n_alt = RefConfidence.evidence([20, 3, 2, 2, 3], [19, 3, 2, 3, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0])
    assert n_ref.tolist() == [19, 2, 2, 3, 0] and n_alt.tolist() == [1, 1, 1, 0, 3]
    table = RefConfidence.build_table()
    assert RefConfidence.gq_numpy([20, 3, 3], [19, 3, 3], [0, 0, 0], [0, 0, 0], [True, True, False], table).tolist() == [30, 9, 0]


def test_parse_bands():
    assert RefConfidence.parse_bands(None).tolist() == [0, 1, 10, 20, 30, 40, 50] == RefConfidence.parse_bands("").tolist()
    assert RefConfidence.parse_bands("0, 5,25").tolist() == [0, 5, 25] and RefConfidence.parse_bands([0, 7.0]).tolist() == [0, 7]
    assert RefConfidence.parse_bands(None).dtype == np.int32
    refused = {"entry 8": list(range(9)), "entry 0": [1, 2], "entry 2": [0, 3, 3], "entry 1": [0, -4], "entry 3": "0,1,2,x",
               "no band": []}
    for entry, bands in refused.items():
        with pytest.raises(ValueError, match=entry):
            RefConfidence.parse_bands(bands)
    with pytest.raises(ValueError, match="entry 2"):
        RefConfidence.parse_bands([0, 5, 2])
    with pytest.raises(ValueError, match="entry 1"):
        RefConfidence.parse_bands([0, 256])
    with pytest.raises(ValueError, match="entry 1"):
        RefConfidence.parse_bands([0, 2.5])


def test_the_block_rule_with_its_minima():
    gq = [0, 0, 9, 9, 4, 50, 50, 30, 50, 0]
    cov = [0, 0, 3, 5, 1, 20, 17, 20, 22, 9]
    s, e, band, dp, q = RefConfidence.blocks_numpy(cov, gq, 1000, [0, 1, 10, 20, 30, 40, 50])
    assert list(zip(s.tolist(), e.tolist(), band.tolist(), dp.tolist(), q.tolist())) == [
        (1000, 1002, 0, 0, 0), (1002, 1005, 1, 1, 4), (1005, 1007, 6, 17, 50), (1007, 1008, 4, 20, 30), (1008, 1009, 6, 22, 50),
        (1009, 1010, 0, 9, 0)]
    on = [True] * 3 + [False] * 2 + [True] * 5
    s, e, band, dp, q = RefConfidence.blocks_numpy(cov, gq, 1000, [0, 1, 10, 20, 30, 40, 50], on)
    assert list(zip(s.tolist(), e.tolist(), band.tolist(), dp.tolist(), q.tolist()))[:3] == [
        (1000, 1002, 0, 0, 0), (1002, 1003, 1, 3, 9), (1003, 1005, OFF_TARGET, 1, 4)]
    assert [len(v) for v in RefConfidence.blocks_numpy([], [], 0, [0])] == [0] * 5
    s, e, band, dp, q = RefConfidence.blocks_numpy([4, 2, 7], [3, 2, 1], 5, [0])
    assert (s.tolist(), e.tolist(), band.tolist(), dp.tolist(), q.tolist()) == ([5], [8], [0], [2], [1])


def test_merge_blocks():
    # what the device reports for a run over a tile border: two touching records of one band; not merged: another region,
    # another band, a gap
    cols = ([0, 0, 0, 1, 1, 1], [10, 522, 600, 600, 700, 801], [522, 600, 700, 700, 800, 900], [6, 6, 4, 4, 4, 4],
            [20, 18, 9, 7, 8, 3], [50, 50, 30, 31, 30, 33])
    merged = RefConfidence.merge_blocks(*cols)
    assert list(zip(*(c.tolist() for c in merged))) == [(0, 10, 600, 6, 18, 50), (0, 600, 700, 4, 9, 30), (1, 600, 800, 4, 7, 30),
                                                         (1, 801, 900, 4, 3, 33)]
    assert [c.dtype for c in merged] == [np.int32, np.int64, np.int64, np.int32, np.int32, np.int32]
    assert [len(c) for c in RefConfidence.merge_blocks([], [], [], [], [], [])] == [0] * 6


def _track(bands=(0, 1, 10, 20, 30, 40, 50)):
    return BlockTrack(["c1", "c2", "c3"], np.array(bands, np.int32), RefConfidence.build_table())


def test_the_track():
    first = ([0, 50, 90], [50, 90, 101], [0, 6, 6], [0, 20, 19], [0, 50, 50])           # interval [0, 100]
    second = ([100, 150], [150, 201], [6, 1], [18, 3], [50, 9])                           # interval [100, 200]: owns 100
    third = ([200, 230, 260], [230, 260, 301], [1, OFF_TARGET, 1], [2, 0, 4], [8, 0, 9])  # interval [200, 300]: owns 200
    want = [("c1", 0, 50, 0, 0, 0), ("c1", 50, 150, 6, 18, 50), ("c1", 150, 230, 1, 2, 8), ("c1", 260, 301, 1, 4, 9),
            ("c2", 5, 9, 0, 0, 0)]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        track = _track()
        pieces = [("c1", (0, 100), first), ("c1", (100, 200), second), ("c1", (200, 300), third),
                  ("c2", (5, 8), ([5], [9], [0], [0], [0]))]
        for k in order:
            track.add(*pieces[k])
        assert track.finish() == want, order
    assert "BASES" in track.log_line() and "GQ 50+ 100 " in track.log_line() and "GQ 0-0 54 " in track.log_line()
    with pytest.raises(ValueError):
        track.add("nowhere", (0, 1), ([0], [2], [0], [0], [0]))
    with pytest.raises(ValueError):
        track.add("c1", (0, 1), ([0], [2], [0, 0], [0], [0]))


def test_the_track_cuts_the_earlier_interval_and_keeps_its_minima():
    track = _track()
    track.add("c1", (0, 100), ([0], [101], [6], [17], [50]))
    track.add("c1", (100, 200), ([100], [201], [4], [30], [31]))
    assert track.finish() == [("c1", 0, 100, 6, 17, 50), ("c1", 100, 201, 4, 30, 31)]
    track = _track()
    track.add_empty("c2", (10, 19))
    track.add_empty("c2", (19, 30), on_target=[False] * 6 + [True] * 6)
    assert track.finish() == [("c2", 10, 19, 0, 0, 0), ("c2", 25, 31, 0, 0, 0)]


# ---- the gVCF --------------------------------------------------------------------------------------------------------------
REFERENCE = {"c1": "ACGTACGTAC" * 40, "c2": "TTGCA" * 20, "c3": "G" * 50}


def _ref_base(contig, pos):
    return REFERENCE[contig][pos]


def _record(contig, pos0, ref, alt="T"):
    line = "%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ\t0/1:30\n" % (contig, pos0 + 1, ref, alt)
    return (contig, pos0, len(ref), line.encode())


BLOCKS = [("c1", 0, 50, 0, 0, 0), ("c1", 50, 150, 6, 18, 50), ("c1", 150, 230, 1, 2, 8), ("c1", 260, 301, 1, 4, 9),
          ("c3", 0, 50, 6, 25, 50)]
def _at(contig, pos0, n=1, alt="T"):
    return _record(contig, pos0, REFERENCE[contig][pos0:pos0 + n], alt)


RECORDS = [
    _at("c1", 50),                           # on a block's first base
    _at("c1", 149),                          # on a block's last base
    _at("c1", 100, 6, "A"),                  # a deletion inside a block
    _at("c1", 225, 10, "C"),                 # a deletion whose REF span leaves its block (and the track: 230 - 260 is no block)
    _at("c1", 298, 5, "A"),                  # ... and one that crosses the last block's end
    _at("c1", 20), _at("c1", 21),            # two adjacent records
    _at("c2", 3),                            # a contig with a record and no block
]


def test_compose_cuts_the_blocks_around_the_records():
    entries = Gvcf.compose(["c1", "c2", "c3"], BLOCKS, RECORDS, _ref_base)
    spans = [(c, s, e, rec) for c, s, e, _line, rec in entries]
    assert spans == [
        ("c1", 0, 20, False), ("c1", 20, 21, True), ("c1", 21, 22, True), ("c1", 22, 50, False),
        ("c1", 50, 51, True), ("c1", 51, 100, False), ("c1", 100, 106, True), ("c1", 106, 149, False), ("c1", 149, 150, True),
        ("c1", 150, 225, False), ("c1", 225, 235, True), ("c1", 260, 298, False), ("c1", 298, 303, True),
        ("c2", 3, 4, True), ("c3", 0, 50, False)]
    lines = {(c, s): line.decode() for c, s, _e, line, _rec in entries}
    assert lines["c1", 0] == "c1\t1\t.\tA\t<NON_REF>\t.\t.\tEND=20\tGT:GQ:MIN_DP\t./.:0:0\n"
    # the pieces of a cut block keep its minima
    assert lines["c1", 51] == "c1\t52\t.\tC\t<NON_REF>\t.\t.\tEND=100\tGT:GQ:MIN_DP\t0/0:50:18\n"
    assert lines["c1", 106] == "c1\t107\t.\tG\t<NON_REF>\t.\t.\tEND=149\tGT:GQ:MIN_DP\t0/0:50:18\n"
    assert lines["c3", 0] == "c3\t1\t.\tG\t<NON_REF>\t.\t.\tEND=50\tGT:GQ:MIN_DP\t0/0:50:25\n"
    # records verbatim
    for contig, pos, _n, line in RECORDS:
        assert lines[contig, pos].encode() == line
    with pytest.raises(ValueError):
        Gvcf.compose(["c1"], [], [_record("c9", 0, "A")], _ref_base)


def test_a_deletion_over_an_interval_boundary():
    """Two intervals share position 100; a deletion's REF span 97 - 103 lies over the boundary, in blocks of two bands."""
    track = _track()
    track.add("c1", (0, 100), ([0], [101], [6], [17], [50]))
    track.add("c1", (100, 200), ([100], [201], [4], [30], [31]))
    entries = Gvcf.compose(["c1", "c2", "c3"], track.finish(), [_at("c1", 97, 7, "T")], _ref_base)
    assert [(s, e, rec) for _c, s, e, _line, rec in entries] == [(0, 97, False), (97, 104, True), (104, 201, False)]
    assert entries[2][3].decode().endswith("END=201\tGT:GQ:MIN_DP\t0/0:31:30\n")


def _tiles(blocks, records, entries, looked_at):
    """Every position of looked_at[contig] (a set) in exactly one block line or under exactly one record's REF span."""
    count = {}
    for contig, s, e, _line, _rec in entries:
        for p in range(s, e):
            count[contig, p] = count.get((contig, p), 0) + 1
    for contig, positions in looked_at.items():
        for p in positions:
            assert count.get((contig, p), 0) == 1, (contig, p)
    for contig, s, e, _line, rec in entries:
        if not rec:
            assert all(p in looked_at[contig] for p in range(s, e)), (contig, s, e)


def test_the_tiling_property():
    looked_at = {"c1": set(), "c2": set(), "c3": set()}
    for contig, s, e, *_ in BLOCKS:
        looked_at[contig] |= set(range(s, e))
    entries = Gvcf.compose(["c1", "c2", "c3"], BLOCKS, RECORDS, _ref_base)
    _tiles(BLOCKS, RECORDS, entries, looked_at)
    # ... and on random blocks and non-overlapping records
    rng = np.random.default_rng(77)
    for _ in range(20):
        edges = np.unique(rng.integers(0, 400, 14))
        blocks = [("c1", int(a), int(b), int(rng.integers(0, 7)), int(rng.integers(0, 40)), int(rng.integers(0, 51)))
                  for a, b in zip(edges[:-1], edges[1:]) if rng.random() < 0.8]
        starts = np.unique(rng.integers(0, 390, 9))
        records = [_record("c1", int(p), REFERENCE["c1"][int(p):int(p) + int(min(rng.integers(1, 8), q - p))])
                   for p, q in zip(starts[:-1], starts[1:])]
        looked = {"c1": set(p for _c, s, e, *_ in blocks for p in range(s, e)) | set(p for _c, s, n, _l in records for p in range(s, s + n))}
        _tiles(blocks, records, Gvcf.compose(["c1"], blocks, records, _ref_base), looked)


class _Fasta(object):
    def get_reference_bytes(self, contig, start, stop):
        return REFERENCE[contig][start:stop].encode()


def test_the_file_and_its_index(tmp_path):
    header = ('##fileformat=VCFv4.2\n##contig=<ID=c1>\n##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">\n',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    full = str(tmp_path / "PEPPER_VARIANT_FULL.vcf.gz")
    out = bgzf.BgzfWriter(full)
    out.write(header[0] + header[1])
    file_order = sorted(RECORDS, key=lambda r: (r[0], r[1]))
    for _c, _p, _n, line in file_order:
        out.write(line)
    out.close()
    track = _track()
    for contig, s, e, band, dp, gq in BLOCKS:
        track.add(contig, (s, e - 1), ([s], [e], [band], [dp], [gq]))
    path = str(tmp_path / Gvcf.GVCF_NAME)
    logged = []
    assert Gvcf.write_gvcf(full, path, track, _Fasta(), log=logged.append) == (len(RECORDS), 7)
    assert len(logged) == 1 and "7 REFERENCE BLOCKS" in logged[0]
    with gzip.open(path, "rb") as fh:
        lines = fh.read().decode().splitlines(keepends=True)
    assert bgzf.read_bgzf(path).decode() == "".join(lines)
    head = [line for line in lines if line.startswith("#")]
    assert "".join(head) == header[0] + Gvcf.EXTRA_HEADER + header[1]
    assert "ID=NON_REF" in head[3] and "ID=END" in head[4] and "ID=MIN_DP" in head[5]
    body = [line for line in lines if not line.startswith("#")]
    assert [line.encode() for line in body if "<NON_REF>" not in line] == [r[3] for r in file_order]
    keys = [(["c1", "c2", "c3"].index(line.split("\t")[0]), int(line.split("\t")[1])) for line in body]
    assert keys == sorted(keys) and len(body) == len(RECORDS) + 7
    index = bgzf.parse_tbi(path + ".tbi")
    assert index["names"] == ["c1", "c2", "c3"] and all(ref["bins"] for ref in index["refs"])
