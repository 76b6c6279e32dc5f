"""Gvcf.compose with a ploidy (options.gvcf together with options.haploid_contigs): the pieces of the reference blocks are cut at
the ploidy boundaries too and a haploid piece writes GT 0 (. where MIN_DP is 0); without a ploidy the output is today's."""
import numpy as np

from pepper_amd.variant import Gvcf, Ploidy
from test_refconf_cpu import BLOCKS, RECORDS, REFERENCE, _at, _ref_base, _tiles

CONTIGS = ["c1", "c2", "c3"]


def _ploidy(given, par=None):
    table = {c: (np.array([s for s, _ in pairs], np.int64), np.array([e for _, e in pairs], np.int64)) for c, pairs in (par or {}).items()}
    contigs = CONTIGS if given == "*" else given.split(",")
    return Ploidy.Ploidy(given, contigs, table, "par.bed" if par else None)


def test_no_ploidy_is_todays_output():
    want = Gvcf.compose(CONTIGS, BLOCKS, RECORDS, _ref_base)
    assert Gvcf.compose(CONTIGS, BLOCKS, RECORDS, _ref_base, ploidy=None) == want
    # a ploidy whose haploid contig has neither a block nor a record changes nothing either
    assert Gvcf.compose(CONTIGS + ["c4"], BLOCKS, RECORDS, _ref_base, ploidy=_ploidy("c4")) == want
    assert Gvcf.block_line("c1", 4, 9, "A", 3, 7) == b"c1\t5\t.\tA\t<NON_REF>\t.\t.\tEND=9\tGT:GQ:MIN_DP\t0/0:7:3\n"
    assert Gvcf.block_line("c1", 4, 9, "A", 0, 0) == b"c1\t5\t.\tA\t<NON_REF>\t.\t.\tEND=9\tGT:GQ:MIN_DP\t./.:0:0\n"
    assert Gvcf.block_line("c1", 4, 9, "A", 3, 7, haploid=True) == b"c1\t5\t.\tA\t<NON_REF>\t.\t.\tEND=9\tGT:GQ:MIN_DP\t0:7:3\n"
    assert Gvcf.block_line("c1", 4, 9, "A", 0, 0, haploid=True) == b"c1\t5\t.\tA\t<NON_REF>\t.\t.\tEND=9\tGT:GQ:MIN_DP\t.:0:0\n"


def test_pieces_are_cut_at_the_par_edges():
    """c1 haploid with PARs on 10 - 30 (inside the depth-0 block, around the records at 20 and 21), 70 - 160 (over the block
    boundary at 150 and the records at 100 and 149) and 225 - 230 (its start on a record's first base); c3 haploid as a whole."""
    ploidy = _ploidy("c1,c3", {"c1": [(10, 30), (70, 160), (225, 230)]})
    entries = Gvcf.compose(CONTIGS, BLOCKS, RECORDS, _ref_base, ploidy=ploidy)
    spans = [(c, s, e, rec) for c, s, e, _line, rec in entries]
    assert spans == [
        ("c1", 0, 10, False), ("c1", 10, 20, False), ("c1", 20, 21, True), ("c1", 21, 22, True), ("c1", 22, 30, False),
        ("c1", 30, 50, False), ("c1", 50, 51, True), ("c1", 51, 70, False), ("c1", 70, 100, False), ("c1", 100, 106, True),
        ("c1", 106, 149, False), ("c1", 149, 150, True), ("c1", 150, 160, False), ("c1", 160, 225, False), ("c1", 225, 235, True),
        ("c1", 260, 298, False), ("c1", 298, 303, True), ("c2", 3, 4, True), ("c3", 0, 50, False)]
    gt = {(c, s): line.decode().rstrip("\n").split("\t")[9] for c, s, _e, line, rec in entries if not rec}
    assert gt == {("c1", 0): ".:0:0", ("c1", 10): "./.:0:0", ("c1", 22): "./.:0:0", ("c1", 30): ".:0:0",
                  ("c1", 51): "0:50:18", ("c1", 70): "0/0:50:18", ("c1", 106): "0/0:50:18", ("c1", 150): "0/0:8:2",
                  ("c1", 160): "0:8:2", ("c1", 260): "0:9:4", ("c3", 0): "0:50:25"}
    lines = {(c, s): line.decode() for c, s, _e, line, _rec in entries}
    assert lines["c1", 70] == "c1\t71\t.\tA\t<NON_REF>\t.\t.\tEND=100\tGT:GQ:MIN_DP\t0/0:50:18\n"
    assert lines["c1", 160] == "c1\t161\t.\tA\t<NON_REF>\t.\t.\tEND=225\tGT:GQ:MIN_DP\t0:8:2\n"
    for contig, pos, _n, line in RECORDS:                        # records verbatim
        assert lines[contig, pos].encode() == line
    # every position still lies in exactly one block line or under one record
    looked_at = {c: set() for c in CONTIGS}
    for contig, s, e, *_ in BLOCKS:
        looked_at[contig] |= set(range(s, e))
    _tiles(BLOCKS, RECORDS, entries, looked_at)
    # each block line has one ploidy
    for c, s, e, line, rec in entries:
        if not rec:
            assert len(set(ploidy.is_haploid(c, np.arange(s, e)).tolist())) == 1, (c, s, e)


def test_a_whole_haploid_run_and_an_edge_on_a_block_boundary():
    star = Gvcf.compose(CONTIGS, BLOCKS, RECORDS, _ref_base, ploidy=_ploidy("*"))
    plain = Gvcf.compose(CONTIGS, BLOCKS, RECORDS, _ref_base)
    assert [e[:3] + e[4:] for e in star] == [e[:3] + e[4:] for e in plain]               # the same pieces ...
    for a, b in zip(star, plain):                                                          # ... with the GT rewritten
        assert a[3] == (b[3] if b[4] else b[3].replace(b"\t0/0:", b"\t0:").replace(b"\t./.:", b"\t.:"))
    # PAR edges that coincide with block boundaries (50, 150) add no piece
    edge = Gvcf.compose(["c1"], BLOCKS[:4], [], _ref_base, ploidy=_ploidy("c1", {"c1": [(50, 150)]}))
    assert [(s, e, line.decode().rstrip("\n").split("\t")[9]) for _c, s, e, line, _r in edge] == [
        (0, 50, ".:0:0"), (50, 150, "0/0:50:18"), (150, 230, "0:8:2"), (260, 301, "0:9:4")]
    assert REFERENCE["c1"][70] == "A" and _at("c1", 70)[1] == 70
