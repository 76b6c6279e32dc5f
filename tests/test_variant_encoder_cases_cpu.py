"""The expectation of tests/test_gpu_variant_encoder_cases.py pinned on the CPU: on every hand-built pileup of
tests/variant_encoder_cases.py the restatement (oracle/pileup_oracle.cpp) equals the reference's own encoder
(oracle/_ref/libref_variant_encoder.so) on candidates, positions, depths, frequencies and images; a committed golden holds what
that build gave (the check that still runs where the build is absent); four small pileups have their counters written out by
hand.  The module also pins what the catalogue promises -- which operation is operation 63 / 64 and on which row, 128 / 129
exceptions in a pass, 512 / 513 votes in a tile, that every row a case is about lies inside a reported candidate window, which
cases the read clipping alters -- so that the GPU module cannot pass by missing an edge.  CPU only; exact integer parity."""
import importlib.util
import os

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import variant_encoder_cases as vc
from conftest import need_reference_build
from coverage_cases import depth_numpy

GOLDEN_NAME = "encoder_variant_cases.npz"
KEYS = ("positions", "depths", "candidate_frequency", "images")


@pytest.fixture(scope="module")
def oracle():
    return pu.load_restatement()


@pytest.fixture(scope="module")
def families():
    return {name: fn() for name, fn in vc.FAMILIES.items()}


@pytest.fixture(scope="module")
def wants(oracle, families):
    """The restatement's result of every case, computed once."""
    return {(family, name): pu.run_variant(oracle, vc.pileup(case), vc.params(case))
            for family, cases in families.items() for name, case in cases.items()}


def _same(got, want, what):
    assert got["candidates"] == want["candidates"], what
    for key in KEYS:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


@pytest.mark.parametrize("family", sorted(vc.FAMILIES))
def test_restatement_equals_reference_build_on_the_catalogue(families, wants, family):
    ref = pu.load_reference_encoder()
    if ref is None:
        need_reference_build("oracle/_ref")
    for name, case in families[family].items():
        _same(wants[family, name], pu.run_variant(ref, vc.pileup(case), vc.params(case), reference_impl=True), (family, name))


def _golden_module(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_variant_cases", os.path.join(golden_dir, "make_golden_variant_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_against_the_committed_golden(families, wants, golden_dir):
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    mod = _golden_module(golden_dir)
    seen = 0
    for family in vc.GOLDEN_FAMILIES:
        for name in families[family]:
            want = mod.as_golden(wants[family, name])
            for key in mod.KEYS:
                stored = g["%s__%s__%s" % (family, name, key)]
                assert stored.dtype == want[key].dtype and np.array_equal(stored, want[key]), (family, name, key)
            seen += 1
    assert seen * len(mod.KEYS) == len(g.files) and seen > 30


def test_golden_reproduces_from_its_script_and_stays_small(golden_dir):
    """What tests/golden/make_golden_variant_cases.py would write today is what is committed; data only, smaller than the
    largest file beside it."""
    ref = pu.load_reference_encoder()
    if ref is None:
        need_reference_build("oracle/_ref")
    want = _golden_module(golden_dir).golden_arrays(ref)
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    assert sorted(g.files) == sorted(want)
    for key, value in want.items():
        assert g[key].dtype == value.dtype and np.array_equal(g[key], value), key
    others = [os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if f != GOLDEN_NAME]
    assert os.path.getsize(os.path.join(golden_dir, GOLDEN_NAME)) < max(others)


# ---- rows worked out by hand ---------------------------------------------------------------------------------------------------
# columns: 0 reference code (A C G T other = 1 2 3 4 5), 1 / 2 / 3 the candidate's SNP code / insert length / deletion length,
# 4 forward strand coverage, 5 / 6 / 7 the candidate's forward support, 8 .. 14 forward A C G T I D *, 15 reverse strand coverage,
# 16 / 17 / 18 the candidate's reverse support, 19 .. 25 reverse A C G T I D *.  Counters are negative; the candidate's own
# columns in its rows are flipped to positive.  Window row 16 is the candidate's row.
CODE = {"A": 1, "C": 2, "G": 3, "T": 4}


def _both(oracle):
    out = [(oracle, False)]
    ref = pu.load_reference_encoder()
    if ref is not None:
        out.append((ref, True))
    return out


def _only(lib, is_ref, case):
    got = pu.run_variant(lib, vc.pileup(case), vc.params(case), reference_impl=is_ref)
    assert len(got["candidates"]) == 1
    return got, got["images"][0]


def _row(**cols):
    row = [0] * 26
    for key, value in cols.items():
        row[int(key[1:])] = value
    return row


def test_by_hand_rescued_anchor_under_a_70_base_insert(oracle, families):
    """min_snp_baseq = 10.  Row 19 (reference C): A, B, C carry G at quality 30 (forward, reverse, forward): coverage 3, SNP votes
    G 2 forward + 1 reverse, strand coverage -2 / -1, the G columns (10 and 21) -2 / -1.  Z's base on row 19 has quality 3: it is
    no coverage, no strand coverage and no letter.  Z's insert behind it sums 3 + 70 x 30 >= 10 x 71: it passes, and because its
    anchor base is below min_snp_baseq the anchor is rescued: coverage 3 + 1 = 4.  Its key would have 72 characters > 61: no
    insert count, no column I (12 / 23), no `2...` candidate.  The SNP: 3 / 4 >= 0.1; depth 4, frequency 3; its columns flipped:
    10 -> 2, 21 -> 1.  Row 20 (window row 17, reference C): A, B, C and Z (forward, quality 30): strand coverage -3 / -1, the C
    columns (9 and 20) -3 / -1."""
    case = families["by_hand"]["rescued_anchor"]
    assert case[2][19:21] == "CC"
    for lib, is_ref in _both(oracle):
        got, img = _only(lib, is_ref, case)
        assert got["candidates"] == ["1G"] and got["positions"].tolist() == [case[0] + 19]
        assert got["depths"].tolist() == [4] and got["candidate_frequency"].tolist() == [3]
        assert img[16].tolist() == _row(c0=2, c1=3, c4=-2, c5=2, c10=2, c15=-1, c16=1, c21=1)
        assert img[17].tolist() == _row(c0=2, c4=-3, c9=-3, c15=-1, c20=-1)


def test_by_hand_truncated_deletion_key(oracle, families):
    """The reference has 60 bases; three reads (forward, reverse, forward) end a match run on row 50 and delete 100 bases from
    row 51 on.  The key is "3" + reference.substr(50, 101) = the 10 bases that are left: 11 characters <= 61, counted (a key of
    102 would not be): deletion votes 3 over coverage 3.  Row 50 (reference T) anchors: strand coverage 0 / 0, the T columns (11
    and 22) -2 / -1, column D (13 and 24) -2 / -1 flipped to 2 / 1, deletion length 10 in column 3, support 2 / 1 in columns 7 and
    18.  Rows 51 .. 59 (window rows 17 .. 25 = 16 + 10 - 1): length and support again, the * columns (14 and 25) -2 / -1 flipped;
    window row 26 is row L, all zero, and so is everything behind it.  Row 49 (window row 15, reference T): strand coverage
    -2 / -1 -- it anchors nothing."""
    case = families["by_hand"]["truncated_deletion"]
    assert len(case[2]) == 60 and case[2][49:52] == "TTG"
    for lib, is_ref in _both(oracle):
        got, img = _only(lib, is_ref, case)
        assert got["candidates"] == ["3" + case[2][50:60]] and got["positions"].tolist() == [case[0] + 50]
        assert got["depths"].tolist() == [3] and got["candidate_frequency"].tolist() == [3]
        assert img[15].tolist() == _row(c0=4, c4=-2, c11=-2, c15=-1, c22=-1)
        assert img[16].tolist() == _row(c0=4, c3=10, c7=2, c11=-2, c13=2, c18=1, c22=-1, c24=1)
        for w in range(17, 26):
            assert img[w].tolist() == _row(c0=CODE[case[2][50 + w - 16]], c3=10, c7=2, c14=2, c18=1, c25=1), w
        assert not img[26:].any()


def test_by_hand_anchoring_last_base(oracle, families):
    """Three reads (forward, reverse, forward): M on rows 10 .. 15, an insert of GT, M on rows 16 .. 21.  Row 15 (reference A) is
    the last base of a match run with an insert behind it: its strand's coverage (columns 4 and 15) is NOT decremented, its
    letter's column (8 and 19) is: 0 / 0 and -2 / -1.  Insert votes 3 over coverage 3: the candidate 2AGT, length 3 in column 2,
    support 2 / 1 in columns 6 and 17, column I (12 and 23) -2 / -1 flipped.  Rows 14 and 16 (window rows 15 and 17, reference A
    and T) anchor nothing: strand coverage -2 / -1."""
    case = families["by_hand"]["anchoring_last_base"]
    assert case[2][14:17] == "AAT"
    for lib, is_ref in _both(oracle):
        got, img = _only(lib, is_ref, case)
        assert got["candidates"] == ["2AGT"] and got["positions"].tolist() == [case[0] + 15]
        assert got["depths"].tolist() == [3] and got["candidate_frequency"].tolist() == [3]
        assert img[16].tolist() == _row(c0=1, c2=3, c6=2, c8=-2, c12=2, c17=1, c19=-1, c23=1)
        assert img[15].tolist() == _row(c0=1, c4=-2, c8=-2, c15=-1, c19=-1)
        assert img[17].tolist() == _row(c0=4, c4=-2, c11=-2, c15=-1, c22=-1)


def test_by_hand_deep_column_clamp_and_wrap(oracle, families):
    """Forward reads: 127 on rows 0 .. 19, one more from row 5, one more from row 10; one reverse read.  Forward strand coverage
    (column 4, never clamped): -127 on rows 0 .. 4, -128 on 5 .. 9, -129 from row 10 on -- as int8: -127, -128 and +127 (the
    wrap).  The forward column of the reference letter holds the same count; columns 8 .. 10 (A C G) are not clamped, column 11
    (T) is: -125.  Row 12 (reference A): 20 of the reads carry C: A forward -109, C forward -20 flipped to 20 (column 9), support
    20 in column 5; coverage 130: depth min(130, 125) = 125, frequency 20.  Reverse: -1 everywhere."""
    case = families["by_hand"]["deep_column"]
    ref = case[2]
    assert ref[12] == "A" and "T" in ref[10:20] and "T" in ref[:5]
    for lib, is_ref in _both(oracle):
        got, img = _only(lib, is_ref, case)
        assert got["candidates"] == ["1C"] and got["depths"].tolist() == [125] and got["candidate_frequency"].tolist() == [20]
        assert not img[:4].any() and not img[24:].any()                 # rows -4 .. -1 and rows L .. of the window
        for r in range(20):
            n = 127 if r < 5 else 128 if r < 10 else 129
            col = 8 + "ACGT".index(ref[r])
            want = _row(c0=CODE[ref[r]], c4=-n, c15=-1)
            want[col] = max(-125, -n) if col == 11 else -n
            want[col + 11] = -1
            if r == 12:
                want[1], want[5], want[8], want[9] = 2, 20, -109, 20
            assert img[4 + r].tolist() == want, r
        wrapped = img.astype(np.int64).astype(np.int8)
        assert wrapped[4:24, 4].tolist() == [-127] * 5 + [-128] * 5 + [127] * 10
        t_row = 10 + ref[10:20].index("T")
        assert img[4 + t_row, 11] == -125 and wrapped[4 + t_row, 11] == -125


# ---- what the catalogue promises -----------------------------------------------------------------------------------------------
def _walk(read_, region_start):
    """(index, op, first row, rows) of every operation."""
    row, out = read_["pos"] - region_start, []
    for i, (op, n) in enumerate(read_["cigar"]):
        adv = n if op in (vc.M, vc.EQ, vc.X, vc.D, vc.N, vc.P) else 0
        out.append((i, op, row, adv))
        row += adv
    return out


def _is_witness(r):
    return r["cigar"] == [(vc.M, 5)]


def test_catalogue_puts_operations_63_and_64_where_it_says(families):
    mo = families["many_operations"]
    for name, kind in (("op64_insert_on_511", vc.I), ("op64_deletion_from_512", vc.D)):
        reads = [r for r in mo[name][3] if not _is_witness(r)]
        assert sorted(len(r["cigar"]) for r in reads) == [63, 64, 65, 128, 129, 200] and {r["reverse"] for r in reads} == {True, False}
        long = [_walk(r, mo[name][0]) for r in reads if len(r["cigar"]) > 64]
        assert len(long) == 4
        for ops in long:
            # operation 63 -- lane 63 of the first pass of the tile's walk, which starts at the read's operation 0 -- is a match run
            # that ends on row 511; operation 64 is the I / D it anchors: on row 511 / from row 512 on
            assert ops[0][2] >= 0 and ops[63][1] == vc.M and ops[63][2] + ops[63][3] - 1 == 511
            assert ops[64][1] == kind and ops[64][2] == 512
    reads = [r for r in mo["op64_match_over_1023"][3] if not _is_witness(r)]
    for r in reads:
        ops = _walk(r, mo["op64_match_over_1023"][0])
        if len(ops) > 64:
            assert ops[64][1] == vc.M and ops[64][2] <= 1023 < 1024 <= ops[64][2] + ops[64][3] - 1
    for r in mo["third_tile_record"][3]:
        if not _is_witness(r):
            owner = [o for o in _walk(r, mo["third_tile_record"][0]) if o[3] > 0 and o[2] <= 1024 <= o[2] + o[3] - 1]
            assert len(r["cigar"]) == 200 and len(owner) == 1 and owner[0][0] >= 64 and owner[0][2] < 1024


def test_catalogue_fills_the_exception_queue_as_it_says(families):
    """A base is an exception when it is not a clean match.  One match run over rows 512 .. 1023 is one pass of the tile's walk; at
    most eight records in the tile, so no wave walks two reads and every pass starts on an empty queue of 128."""
    eq = families["exception_queue"]
    for name, n in (("exceptions_128", 128), ("exceptions_129", 129), ("every_base", 512)):
        start, _end, ref, reads, _over = eq[name]
        in_tile = [r for r in reads if r["pos"] - start <= 1023 and r["pos"] - start + bu.ref_length(r["cigar"]) - 1 >= 512]
        assert len(in_tile) <= 8
        counts = []
        for r in in_tile:
            assert len(r["cigar"]) == 1 and r["cigar"][0][0] == vc.M and (r["qual"] >= 1).all()
            row0 = r["pos"] - start
            counts.append(sum(1 for k, b in enumerate(r["seq"]) if 512 <= row0 + k <= 1023 and b != ref[row0 + k]))
        assert sorted(counts) == [0, 0, 0, n, n]
        assert {r["reverse"] for r in in_tile if r["cigar"] == [(vc.M, 512)]} == {True, False}


def test_catalogue_casts_the_votes_it_says(families, wants):
    """Every I and D of these reads has its anchor in the second tile, a read base in front of it, default qualities and a short
    key: each is one vote.  votes_576: which 64 votes find the buffer full is the waves' order; the three reads that start last
    cast 96 votes, 43 of them on rows that pass and 53 on rows that do not (a deletion anchored where the others' inserts are lies on
    a passing row): fewer than 64 of either, so no order spills one kind alone from them."""
    assert sorted(families["votes"]) == ["votes_512", "votes_513", "votes_576"]
    for name, n in (("votes_512", 512), ("votes_513", 513), ("votes_576", 576)):
        start, _end, _ref, reads, over = families["votes"][name]
        assert not over
        per_read = [[first - 1 for _i, op, first, _n in _walk(r, start) if op in (vc.I, vc.D)] for r in reads]
        anchors = [a for mine in per_read for a in mine]
        assert len(anchors) == n and min(anchors) >= 512 and max(anchors) <= 1023
        passing = set((wants["votes", name]["positions"] - start).tolist())
        assert len(set(anchors) & passing) >= 32 and len(set(anchors) - passing) >= 16      # rows that pass and rows that do not
        if name == "votes_576":
            assert [r["pos"] - start for r in reads[-3:]] == [522, 524, 526] and [len(mine) for mine in per_read[-3:]] == [32, 32, 32]
            assert [sum(a in passing for a in mine) for mine in per_read[-3:]] == [6, 31, 6]
            assert sum(a not in passing for a in anchors) == 53 < n - 512          # whatever spills, some of it is on rows that pass


@pytest.mark.parametrize("family", sorted(vc.FAMILIES))
def test_every_named_row_lies_inside_a_reported_window(families, wants, family):
    """The oracle reports candidate windows only: a row that no window shows tests nothing."""
    named = 0
    for name, case in families[family].items():
        rows = (wants[family, name]["positions"] - case[0]).tolist()
        for edge in vc.EDGES[family, name]:
            assert any(abs(edge - row) <= 16 for row in rows), (family, name, edge)
            named += 1
        assert {True, False} == {r["reverse"] for r in case[3]} or len(case[3]) < 2, (family, name)
    assert named >= 2


def test_catalogue_shapes(families, wants):
    te = families["tile_edges"]
    for case in te.values():
        assert case[0] == vc.R0 > 0 and case[1] - case[0] + 1 == 1537
    starts = {(r["pos"] - vc.R0, r["cigar"][0]) for r in te["first_m"][3]}
    assert starts >= {(row, (vc.M, n)) for row in vc.TILE_ROWS for n in (1, 600)} | {(-1, (vc.M, 30)), (-600, (vc.M, 650)), (vc.L0, (vc.M, 5))}
    assert any(r["mapq"] == 0 for r in te["first_m"][3])
    lead = {(r["pos"] - vc.R0, tuple(op for op, _ in r["cigar"])) for r in te["leading"][3]}
    assert lead >= {(row, ops) for row in (0, 512, 1024, vc.L0 - 1)
                    for ops in ((vc.S, vc.I, vc.M), (vc.H, vc.S, vc.I, vc.M), (vc.I, vc.M), (vc.D, vc.M))}
    assert len(te["all"][3]) > max(len(c[3]) for n, c in te.items() if n != "all")
    lengths = [n for r in families["insert_quality"]["lengths"][3] for op, n in r["cigar"] if op == vc.I]
    assert sorted(set(lengths)) == sorted(vc.INSERT_LENGTHS) and 510 in vc.EDGES["insert_quality", "lengths"]
    # inserts of 60 and more and a deletion of 60 are no candidates; 59 are
    got = wants["insert_quality", "lengths"]
    assert max(len(c) for c in got["candidates"] if c[0] == "2") == 61 and len([c for c in got["candidates"] if c[0] == "2"]) == 11
    got = wants["deletion_keys", "lengths"]
    assert sorted(len(c) for c in got["candidates"] if c[0] == "3") == [3, 60, 61]
    # coverage 0 passes under min_coverage_threshold 0; one read short of the minimum does not
    assert wants["thresholds", "coverage_zero"]["depths"].tolist() == [0]
    assert (wants["thresholds", "coverage_at_minimum"]["positions"] - 45_000).tolist() == [20]
    assert [int(wants["thresholds", "depth_%d" % d]["depths"][0]) for d in vc.DEPTHS] == [125] * 5
    assert [int(wants["thresholds", "depth_%d" % d]["images"][0][16, 4] + wants["thresholds", "depth_%d" % d]["images"][0][16, 15])
            for d in vc.DEPTHS] == [-d for d in vc.DEPTHS]
    # the narrow window reports its two inner sites only
    assert (wants["region_edges", "narrow_window"]["positions"] - 46_000).tolist() == [30, 60]
    for kind, first in (("snp", "1"), ("insert", "2"), ("deletion", "3")):
        got = wants["region_edges", kind]
        rows = sorted({int(p) - 46_000 for p, c in zip(got["positions"], got["candidates"]) if c[0] == first})
        # (behind a match run that ends on row L - 1 the walk stops: no insert and no deletion is anchored there)
        assert rows == list(vc.EDGE_SITES if kind == "snp" else vc.EDGE_SITES[:-1]), kind
    mr = families["many_regions"]
    assert len(mr) == vc.N_REGIONS and {c[1] - c[0] + 1 for c in mr.values()} == {1, 2, 3, 513}
    assert {len(c[3]) for c in mr.values()} == {0, 1, 2, 3} and sum(len(wants["many_regions", n]["candidates"]) > 0 for n in mr) >= 50
    # the rare letters of `letters` are allele keys
    assert {"1n", "1N", "1R", "1*", "1a"} <= set(wants["letters", "qualities_30"]["candidates"])


def test_depth_exact_names_the_cases_whose_named_rows_stay_within_the_bins(families):
    """Every family has its entry.  The rows only the depth track shows (DEPTH_ONLY) are within the bins in every case; the
    cases of DEPTH_EXACT are those whose EDGES rows are too (row L, behind the region, has no depth)."""
    assert sorted(vc.DEPTH_EXACT) == sorted(vc.FAMILIES)
    depth_only = 0
    for family in sorted(vc.FAMILIES):
        exact = []
        for name, case in families[family].items():
            q = vc.params(case)
            depth = depth_numpy(case[3], case[0], case[1], q.min_snp_baseq, q.min_indel_baseq, 1)
            for r in vc.DEPTH_ONLY[family, name]:
                assert r >= len(depth) or int(depth[r]) <= 7, (family, name, r)
                depth_only += 1
            if all(int(depth[r]) <= 7 for r in vc.EDGES[family, name]):
                exact.append(name)
        assert sorted(exact) == sorted(vc.DEPTH_EXACT[family]), family
    assert depth_only >= 6


# what bam_utils.restated_get_reads (the reference's get_reads) does to the catalogue's reads before the walk sees them: an insert
# or a soft clip in front of the first aligned base is dropped with everything else in front of it; a read that starts on the
# fetch's last position is not fetched; operations behind the region's end are cut, and with them the anchoring bit of a match run
# that ends on the last row.  The packed form of these cases therefore tests the clip, not those edges of the walk.
ALTERED_BY_THE_CLIP = {("tile_edges", "first_m"), ("tile_edges", "leading"), ("tile_edges", "anchor_ends"), ("tile_edges", "gaps"),
                       ("tile_edges", "all"), ("insert_quality", "first_and_last"), ("region_edges", "insert"),
                       ("region_edges", "deletion")}


def _one_row_three_reads(case):
    """many_regions: the third read of a region starts on row 0; where the region has one row, that is the fetch's last position
    and the read is not fetched."""
    return case[1] == case[0] and len(case[3]) == 3


def test_which_cases_the_read_clipping_alters(oracle, families):
    assert set(vc.PACKED_FAMILIES) == set(vc.FAMILIES) - {"letters"} and set(vc.PACKED_AS_ONE_BATCH) <= set(vc.PACKED_FAMILIES)
    altered, with_candidates = set(), {}
    for family in vc.PACKED_FAMILIES:
        for name, case in families[family].items():
            reads, q = vc.bam_reads(case), vc.params(case)
            clipped = bu.restated_get_reads(reads, case[0], case[1], False, 1)
            for r in clipped:
                assert r["cigar"][0][0] in (vc.M, vc.EQ, vc.X), (family, name)
            a = pu.run_variant(oracle, pu.FlatPileup(case[0], case[1], case[2], reads), q)
            b = pu.run_variant(oracle, pu.FlatPileup(case[0], case[1], case[2], clipped), q)
            with_candidates[family] = with_candidates.get(family, 0) + (len(b["candidates"]) > 0)
            # (the regions of many_regions with fewer than three reads report nothing, packed or not)
            assert len(b["candidates"]) > 0 or family in vc.PACKED_AS_ONE_BATCH, (family, name)
            if a["candidates"] != b["candidates"] or any(not np.array_equal(a[k], b[k]) for k in KEYS):
                altered.add((family, name))
    mr = families["many_regions"]
    short = {("many_regions", name) for name, case in mr.items() if _one_row_three_reads(case)}
    assert len(short) >= 20 and with_candidates["many_regions"] >= 50
    assert altered == ALTERED_BY_THE_CLIP | short
    # one file for all of many_regions: every region's fetch sees its own reads and nobody else's
    every, per_case = vc.packed_batch(mr)
    for name, case, mine in per_case:
        assert bu.restated_get_reads(every, case[0], case[1], False, 1) == bu.restated_get_reads(mine, case[0], case[1], False, 1)
