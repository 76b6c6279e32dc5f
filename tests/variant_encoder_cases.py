"""Hand-built pileups for the variant summary encoder (pepper_amd/csrc/encoder.hip: segment_reads_kernel, tile_count_kernel,
unpack_clip_kernel and the candidate enumeration), at the edges of its bookkeeping: 512-row tiles and the record the tile BEFORE
a read's first row gets, the anchoring last base of a match run, the three ways an insert's qualities are summed, the 61-byte
allele key, 64 CIGAR operations per wavefront pass with the next operation read across the pass boundary, the 128-entry
exception queue of a wave, the 512 indel votes a tile keeps in LDS, the +-125 clamp, the region's first and last 16 rows.  No
GPU, no tests: the catalogue is read by tests/test_variant_encoder_cases_cpu.py (the restatement against the reference build,
the golden, rows worked out by hand, what the catalogue promises), tests/test_gpu_variant_encoder_cases.py (the kernels) and
tests/golden/make_golden_variant_cases.py.

Every family is a function -> {name: (region_start, region_end, reference, reads, params_overrides)}; `reads` is a list of
dicts as pileup_utils.FlatPileup takes them, `params_overrides` what pileup_utils.make_params takes beside the candidate region
(params(case) builds them; the key "candidate_region" = (first row, last row) narrows the window, default: the region).  Nothing
is drawn at random.  Positions are stated as ROWS (position - region_start) in the comment next to the read that puts
something there.  Both strands appear in every case.

The oracle returns candidate windows only (33 rows around a candidate), so an edge no window shows tests nothing: EDGES[(family,
name)] lists the rows a case is about, and each of them must lie inside a reported window.  Where the reads of the edge make no
candidate of their own, _case() lays a WITNESS on the row: three reads of five bases (rows row - 2 .. row + 2; forward, reverse,
forward) that carry another base on `row` -- coverage 3 = min_coverage_threshold, a SNP in 3 of 3."""
import numpy as np

import pileup_utils as pu
import polish_encoder_cases as pc
from polish_encoder_cases import D, EQ, H, I, M, N, P, S, X, base_at, reference  # noqa: F401 -- the catalogue's vocabulary

R0 = 40_000                 # region_start of the three-tile region
L0 = 1537                   # three tiles of 512 rows and one row
TP = 512                    # rows of a tile
EDGES = {}                  # (family, name) -> rows (clamped into the region) that a reported candidate window must show
DEPTH_ONLY = {}             # (family, name) -> rows that no window can show (not walked, mapping quality 0): the depth track sees them


def alt_of(base):
    """Another base than `base` (the next of ACGT)."""
    return "ACGT"[("ACGT".index(base.upper()) + 1) & 3]


def read(region_start, row, cigar, reverse, mapq=30, seq=None, alts=(), low=None, qual=30, ins_qual=None, clip_qual=None,
         ref=None):
    """A read whose alignment starts on `row` of the region (type_read.pos = region_start + row: the first reference-consuming
    operation starts there; S, H and I in front of it do not move it).  Without `seq`: aligned bases copy the reference (base_at,
    or ref[row] where `ref` is given) but for the rows in `alts` and every base of an X run (alt_of), inserted bases cycle through
    ACGT, clipped bases are T and G; N and P take read bases too (A), as the reference's walk advances the read over them.
    Qualities: `qual`, but `low[row]` for the aligned base on `row`, `ins_qual` (a number or one per base) for inserted bases,
    `clip_qual` for clipped ones."""
    pos, low = region_start + row, low or {}
    out, q, at = [], [], pos
    for op, n in cigar:
        if op in (M, EQ, X):
            for k in range(n):
                r = at + k - region_start
                b = ref[r] if ref is not None and 0 <= r < len(ref) else base_at(at + k)
                out.append(alt_of(b) if (r in alts or op == X) and b.upper() in "ACGT" else b)
                q.append(low.get(r, qual))
            at += n
        elif op == I:
            out.extend("ACGT"[(k + n) & 3] for k in range(n))
            q.extend([qual if ins_qual is None else ins_qual] * n if np.isscalar(ins_qual) or ins_qual is None else list(ins_qual)[:n])
        elif op == S:
            out.extend("TG"[k & 1] for k in range(n))
            q.extend([qual if clip_qual is None else clip_qual] * n)
        elif op in (N, P):
            out.extend("A" * n)
            q.extend([qual] * n)
            at += n
        elif op == D:
            at += n
    if seq is not None:
        assert len(seq) == len(out), (row, cigar)
        out = list(seq)
    assert len(q) == len(out), (row, cigar)
    return dict(pos=pos, reverse=bool(reverse), mapq=mapq, seq="".join(out), qual=np.array(q, np.uint8), cigar=list(cigar))


def witness(region_start, row, ref=None):
    """Three reads over rows row - 2 .. row + 2 (forward, reverse, forward) with another base on `row`."""
    return [read(region_start, row - 2, [(M, 5)], k == 1, alts=(row,), ref=ref) for k in range(3)]


def _case(key, region_start, length, reads, edges, over=None, ref=None, witnesses=None, depth_only=()):
    """edges: the rows the case is about (rows outside the region count as the nearest row inside).  witnesses: the rows that get
    a witness; None: every edge; (): none -- the reads make their own candidates."""
    clamp = lambda r: min(max(r, 0), length - 1)                                   # noqa: E731
    ref = reference(region_start, length) if ref is None else ref
    reads = list(reads)
    for row in sorted({clamp(r) for r in (edges if witnesses is None else witnesses)}):
        reads += witness(region_start, row, ref)
    reads.sort(key=lambda r: r["pos"])           # (stable: as a coordinate-sorted file delivers them)
    EDGES[key] = tuple(sorted({clamp(r) for r in edges}))
    DEPTH_ONLY[key] = tuple(depth_only)
    return (region_start, region_start + length - 1, ref, reads, dict(over or {}))


def params(case):
    over = dict(case[4])
    lo, hi = over.pop("candidate_region", (0, case[1] - case[0]))
    return pu.make_params(case[0] + lo, case[0] + hi, **over)


def pileup(case):
    return pu.FlatPileup(case[0], case[1], case[2], case[3])


# ---- tile_edges ---------------------------------------------------------------------------------------------------------------
TILE_ROWS = (0, 511, 512, 1023, 1024, L0 - 2, L0 - 1)


def _first_m_reads(R):
    out = []
    for k, row in enumerate(TILE_ROWS):
        out.append(read(R, row, [(M, 1)], k % 2))                        # row `row` alone (0, 511, 512, 1023, 1024, 1535, 1536)
        out.append(read(R, row, [(M, 600)], (k + 1) % 2, alts=(row + 1,)))   # rows row .. row + 599: from 1023 on past L - 1 = 1536
    out.append(read(R, -1, [(M, 30)], 1))                                # starts on row -1: rows -1 .. 28
    out.append(read(R, -600, [(M, 650)], 0))                             # starts on row -600: rows -600 .. 49
    out.append(read(R, L0, [(M, 5)], 0, alts=(L0,)))                     # starts on row L: pos > region_end, not walked
    out.append(read(R, L0, [(S, 2), (I, 2), (M, 5)], 1))                 # ... nor is its insert (it would be anchored on row L - 1)
    # rows 1300 .. 1349 under a read of mapping quality 0 that disagrees on every fifth base: not counted
    out.append(read(R, 1300, [(M, 50)], 0, mapq=0, alts=tuple(range(1300, 1350, 5))))
    return out


def _leading_reads(R):
    """The first aligned row on 0, 512, 1024 and L - 1 = 1536 with an insert / a deletion in front of it: anchored on the row
    before.  Row 0: anchor -1, dropped.  Rows 512 / 1024: anchors 511 / 1023, the last rows of the previous tiles, which these
    reads do not otherwise touch.  Row 1536: anchor 1535."""
    out = []
    for k, row in enumerate((0, 512, 1024, L0 - 1)):
        out.append(read(R, row, [(S, 3), (I, 2), (M, 20)], k % 2, clip_qual=7))                   # I anchored on row - 1; its "anchor" base is a clipped one
        out.append(read(R, row, [(H, 5), (S, 2), (I, 2), (M, 20)], (k + 1) % 2, clip_qual=9))     # the same behind a hard clip
        out.append(read(R, row, [(I, 2), (M, 20)], k % 2))                                        # nothing in front: read_index - 1 < 0, dropped
        out.append(read(R, row, [(D, 3), (M, 20)], (k + 1) % 2))                                  # D on rows row .. row + 2, anchored on row - 1
        out.append(read(R, row, [(D, 3), (M, 20)], k % 2))
    return out


def _anchor_end_reads(R):
    out = []
    for rev in (0, 1):
        out.append(read(R, 490, [(M, 22), (I, 3), (M, 10)], rev))        # M 490 .. 511, I anchored on row 511 (the tile's last), M 512 ..
        out.append(read(R, 495, [(M, 17), (D, 4), (M, 10)], rev))        # M 495 .. 511, D on rows 512 .. 515 anchored on row 511
        out.append(read(R, L0 - 10, [(M, 10), (I, 3), (M, 4)], rev))     # M 1527 .. 1536 = L - 1, then I: it starts on row L, the walk stops first
        out.append(read(R, L0 - 12, [(M, 12), (D, 5), (M, 4)], rev))     # M 1525 .. 1536, then D on rows L ..: not walked either
    return out


def _gap_reads(R):
    out = []
    for j, op in enumerate((D, N, P)):
        out.append(read(R, -20, [(M, 10), (op, 25), (M, 10)], j % 2))             # gap over rows -10 .. 14: starts before row 0; M 15 .. 24
        out.append(read(R, 500, [(M, 12), (op, 9), (M, 10)], (j + 1) % 2))        # M 500 .. 511, gap starts on row 512 (.. 520)
        out.append(read(R, 490, [(M, 10), (op, 12), (M, 10)], j % 2))             # gap 500 .. 511 ends on row 511, M from 512
        out.append(read(R, 390, [(M, 10), (op, 701), (M, 10)], (j + 1) % 2))      # gap over rows 400 .. 1100: tile starts 512 and 1024
        out.append(read(R, 1500, [(M, 20), (op, 40), (M, 5)], j % 2))             # gap over rows 1520 .. 1559: past L - 1 = 1536
    return out


def tile_edges():
    """L = 1 537.  One case per kind of read, and `all`: every read of the others in one pileup."""
    R, L = R0, L0
    parts = dict(
        first_m=(_first_m_reads(R), TILE_ROWS + (-1, L0, 1310), None, (1300, 1349, L0)),
        leading=(_leading_reads(R), (0, 511, 512, 1023, 1024, L0 - 2, L0 - 1), None, ()),
        anchor_ends=(_anchor_end_reads(R), (511, 512, L0 - 1), None, ()),
        gaps=(_gap_reads(R), (0, 14, 399, 400, 499, 511, 512, 520, 1023, 1024, 1100, 1101, 1519, 1520, L0 - 1), None, ()))
    cases = {name: _case(("tile_edges", name), R, L, reads, edges, depth_only=depth) for name, (reads, edges, _w, depth) in parts.items()}
    every = [r for reads, _e, _w, _d in parts.values() for r in reads]
    edges = tuple(sorted({e for _r, e, _w, _d in parts.values() for e in e}))
    cases["all"] = _case(("tile_edges", "all"), R, L, every, edges, depth_only=(1300, 1349, L0))
    return cases


# ---- anchors ------------------------------------------------------------------------------------------------------------------
ANCHOR_FOLLOW = (I, D, S, N, None)
ANCHOR_ROWS = (19, 49, 79, 109, 139)           # the last row of the match run in front of each of ANCHOR_FOLLOW


def _anchor_reads(R, kind, rev, **kw):
    out = []
    for follow, last in zip(ANCHOR_FOLLOW, ANCHOR_ROWS):
        tail = {I: [(I, 2), (M, 6)], D: [(D, 2), (M, 6)], S: [(S, 4)], N: [(N, 3), (M, 6)], None: []}[follow]
        out.append(read(R, last - 9, [(kind, 10)] + tail, rev, **kw))    # kind on rows last - 9 .. last, then `follow`
    return out


def anchors():
    """L = 160.  The last base of a match run followed by I, by D (anchoring: its strand's coverage column is not decremented), by
    S, by N and by nothing (not anchoring), for M, = and X runs; the same with that base's quality below / at min_snp_baseq; match
    runs of one base that are their own anchor."""
    R, L = 41_000, 160
    cases = {}
    for name, kind in (("m_runs", M), ("eq_runs", EQ), ("x_runs", X)):
        reads = _anchor_reads(R, kind, 0) + _anchor_reads(R, kind, 1) + _anchor_reads(R, kind, 0)
        cases[name] = _case(("anchors", name), R, L, reads, ANCHOR_ROWS)
    for name, q in (("anchor_quality_below", 9), ("anchor_quality_at", 10)):
        low = {row: q for row in ANCHOR_ROWS}
        reads = _anchor_reads(R, M, 0, low=low) + _anchor_reads(R, M, 1, low=low) + _anchor_reads(R, EQ, 1)
        cases[name] = _case(("anchors", name), R, L, reads, ANCHOR_ROWS, over=dict(min_snp_baseq=10, min_indel_baseq=10))
    reads = []
    for k, kind in enumerate((M, EQ, X)):
        for rev in (0, 1, 0):
            reads.append(read(R, 20 + 30 * k, [(kind, 1), (I, 3), (M, 5)], rev))         # one base on row 20 / 50 / 80, I anchored on it
            reads.append(read(R, 30 + 30 * k, [(kind, 1), (D, 2), (M, 5)], rev))         # one base on row 30 / 60 / 90, D anchored on it
    cases["runs_of_one"] = _case(("anchors", "runs_of_one"), R, L, reads, (20, 30, 50, 60, 80, 90), witnesses=())
    return cases


# ---- insert_quality -----------------------------------------------------------------------------------------------------------
INSERT_LENGTHS = (1, 3, 4, 6, 7, 8, 31, 32, 33, 58, 59, 60, 63, 64, 65, 130)


def _ins_quals(n, k):
    return [(7 * j + 3 * n + k) % 38 + 2 for j in range(n)]


def insert_quality():
    """The quality sum of an insert (its anchor base and its bases): two unaligned dwords up to 8 bytes, a per-lane loop up to
    n_ins = len + 1 = 33, the wave's sum beyond; the key of anchor + bases is kept up to 61 characters ("2" + 60): 59 inserted
    bases are counted, 60 are not."""
    cases = {}
    R, L = 42_000, 40 * len(INSERT_LENGTHS) + 20
    reads = []
    for k, n in enumerate(INSERT_LENGTHS):
        a = 30 + 40 * k                                                   # anchors on rows 30, 70, ..: row 510 for 63 bases, 550 for 64
        for j, rev in enumerate((0, 1, 1)):
            reads.append(read(R, a - 9, [(M, 10), (I, n), (M, 10)], rev, ins_qual=_ins_quals(n, j)))
    cases["lengths"] = _case(("insert_quality", "lengths"), R, L, reads, tuple(30 + 40 * k for k in range(len(INSERT_LENGTHS))))
    # the sum exactly min_indel_baseq x (len + 1) and one below it, on each of the three ways of summing
    R, L = 42_000, 420
    reads, edges = [], []
    for k, n in enumerate((1, 7, 8, 20, 32, 33, 70)):
        for j, short in enumerate((0, 1)):
            a = 20 + 50 * k + 25 * j                                      # exact on rows 20, 70, ..; one short on rows 45, 95, ..
            edges.append(a)
            quals = [10] * n
            quals[-1] = 8 - short                                         # 12 (anchor) + 10 x (n - 1) + 8 = 10 x (n + 1)
            for rev in (0, 1, 0):
                reads.append(read(R, a - 9, [(M, 10), (I, n), (M, 10)], rev, low={a: 12}, ins_qual=quals))
    cases["sum_at_threshold"] = _case(("insert_quality", "sum_at_threshold"), R, L, reads, edges, over=dict(min_indel_baseq=10))
    # the rescue: the anchor base is below min_snp_baseq, the insert's sum passes: the anchor counts for the coverage; an insert
    # of 70 bases does that too, and nothing else (its key is too long)
    R, L = 42_000, 140
    reads = []
    for rev in (0, 1, 0):
        reads.append(read(R, 21, [(M, 10), (I, 4), (M, 10)], rev, low={30: 3}))          # anchor row 30, quality 3 < 10; 3 + 4 x 30 >= 10 x 5
        reads.append(read(R, 61, [(M, 10), (I, 70), (M, 10)], rev, low={70: 3}))         # anchor row 70: coverage + 1, no insert
        reads.append(read(R, 91, [(M, 10), (I, 4), (M, 10)], rev, low={100: 3}, ins_qual=2))   # anchor row 100: 3 + 4 x 2 < 50, no rescue
    cases["rescue"] = _case(("insert_quality", "rescue"), R, L, reads, (30, 70, 100), over=dict(min_snp_baseq=10, min_indel_baseq=10))
    R, L = 42_000, 120
    reads = []
    for rev in (0, 1, 0):
        reads.append(read(R, 11, [(M, 10), (I, 5)], rev))                                 # I anchored on row 20 ends the read
        reads.append(read(R, 41, [(M, 10), (I, 5), (S, 3)], rev))                         # ... on row 50, a soft clip behind it
        reads.append(read(R, 71, [(S, 4), (I, 3), (M, 10)], rev, clip_qual=1))            # first query bases behind a clip: anchored on row 70
        reads.append(read(R, 101, [(I, 3), (M, 10)], rev))                                # nothing in front: dropped (row 100)
    cases["first_and_last"] = _case(("insert_quality", "first_and_last"), R, L, reads, (20, 50, 70, 100))
    return cases


# ---- deletion_keys ------------------------------------------------------------------------------------------------------------
def _with(ref, changes):
    s = list(ref)
    for row, c in changes.items():
        s[row] = c
    return "".join(s)


def deletion_keys():
    cases = {}
    R, L = 43_000, 500
    reads = []
    for k, n in enumerate((1, 58, 59, 60)):
        for rev in (0, 1, 0):
            reads.append(read(R, 11 + 120 * k, [(M, 10), (D, n), (M, 10)], rev))          # anchors on rows 20, 140, 260, 380; 60 is not counted
    cases["lengths"] = _case(("deletion_keys", "lengths"), R, L, reads, (20, 140, 260, 380))
    # 100 deleted bases anchored 10 rows before the reference ends: substr shortens the key to 10 bases, and it is counted
    R, L = 43_000, 200
    reads = [read(R, L - 19, [(M, 10), (D, 100), (M, 5)], rev) for rev in (0, 1, 0)]       # M 181 .. 190 = L - 10, D from 191 on
    cases["past_the_reference"] = _case(("deletion_keys", "past_the_reference"), R, L, reads, (L - 10, L - 1), witnesses=())
    # the reference one base shorter than the region (ref_len = 199 < L): row 199 reads as no letter.  (The reference's own code
    # then reads reference_sequence[size()], the string's terminator, which is defined; any shorter and it reads behind its string)
    ref = reference(R, L - 1)
    reads = [read(R, L - 20, [(M, 10), (D, 100), (M, 5)], rev) for rev in (0, 1, 0)]       # M 180 .. 189 = ref_len - 10, D from 190 on
    cases["short_reference"] = _case(("deletion_keys", "short_reference"), R, L, reads, (L - 11, L - 2, L - 1), ref=ref, witnesses=(L - 1,))
    # anchored on a reference N (no column is written, the vote is) and on a lower-case base
    R, L = 43_000, 120
    ref = reference(R, L)
    ref = _with(ref, {30: "N", 31: "n", 60: ref[60].lower(), 61: ref[61].lower(), 62: ref[62].lower()})
    reads = []
    for rev in (0, 1, 0):
        reads.append(read(R, 21, [(M, 10), (D, 3), (M, 10)], rev, ref=ref))               # anchor row 30 = N, D over 31 (n) .. 33
        reads.append(read(R, 51, [(M, 10), (D, 3), (M, 10)], rev, ref=ref))               # anchor row 60 = lower case, D over 61 .. 63
    cases["odd_reference"] = _case(("deletion_keys", "odd_reference"), R, L, reads, (30, 60), ref=ref, witnesses=())
    # rows 30 .. 49 lie inside three deletions and under nothing else: coverage 0, the * columns alone; witnesses on 22 and 57
    reads = [read(R, 15 + j, [(M, 10), (D, 30 - 2 * j), (M, 10)], j == 1) for j in range(3)]   # D over 25 .. 54, 26 .. 53, 27 .. 52
    cases["deletion_only"] = _case(("deletion_keys", "deletion_only"), R, L, reads, (30, 49), witnesses=(20, 59))
    return cases


# ---- letters ------------------------------------------------------------------------------------------------------------------
ODD_BASES = "acgtNnR*"


def _letter_case(key, qual):
    R, L = 44_000, 120
    ref = reference(R, L)
    ref = _with(ref, dict([(r, ref[r].lower()) for r in range(40, 48)] + [(r, "N") for r in range(70, 74)] + [(r, "n") for r in range(74, 78)]))
    reads = []
    for row in (10, 40, 70):                                              # upper-case, lower-case and N / n reference under the eight bases
        for rev in (0, 1, 0, 1):
            reads.append(read(R, row, [(M, 8)], rev, seq=ODD_BASES, qual=qual, ref=ref))
            reads.append(read(R, row - 4, [(M, 16)], rev, ref=ref))       # ... beside reads that copy the reference (its case included)
    return _case(key, R, L, reads, (10, 17, 40, 47, 70, 77), ref=ref, witnesses=() if qual else (5, 22, 35, 52, 65, 82))


def letters():
    """Read bases acgtNnR* against upper-case and lower-case reference bases and a reference N: get_feature_index's column rules
    (no column under a reference N; `*` column for a letter outside ACGT), the case-sensitive mismatch test, rare-alphabet
    allele keys.  low_quality: the same bases at quality 0 -- nothing of them counts."""
    return {"qualities_30": _letter_case(("letters", "qualities_30"), 30), "low_quality": _letter_case(("letters", "low_quality"), 0)}


# ---- many_operations ----------------------------------------------------------------------------------------------------------
def many_operations():
    """The polish catalogue's reads of 63, 64, 65, 128, 129 and 200 operations (polish_encoder_cases.many_operations: operation
    64 an I anchored on row 511 / a D that starts on row 512 / an M over 1023 | 1024; a third-tile record that opens at operation
    100, 148, 196), with witnesses.  In the first two cases operation 63 is the match run whose last base -- on row 511 -- the
    I / D of operation 64 anchors: the anchoring bit of lane 63 comes from the next pass's first operation."""
    cases = {}
    for name, case in pc.many_operations().items():
        edges = dict(op64_insert_on_511=(511, 512), op64_deletion_from_512=(511, 512), op64_match_over_1023=(1023, 1024),
                     third_tile_record=(1023, 1024))[name]
        cases[name] = _case(("many_operations", name), case[0], case[1] - case[0] + 1, case[3], edges)
    return cases


# ---- exception_queue ----------------------------------------------------------------------------------------------------------
def exception_queue():
    """One match run over the whole second tile (rows 512 .. 1023: one pass of the walk, eight rows per lane) that disagrees with
    the reference on 128 bases (the wave's queue takes them in one piece), on 129 (row slot by row slot) and on every base.  On
    both strands, beside three clean reads: five records in the tile, so each wave walks one read and starts on an empty
    queue."""
    R, L = R0, L0
    cases = {}
    for name, rows in (("exceptions_128", range(512, 1024, 4)), ("exceptions_129", list(range(512, 1024, 4)) + [1022]),
                       ("every_base", range(512, 1024))):
        alts = tuple(rows)
        reads = [read(R, 512, [(M, 512)], rev, alts=alts) for rev in (0, 1)]              # rows 512 .. 1023
        reads += [read(R, 500, [(M, 530)], rev) for rev in (0, 1, 0)]                     # clean: rows 500 .. 1029
        cases[name] = _case(("exception_queue", name), R, L, reads, (512, 1022, 1023), witnesses=())
    return cases


# ---- votes --------------------------------------------------------------------------------------------------------------------
def votes():
    """Indel votes of one tile (rows 512 .. 1023): eight reads of (M4 I1) x 32 and eight of (M4 D1) x 32 = 512 votes, the last fit
    of the tile's LDS buffer; one more read with one insert = 513, the first spill.  The last of the sixteen starts two rows
    later: its 32 anchors are nobody else's and do not pass (1 of 16 reads).  Which votes find the buffer full depends on the
    order in which the waves reach it, so one spilled vote is of one kind only: votes_576 has 64 past the buffer, cast by the two
    reads that start last -- one whose inserts share the others' anchors (they pass) and one whose deletions are anchored where
    nobody else's are (they do not) -- behind the 32 non-passing votes of the sixteenth read.  No order is promised; but 64
    votes cannot all be non-passing (there are 53 such in the case: 26 + 26 deletions off the inserts' rows of the reads that
    start on rows 522 and 526, and the insert on row 651 -- the rest lie on rows that pass), and where the reads that start last
    are the ones that spill, their 96 votes are 43 on rows that pass and 53 on rows that do not."""
    R, L = R0, L0
    cases = {}
    for name, extra in (("votes_512", 0), ("votes_513", 1), ("votes_576", 64)):
        reads = [read(R, 520, [(M, 4), (I, 1)] * 32, k % 2) for k in range(8)]            # I anchored on rows 523, 527, .., 647
        reads += [read(R, 520 + (2 if k == 7 else 0), [(M, 4), (D, 1)] * 32, k % 2) for k in range(8)]   # D anchored on 523, 528, .., 678
        if extra == 1:
            reads.append(read(R, 700, [(M, 5), (I, 2), (M, 5)], 1))                       # I anchored on row 704
        if extra == 64:
            reads.append(read(R, 524, [(M, 4), (I, 1)] * 32, 1))                          # I anchored on rows 527, .., 647 (shared: they pass) and 651
            reads.append(read(R, 526, [(M, 4), (D, 1)] * 32, 0))                          # D anchored on rows 529, 534, .., 684: nobody else's
        cases[name] = _case(("votes", name), R, L, reads, (523, 647, 678), witnesses=())
    return cases


# ---- thresholds ---------------------------------------------------------------------------------------------------------------
DEPTHS = (125, 126, 127, 128, 129)


def thresholds():
    cases = {}
    # min_coverage_threshold 0: the anchors of three deletions have quality 0, so row 20 has coverage 0, three deletion votes over
    # max(1, 0) and passes: a candidate of depth 0
    R, L = 45_000, 60
    reads = [read(R, 11, [(M, 10), (D, 4), (M, 10)], rev, low={20: 0}) for rev in (0, 1, 0)]
    cases["coverage_zero"] = _case(("thresholds", "coverage_zero"), R, L, reads, (20,), over=dict(min_coverage_threshold=0), witnesses=())
    # coverage exactly min_coverage_threshold = 3 on row 20 (reported), 2 on row 40 (not)
    reads = [read(R, 15, [(M, 10)], rev, alts=(20,)) for rev in (0, 1, 0)] + [read(R, 35, [(M, 10)], rev, alts=(40,)) for rev in (0, 1)]
    cases["coverage_at_minimum"] = _case(("thresholds", "coverage_at_minimum"), R, L, reads, (20,), witnesses=())
    # 125 .. 129 reads on one row: columns 11 .. 24 are clamped to +-125, the others are not and wrap as int8 from 129 on
    for depth in DEPTHS:
        reads = [read(R, 0, [(M, 30)], k % 8 == 7, alts=(12,) if k % 5 == 0 else ()) for k in range(depth)]   # rows 0 .. 29; a SNP in a fifth
        cases["depth_%d" % depth] = _case(("thresholds", "depth_%d" % depth), R, 30, reads, (12,), witnesses=())
    return cases


# ---- region_edges -------------------------------------------------------------------------------------------------------------
LE = 100                                                                   # rows of the region_edges regions
EDGE_SITES = (0, 1, 15, 16, 17, LE - 18, LE - 17, LE - 16, LE - 2, LE - 1)


def region_edges():
    """L = 100.  A SNP / an insert / a deletion candidate on each of the rows 0, 1, 15, 16, 17, L - 18, L - 17, L - 16, L - 2 and
    L - 1: windows that reach in front of row 0 (zero rows) and to the all-zero row L and past it."""
    R, L = 46_000, LE
    cases = {}
    reads = [read(R, 0, [(M, L)], rev, alts=EDGE_SITES) for rev in (0, 1, 0)] + [read(R, -5, [(M, L + 10)], 1)]
    cases["snp"] = _case(("region_edges", "snp"), R, L, reads, EDGE_SITES, witnesses=())
    reads = [read(R, -5, [(M, L + 10)], 1)]
    for row in EDGE_SITES:
        for rev in (0, 1, 0):
            reads.append(read(R, max(0, row - 3), [(M, row - max(0, row - 3) + 1), (I, 2)] + ([(M, 3)] if row < L - 1 else []), rev))
    cases["insert"] = _case(("region_edges", "insert"), R, L, reads, EDGE_SITES, witnesses=())
    reads = [read(R, -5, [(M, L + 10)], 1)]
    for k, row in enumerate(EDGE_SITES):
        n = (2, 20, 3, 16, 17, 25, 2, 20, 5, 4)[k]                        # 20 from row 1: spill rows to window row 32; from L - 16, L - 2, L - 1: to row L and past it
        for rev in (0, 1, 0):
            reads.append(read(R, max(0, row - 3), [(M, row - max(0, row - 3) + 1), (D, n), (M, 3)], rev))
    cases["deletion"] = _case(("region_edges", "deletion"), R, L, reads, EDGE_SITES, witnesses=())
    # a candidate window narrower than the region: SNPs on rows 29 and 61 lie just outside it
    reads = [read(R, 0, [(M, L)], rev, alts=(29, 30, 60, 61)) for rev in (0, 1, 0)]
    cases["narrow_window"] = _case(("region_edges", "narrow_window"), R, L, reads, (30, 60), over=dict(candidate_region=(30, 60)), witnesses=())
    return cases


# ---- many_regions -------------------------------------------------------------------------------------------------------------
N_REGIONS = 300


def many_regions():
    """300 regions of 1, 2, 3 and (every tenth) 513 rows with 0 to 3 reads each: every matrix starts on a row that is a multiple
    of 16, every region's site and vote lists lie between its neighbours'.  Regions with three reads carry a SNP on row 0 and an
    insert anchored on it."""
    cases = {}
    for i in range(N_REGIONS):
        R = 100_000 + 1_000 * i
        L = 513 if i % 10 == 9 else 1 + i % 3
        n_reads = (i * 7 + i // 4) % 4
        reads = [read(R, -1 + (j == 2), [(M, 2 - (j == 2)), (I, 1 + i % 3), (M, L + 1)], (i + j) % 2, alts=(0, L - 1)) for j in range(n_reads)]
        cases["r%03d" % i] = _case(("many_regions", "r%03d" % i), R, L, reads, (0, L - 1) if n_reads == 3 else (), witnesses=())
    return cases


# ---- by_hand ------------------------------------------------------------------------------------------------------------------
def by_hand():
    """Pileups small enough to work out on paper: tests/test_variant_encoder_cases_cpu.py holds their counters as literals."""
    cases = {}
    R = 600
    # A, B, C: M on rows 5 .. 34, another base on row 19 (forward, reverse, forward).  Z: M 10 .. 19, I of 70 anchored on row 19
    # whose base has quality 3 < min_snp_baseq = 10, M 20 .. 29; forward
    reads = [read(R, 5, [(M, 30)], rev, alts=(19,)) for rev in (0, 1, 0)] + [read(R, 10, [(M, 10), (I, 70), (M, 10)], 0, low={19: 3})]
    cases["rescued_anchor"] = _case(("by_hand", "rescued_anchor"), R, 40, reads, (19,), over=dict(min_snp_baseq=10, min_indel_baseq=10), witnesses=())
    R = 700
    # three reads (forward, reverse, forward): M on rows 41 .. 50, D of 100 from row 51 on, M; the reference has 60 bases
    reads = [read(R, 41, [(M, 10), (D, 100), (M, 5)], rev) for rev in (0, 1, 0)]
    cases["truncated_deletion"] = _case(("by_hand", "truncated_deletion"), R, 60, reads, (50,), witnesses=())
    R = 800
    # three reads (forward, reverse, forward): M on rows 10 .. 15, I of 2 anchored on row 15, M on rows 16 .. 21
    reads = [read(R, 10, [(M, 6), (I, 2), (M, 6)], rev) for rev in (0, 1, 0)]
    cases["anchoring_last_base"] = _case(("by_hand", "anchoring_last_base"), R, 40, reads, (15,), witnesses=())
    R = 900
    # forward reads only: 127 over rows 0 .. 19, one over 5 .. 19, one over 10 .. 19: depth 127, 128, 129; twenty of the first
    # carry another base on row 12; one reverse read over rows 0 .. 19
    reads = [read(R, 0, [(M, 20)], 0, alts=(12,) if k < 20 else ()) for k in range(127)]
    reads += [read(R, 5, [(M, 15)], 0), read(R, 10, [(M, 10)], 0), read(R, 0, [(M, 20)], 1)]
    cases["deep_column"] = _case(("by_hand", "deep_column"), R, 20, reads, (12,), witnesses=())
    return cases


FAMILIES = dict(by_hand=by_hand, tile_edges=tile_edges, anchors=anchors, insert_quality=insert_quality, deletion_keys=deletion_keys,
                letters=letters, many_operations=many_operations, exception_queue=exception_queue, votes=votes,
                thresholds=thresholds, region_edges=region_edges, many_regions=many_regions)
GOLDEN_FAMILIES = ("by_hand", "tile_edges", "anchors", "insert_quality", "deletion_keys", "letters", "many_operations", "thresholds",
                   "region_edges")
# The depth track (bins [0 .. 7]) runs on every case of every family and is compared on every row, the rows no window shows among
# them.  Eight bins tell depths 0 .. 7 apart and put everything deeper into the last one.  The DEPTH_ONLY rows of every case stay
# at 7 or below, so the track sees them exactly (tile_edges: the rows under the read of mapping quality 0 hold the two 600-base
# reads and the witness, row L no depth at all -- while the tile-edge rows themselves, under every read of the case and their
# witnesses, go past 7).  DEPTH_EXACT names the cases whose EDGES rows stay at 7 or below too: there the track tells the exact
# depth of every row the case is about (tests/test_variant_encoder_cases_cpu.py checks that it is exactly those cases).  The
# others -- the tile-edge, 64-operation and vote cases pile more than seven reads on their rows -- are compared all the same: their
# runs must equal the numpy rule's, which takes depth 8 and depth 20 for one class.
DEPTH_EXACT = {
    "by_hand": ("rescued_anchor", "truncated_deletion", "anchoring_last_base"),
    "tile_edges": (),
    "anchors": ("m_runs", "eq_runs", "x_runs", "anchor_quality_below", "anchor_quality_at", "runs_of_one"),
    "insert_quality": ("lengths", "sum_at_threshold", "rescue", "first_and_last"),
    "deletion_keys": ("lengths", "past_the_reference", "short_reference", "odd_reference", "deletion_only"),
    "letters": ("low_quality",),
    "many_operations": (),
    "exception_queue": ("exceptions_128", "exceptions_129", "every_base"),
    "votes": (),
    "thresholds": ("coverage_zero", "coverage_at_minimum"),
    "region_edges": ("snp", "narrow_window"),
    "many_regions": tuple("r%03d" % i for i in range(N_REGIONS)),
}

# ---- the packed form ----------------------------------------------------------------------------------------------------------
# Families that also run from a BAM (PackedEncoder.pack + encode: unpack_clip_kernel clips and decodes the reads on the device):
# all but `letters`.  A BAM holds its bases in four bits, upper case, of the alphabet =ACMGRSVTWYHKDBN: the lower-case letters and
# the `*` that family is about cannot be written, and bam_reads() would leave only its clean reads.  (Reference bases in lower case
# and a reference N reach the packed form through deletion_keys / odd_reference.)  many_regions is packed as ONE file and ONE
# pack() call over all of its regions: packed_batch().
PACKED_FAMILIES = ("by_hand", "tile_edges", "anchors", "insert_quality", "deletion_keys", "many_operations", "exception_queue", "votes",
                   "thresholds", "region_edges", "many_regions")
PACKED_AS_ONE_BATCH = ("many_regions",)
BAM_LETTERS = set("=ACMGRSVTWYHKDBN")


def bam_reads(case):
    """The case's reads as a BAM can hold them, named in file order: bases in upper case; none with an N or P operation (there
    the variant walk takes read bases a BAM record does not have) or with a base outside the BAM alphabet."""
    out = []
    for r in case[3]:
        seq = r["seq"].upper()
        if any(op in (N, P) for op, _ in r["cigar"]) or not set(seq) <= BAM_LETTERS:
            continue
        out.append(dict(r, seq=seq, name="q%d" % len(out)))
    return out


def packed_batch(cases):
    """The cases of a family whose regions lie apart on one contig, in catalogue order -> (the reads of all of them as one file
    holds them: sorted by position, named in file order; [(name, case, its reads among them)])."""
    every, per_case = [], []
    for name, case in cases.items():
        mine = [dict(r, name="q%d" % (len(every) + k)) for k, r in enumerate(bam_reads(case))]
        every += mine
        per_case.append((name, case, mine))
    assert all(a["pos"] <= b["pos"] for a, b in zip(every, every[1:]))
    return every, per_case
