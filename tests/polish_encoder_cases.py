"""Hand-built pileups for the polish summary encoder (pepper_amd/csrc/encoder_polish.hip), at the edges of its bookkeeping:
512-row tiles, the second record of an insert in front of a read's first aligned base, 64 CIGAR operations per wavefront
pass, the three scans that carry across 1 024, the first sizes of the record and insert-slot buffers.  No GPU, no tests: the
catalogue is read by tests/test_polish_encoder_cases_cpu.py (the restatement against the reference build, the goldens, rows
worked out by hand), tests/test_gpu_polish_encoder_cases.py (the kernels) and tests/golden/make_golden_polish_cases.py.

Every family is a function -> {name: (region_start, region_end, reference, reads, spans)}; `reads` is a list of dicts as
pileup_utils.FlatPileup takes them, `spans` a list of (start_pos, end_pos).  Nothing is drawn at random.  Positions are stated
as ROWS (position - region_start) in the comment next to the read that puts something there."""
import numpy as np

import pileup_utils as pu

M, I, D, N, S, H, P, EQ, X = pu.OP_M, pu.OP_I, pu.OP_D, pu.OP_N, pu.OP_S, pu.OP_H, pu.OP_P, pu.OP_EQ, pu.OP_X

R0 = 30_000                 # region_start of the three-tile region
L0 = 1537                   # three tiles of 512 rows and one row
EDGE_ROWS = (0, 511, 512, 1023, 1024, 1535, 1536)
DELETION_ONLY_ROWS = range(1160, 1255)     # of tile_edges()["gaps"]: inside two forward and one reverse deletion, nothing else
MAPQ0_ROWS = range(1300, 1350)             # of tile_edges()["gaps"]: under a read of mapping quality 0, nothing else


def base_at(pos):
    """The draft's base at a genomic position (any integer: reads reach in front of the regions)."""
    return "ACGT"[(pos * 7 + pos // 5 + pos // 64) & 3]


def reference(start, length):
    return "".join(base_at(start + i) for i in range(length))


def read(region_start, row, cigar, reverse, mapq=30, seq=None, salt=0):
    """A read whose alignment starts on `row` of the region (type_read.pos = region_start + row: the first reference-consuming
    operation starts there; S, H and I in front of it do not move it).  Without `seq`: aligned bases copy the draft except one
    in eleven, inserted bases cycle through ACGT, clipped bases are T and G."""
    pos = region_start + row
    if seq is None:
        out, at = [], pos
        for op, n in cigar:
            if op in (M, EQ, X):
                for k in range(n):
                    b = base_at(at + k)
                    out.append("ACGT"[("ACGT".index(b) + 1) & 3] if (at + k + salt) % 11 == 0 else b)
                at += n
            elif op == I:
                out.extend("ACGT"[(k + n + salt) & 3] for k in range(n))
            elif op == S:
                out.extend("TG"[k & 1] for k in range(n))
            elif op in (D, N, P):
                at += n
        seq = "".join(out)
    assert len(seq) == sum(n for op, n in cigar if op in (M, EQ, X, I, S)), (row, cigar)
    return dict(pos=pos, reverse=bool(reverse), mapq=mapq, seq=seq, qual=np.full(len(seq), 30, np.uint8), cigar=list(cigar))


def _case(region_start, length, reads, spans=None):
    reads = sorted(reads, key=lambda r: r["pos"])           # (stable: as a coordinate-sorted file delivers them)
    end = region_start + length - 1
    return (region_start, end, reference(region_start, length), reads, list(spans) if spans else [(region_start, end)])


# ---- tile_edges ---------------------------------------------------------------------------------------------------------------
def _first_m_reads(R):
    out = []
    for k, row in enumerate(EDGE_ROWS):
        out.append(read(R, row, [(M, 1)], k % 2, salt=k))                # row `row` alone (0, 511, 512, 1023, 1024, 1535, 1536)
        out.append(read(R, row, [(M, 600)], (k + 1) % 2, salt=k))        # rows row .. row + 599: from 1023 on past L - 1 = 1536
    return out


def _leading_insert_reads(R):
    """The first reference-consuming base on each edge row, an insert in front of it: anchored on the row before.  Row 0: anchor
    -1, dropped.  Rows 512 / 1024: anchors 511 / 1023, the last rows of the previous tiles, which these reads do not otherwise
    touch.  Row 1536 = L - 1: anchor 1535."""
    out = []
    for k, row in enumerate(EDGE_ROWS):
        out.append(read(R, row, [(I, 2), (M, 20)], k % 2, salt=k))                           # I anchored on row - 1; M on row .. row + 19
        out.append(read(R, row, [(S, 3), (I, 1), (M, 20)], (k + 1) % 2, salt=k + 1))         # the same behind a soft clip
        out.append(read(R, row, [(H, 5), (S, 2), (I, 3), (M, 20)], k % 2, salt=k + 2))       # ... behind a hard and a soft clip
    # the first aligned base on row L, the first one behind the region: I anchored on row L - 1 = 1536.  Under span = region the
    # read starts past end_pos and is not walked; under a span that ends behind the region (spans, scan_edges) it counts
    out.append(read(R, L0, [(I, 2), (M, 5)], 0, salt=1))
    out.append(read(R, L0, [(S, 1), (I, 5), (M, 5)], 1, salt=2))
    return out


def _inner_insert_reads(R, L):
    out = []
    for anchor in (510, 511, 512, 1023, 1024):
        for j, (n, rev) in enumerate(((1, 0), (4, 1), (2, 1))):
            # M on rows anchor - 30 + j .. anchor, I of n bases anchored on `anchor`, M on anchor + 1 .. anchor + 40
            out.append(read(R, anchor - 30 + j, [(M, 31 - j), (I, n), (M, 40)], rev, salt=anchor + j))
    out.append(read(R, 0, [(M, 1), (I, 3), (M, 10)], 0))                 # M on row 0, I anchored on row 0, M on rows 1 .. 10
    out.append(read(R, -5, [(M, 6), (I, 2), (M, 5)], 1))                 # M on rows -5 .. 0, I anchored on row 0, M on rows 1 .. 5
    out.append(read(R, L - 17, [(M, 17), (I, 4)], 0))                    # M on rows 1520 .. 1536 = L - 1, then I (starts on row L)
    out.append(read(R, L - 17, [(M, 17), (D, 5)], 1))                    # M on rows 1520 .. 1536, then D on rows L .. L + 4
    return out


def _gap_reads(R):
    out = []
    for j, op in enumerate((D, N, P)):
        out.append(read(R, 480, [(M, 20), (op, 31), (M, 20)], j % 2, salt=j))            # gap over rows 500 .. 530
        out.append(read(R, 500, [(M, 12), (op, 9), (M, 10)], (j + 1) % 2, salt=j))       # M 500 .. 511, gap starts on row 512 (.. 520)
        out.append(read(R, 490, [(M, 10), (op, 12), (M, 10)], j % 2, salt=j))            # gap 500 .. 511 ends on row 511, M from 512
        out.append(read(R, 390, [(M, 10), (op, 701), (M, 10)], (j + 1) % 2, salt=j))     # gap over rows 400 .. 1100: tile starts 512, 1024
        out.append(read(R, -20, [(M, 10), (op, 25), (M, 10)], j % 2, salt=j))            # gap over rows -10 .. 14: starts before row 0
        out.append(read(R, 1500, [(M, 20), (op, 40), (M, 5)], (j + 1) % 2, salt=j))      # gap over rows 1520 .. 1559: past L - 1 = 1536
    # rows 1160 .. 1254 lie inside all three deletions and under nothing else (DELETION_ONLY_ROWS): coverage 0, gap counts 2 and 1
    # (row 1159 is the third deletion's first row: it holds that deletion's coverage credit of 100)
    out.append(read(R, 1150, [(M, 5), (D, 100), (M, 5)], 0))             # M 1150 .. 1154, D 1155 .. 1254, M 1255 .. 1259; forward
    out.append(read(R, 1152, [(M, 5), (D, 100), (M, 5)], 0))             # M 1152 .. 1156, D 1157 .. 1256, M 1257 .. 1261; forward
    out.append(read(R, 1154, [(M, 5), (D, 100), (M, 5)], 1))             # M 1154 .. 1158, D 1159 .. 1258, M 1259 .. 1263; reverse
    out.append(read(R, 1300, [(M, 50)], 0, mapq=0))                      # rows 1300 .. 1349, mapping quality 0 (MAPQ0_ROWS): not counted
    out.append(read(R, -1, [(M, 30)], 1))                                # starts on row -1: rows -1 .. 28
    out.append(read(R, -600, [(M, 650)], 0))                             # starts on row -600: rows -600 .. 49
    return out


ODD_BASES = "acgtNnR*-"


def _odd_base_reads(R):
    ref8a, ref8b = reference(R + 695, 8), reference(R + 703, 8)
    return [read(R, 700, [(M, 9)], 0, seq=ODD_BASES),                                    # rows 700 .. 708
            read(R, 703, [(M, 9)], 1, seq=ODD_BASES),                                    # rows 703 .. 711
            read(R, 695, [(M, 8), (I, 9), (M, 8)], 1, seq=ref8a + ODD_BASES + ref8b),    # I of the nine bases anchored on row 702
            read(R, 695, [(M, 8), (I, 9), (M, 8)], 0, seq=ref8a + ODD_BASES[::-1] + ref8b)]


def tile_edges():
    """L = 1 537, span = region.  One case per kind of read, so that the stretches some of them need empty stay empty, and `all`:
    every read of the others in one pileup."""
    R, L = R0, L0
    parts = dict(first_m=_first_m_reads(R), leading_inserts=_leading_insert_reads(R), inner_inserts=_inner_insert_reads(R, L),
                 gaps=_gap_reads(R), odd_bases=_odd_base_reads(R))
    cases = {name: _case(R, L, reads) for name, reads in parts.items()}
    cases["all"] = _case(R, L, [r for reads in parts.values() for r in reads])
    return cases


# ---- many_operations ----------------------------------------------------------------------------------------------------------
PATTERN = ((M, 2), (I, 1), (M, 3), (D, 2))         # 7 reference rows and 6 read bases per 4 operations
# operations in front of the pattern so that operation 64 -- the first of the wavefront's second pass -- is of the wanted kind:
# operation i >= len(prefix) is PATTERN[(i - len(prefix)) % 4]
PREFIX = {I: [(S, 2), (M, 1), (D, 1)], D: [(S, 2)], M: [(H, 3), (S, 2)]}


def many_op_read(R, n_ops, kind, target_row, reverse, index=None, salt=0):
    """A read of n_ops operations whose operation `index` (64 where the read has one, else its last operation of that kind) is
    an I anchored on target_row / a D that starts on target_row / an M of 3 whose first row is target_row."""
    ops = (PREFIX[kind] + list(PATTERN) * ((n_ops + 3) // 4))[:n_ops]
    if index is None:
        index = 64 if n_ops > 64 else max(i for i in range(n_ops) if ops[i][0] == kind and (kind != M or ops[i][1] == 3))
    assert ops[index][0] == kind and (kind != M or ops[index][1] == 3)
    before = sum(n for op, n in ops[:index] if op in (M, D))      # reference rows in front of the operation
    first = target_row + 1 if kind == I else target_row           # (an insert is anchored on the row before its `first`)
    return read(R, first - before, ops, reverse, salt=salt)


OP_COUNTS = (63, 64, 65, 128, 129, 200)


def many_operations():
    R, L = R0, L0
    cases = {}
    # operation 64 (62 / 63 of the two shortest reads) is an I anchored on row 511 -- the last row of the first tile
    cases["op64_insert_on_511"] = _case(R, L, [many_op_read(R, n, I, 511, k % 2, salt=k) for k, n in enumerate(OP_COUNTS)])
    # ... a D over rows 512 .. 513: it starts on the first row of the second tile
    cases["op64_deletion_from_512"] = _case(R, L, [many_op_read(R, n, D, 512, (k + 1) % 2, salt=k) for k, n in enumerate(OP_COUNTS)])
    # ... an M over rows 1022 .. 1024 and one over 1023 .. 1025: both cross 1023 / 1024
    cases["op64_match_over_1023"] = _case(R, L, [many_op_read(R, n, M, 1022 + k % 2, k % 2, salt=k) for k, n in enumerate(OP_COUNTS)])
    # reads of 200 operations whose record for the third tile (rows 1024 ..) begins at operation 100 (an M over rows 1023 ..
    # 1025), at operation 148 (a D over rows 1023 .. 1024) and at operation 196 (an M over 1022 .. 1024)
    cases["third_tile_record"] = _case(R, L, [many_op_read(R, 200, M, 1023, 0, index=100),
                                              many_op_read(R, 200, D, 1023, 1, index=148, salt=1),
                                              many_op_read(R, 200, M, 1022, 1, index=196, salt=2)])
    return cases


# ---- spans --------------------------------------------------------------------------------------------------------------------
def spans():
    """The `all` pileup of tile_edges under spans that differ from the region (R = region_start, L = 1 537)."""
    R, L = R0, L0
    start, end, ref, reads, _ = tile_edges()["all"]
    return {"all": (start, end, ref, reads, [
        (R - 50, R + L + 49),              # wider on both sides: rows -50 .. L + 49, the rows outside the region are zero
        (R + 100, R + 900),                # narrower
        (R + 511, R + 512),                # the two rows either side of the first tile start
        (R + 512, R + 512),                # one row, the first of the second tile
        (R + L - 1, R + L + 5),            # from the last row on: end_pos lies past the region, the I behind row L - 1 is walked
        (R - 100, R - 1),                  # entirely in front of the region
        (R + L + 100, R + L + 200),        # entirely behind it
        (R, R)])}                          # row 0 alone


# ---- scan_edges ---------------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = (1, 2, 511, 512, 513, 1023, 1024, 1025, 2048, 2049)


def scan_edges():
    """Ten regions whose lengths sit either side of the 1 024 rows a scan block takes (and of the 512-row tile), each under its
    own span and under one that is two rows wider on both sides (so that the insert behind row L - 1 is walked)."""
    cases = {}
    for k, L in enumerate(SCAN_LENGTHS):
        R = 50_000 + 3_000 * k
        reads = [read(R, 0, [(M, 1), (I, 2)] + ([(M, L - 1)] if L > 1 else []), k % 2, salt=k),   # I anchored on row 0; M 0 .. L - 1
                 read(R, -2, [(M, 3), (I, 3), (M, L + 4)], (k + 1) % 2, salt=k),                   # M -2 .. 0, I anchored on row 0, M 1 .. L + 4
                 read(R, max(0, L - 10), [(M, min(L, 10)), (I, 4), (M, 5)], k % 2, salt=k + 1),    # M .. L - 1, I anchored on row L - 1
                 read(R, L - 1, [(M, 1), (I, 1 + k % 3)], (k + 1) % 2, salt=k),                    # M on row L - 1, I anchored on it
                 read(R, L, [(I, 2 + k % 2), (M, 3)], k % 2, salt=k + 3)]                          # first base on row L: I anchored on row L - 1
        if L > 1023:
            reads.append(read(R, 1000, [(M, 24), (I, 5), (M, 30)], 1, salt=k))                     # M 1000 .. 1023, I anchored on row 1023
            reads.append(read(R, 1010, [(M, 14), (I, 7), (M, 30)], 0, salt=k))                     # M 1010 .. 1023, I anchored on row 1023
        if L > 1024:
            reads.append(read(R, 1010, [(M, 15), (I, 6), (M, 20)], 0, salt=k + 2))                 # M 1010 .. 1024, I anchored on row 1024
        cases["L%d" % L] = _case(R, L, reads, [(R, R + L - 1), (R - 2, R + L + 1)])
    return cases


# ---- many_regions -------------------------------------------------------------------------------------------------------------
N_REGIONS = 1100
INSERT_REGIONS = (1022, 1023, 1024, 1025, 1026, N_REGIONS - 1)


def many_regions():
    """1 100 regions of 1 to 3 positions with 0 to 3 reads each; inserts in regions 1 022 .. 1 026 and in the last one: a carry
    lost past 1 024 regions (polish_bases_kernel) or 1 024 tiles (polish_tile_offsets_kernel: one tile per region) moves rows."""
    cases = {}
    for i in range(N_REGIONS):
        R = 100_000 + 10 * i
        L = 2 + i % 2 if i in INSERT_REGIONS else 1 + i % 3
        n_reads = (i * 7 + i // 4) % 4
        reads = [read(R, -1 + j, [(M, L + 2)], (i + j) % 2, salt=i + j) for j in range(n_reads)]      # rows -1 + j .. L + j
        if i in INSERT_REGIONS:
            # M on rows -1 .. 0, I of 1 + i % 4 bases anchored on row 0, M on rows 1 .. 3
            reads.append(read(R, -1, [(M, 2), (I, 1 + i % 4), (M, 3)], i % 2, salt=i))
            reads.append(read(R, 0, [(M, 1), (I, 2), (M, 2)], (i + 1) % 2, salt=i + 1))               # M row 0, I anchored on row 0
        cases["r%04d" % i] = _case(R, L, reads)
    return cases


# ---- staircase ----------------------------------------------------------------------------------------------------------------
def staircase():
    """40 reads, read k on rows k .. 63, all A (k even) or all C (k odd), reverse where k % 3 == 0: the coverage of row c < 40 is
    c + 1, and the quotients count / coverage * 254 take many values that are not integers."""
    R, L = 7_000, 64
    reads = [read(R, k, [(M, L - k)], k % 3 == 0, seq="AC"[k % 2] * (L - k)) for k in range(40)]
    return {"staircase": _case(R, L, reads)}


# ---- capacity -----------------------------------------------------------------------------------------------------------------
def capacity():
    """What outgrows the first sizes of a new handle's buffers.  long_inserts: L = 200, inserts of 3 000 bases on two anchors:
    6 000 insert slots > 2 * 200 + 4 096.  many_records: L = 20 000, 60 reads of M(6 .. 13) D(500 .. 1 100) repeated: every D
    that crosses a tile start is a record, ~39 per read, more than bases / 512 + 2 * reads + 1 024."""
    cases = {}
    R, L = 9_000, 200
    reads = [read(R, 0, [(M, 200)], 0), read(R, 10, [(M, 150)], 1, salt=1), read(R, -30, [(M, 100)], 0, salt=2),
             read(R, 20, [(M, 31), (I, 3000), (M, 40)], 0, salt=3),          # M 20 .. 50, I of 3 000 bases anchored on row 50
             read(R, 100, [(M, 21), (I, 3000), (M, 40)], 1, salt=4),         # M 100 .. 120, I of 3 000 bases anchored on row 120
             read(R, 30, [(M, 21), (I, 7), (M, 60)], 1, salt=5)]             # I of 7 anchored on row 50 as well
    cases["long_inserts"] = _case(R, L, reads)
    R, L = 5_000, 20_000
    reads = []
    for k in range(60):
        row = (k * 137) % 2000
        cigar, at, j = [], row, 0
        while at < L - 1200:
            n, d = 6 + (k * 5 + j * 3) % 8, 500 + (k * 37 + j * 101) % 601
            cigar += [(M, n), (D, d)]
            at += n + d
            j += 1
        cigar.append((M, 8))
        reads.append(read(R, row, cigar, k % 2, salt=k))
    cases["many_records"] = _case(R, L, reads)
    return cases


# ---- by_hand ------------------------------------------------------------------------------------------------------------------
def by_hand():
    """Two pileups small enough to work out on paper: tests/test_polish_encoder_cases_cpu.py holds their rows as literals."""
    cases = {}
    R = 500
    cases["deletion_only"] = _case(R, 30, [
        read(R, 2, [(M, 2), (D, 10), (M, 2)], 0, seq="ACGT"),      # AC on rows 2 .. 3, D rows 4 .. 13, GT on rows 14 .. 15; forward
        read(R, 3, [(M, 2), (D, 10), (M, 2)], 0, seq="ACGT"),      # AC on rows 3 .. 4, D rows 5 .. 14, GT on rows 15 .. 16; forward
        read(R, 4, [(M, 2), (D, 10), (M, 2)], 1, seq="ACGT")])     # AC on rows 4 .. 5, D rows 6 .. 15, GT on rows 16 .. 17; reverse
    R = 800
    cases["insert_on_deletion_start"] = _case(R, 10, [
        read(R, 0, [(M, 3), (I, 2), (M, 3)], 0, seq="GGG" + "AC" + "TTT"),   # G on rows 0 .. 2, AC anchored on row 2, T on rows 3 .. 5
        read(R, 1, [(M, 1), (D, 4), (M, 2)], 1, seq="CAA")])                  # C on row 1, D rows 2 .. 5 (starts on row 2), A on 6 .. 7
    return cases


FAMILIES = dict(by_hand=by_hand, tile_edges=tile_edges, many_operations=many_operations, spans=spans, scan_edges=scan_edges,
                many_regions=many_regions, staircase=staircase, capacity=capacity)
GOLDEN_FAMILIES = ("tile_edges", "many_operations", "spans", "scan_edges")


def pileup(case):
    return pu.FlatPileup(case[0], case[1], case[2], case[3])
