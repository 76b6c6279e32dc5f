"""The evidence the reference blocks are made from, restated for the tests (a helper, not a test).

evidence_numpy is the part of the reference's per-read walk (region_summary.cpp:353-565) that fills the letter, insert and `*`
columns of the image matrix, over the dict reads of pileup_utils.simulate_reads, beside coverage_cases.depth_numpy for the
coverage.  Expected blocks of the GPU tests are RefConfidence's numpy rule (gq_numpy, blocks_numpy) over it: nothing comes
from the code under test."""
import numpy as np

from coverage_cases import OP_D, OP_EQ, OP_I, OP_M, OP_N, OP_P, OP_S, OP_X, depth_numpy


def evidence_numpy(reads, reference, region_start, region_end, min_snp_baseq, min_indel_baseq, min_mapq):
    """-> (cov, ref_col, ins, star, ref_is_acgt), int64 / bool [region_end - region_start + 1]; reference[i] is the base of
    position region_start + i.

    A read counts as for depth_numpy.  A column of a position is only written where its reference base is one of ACGT
    (get_feature_index, :201-230).  Of a counted read: an aligned base inside the region whose quality is >= min_snp_baseq adds
    one to the column of its letter, forward or reverse -- to `*` when the letter is none of ACGT (:394-425); ref_col is the
    sum of both strands of the reference letter's column.  An insert whose anchor ref_position - 1 lies inside the region, with a
    read base in front of it, of at most 59 bases, whose anchor and inserted qualities sum to >= min_indel_baseq x their number
    adds one to the anchor's insert column (:432-462).  Every deleted base inside the region adds one to `*` (:542-552)."""
    n = region_end - region_start + 1
    ref = np.frombuffer(reference[:n].upper().encode(), np.uint8)
    assert len(ref) == n
    valid = np.isin(ref, np.frombuffer(b"ACGT", np.uint8))
    ref_col, ins, star = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for read in reads:
        if read["mapq"] < min_mapq or read["mapq"] <= 0:
            continue
        qual = np.asarray(read["qual"], np.int64)
        seq = np.frombuffer(read["seq"].upper().encode(), np.uint8)
        ref_position, read_index = int(read["pos"]), 0
        for op, k in read["cigar"]:
            if ref_position > region_end:
                break
            if op in (OP_M, OP_EQ, OP_X):
                lo, hi = max(ref_position, region_start), min(ref_position + k - 1, region_end)
                if lo <= hi:
                    at = slice(read_index + lo - ref_position, read_index + hi - ref_position + 1)
                    rows = slice(lo - region_start, hi - region_start + 1)
                    good = (qual[at] >= min_snp_baseq) & valid[rows]
                    letter = np.isin(seq[at], np.frombuffer(b"ACGT", np.uint8))
                    ref_col[rows] += good & letter & (seq[at] == ref[rows])
                    star[rows] += good & ~letter
                ref_position += k
                read_index += k
            elif op == OP_I:
                anchor = ref_position - 1
                if region_start <= anchor <= region_end and read_index - 1 >= 0 and k + 2 <= 61:
                    if qual[read_index - 1:read_index + k].sum() >= min_indel_baseq * (k + 1) and valid[anchor - region_start]:
                        ins[anchor - region_start] += 1
                read_index += k
            elif op == OP_D:
                lo, hi = max(ref_position, region_start), min(ref_position + k - 1, region_end)
                if lo <= hi:
                    star[lo - region_start:hi - region_start + 1] += valid[lo - region_start:hi - region_start + 1]
                ref_position += k
            elif op in (OP_N, OP_P):
                ref_position += k
                read_index += k
            elif op == OP_S:
                read_index += k
    cov = depth_numpy(reads, region_start, region_end, min_snp_baseq, min_indel_baseq, min_mapq)
    return cov, ref_col, ins, star, valid
