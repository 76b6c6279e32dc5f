"""The depth the coverage track reports, restated for the tests (a helper, not a test).

depth_numpy is the coverage part of the reference's per-read walk (region_summary.cpp:353-470) over the dict reads of
pileup_utils.simulate_reads -- nothing else of the walk: which bases count, which insert anchors are rescued, what advances
the reference and the read.  Expected runs and totals of the GPU tests are Coverage.runs_numpy / totals_numpy of it."""
import numpy as np

OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = range(9)


def depth_numpy(reads, region_start, region_end, min_snp_baseq, min_indel_baseq, min_mapq):
    """-> int64 [region_end - region_start + 1]: coverage_vector of the region (both ends inclusive).

    A read counts when its mapping quality is >= min_mapq (the fetch's filter) and > 0 (:619).  Of a counted read: every
    aligned base (M, =, X) inside the region whose quality is >= min_snp_baseq adds one to its position (:378-379); an insert
    whose anchor ref_position - 1 lies inside the region and has a read base in front of it (read_index - 1 >= 0) adds one to the
    anchor when the qualities of the anchor base and the inserted bases sum to >= min_indel_baseq x their number while the
    anchor base's own quality is below min_snp_baseq (:432-454); deleted bases add nothing (:550 is commented out); N and P
    advance the reference and -- through the missing break -- the read (:556-561); S advances the read; the walk of a read
    stops at the first operation that starts behind the region (:355)."""
    cov = np.zeros(region_end - region_start + 1, np.int64)
    for read in reads:
        if read["mapq"] < min_mapq or read["mapq"] <= 0:
            continue
        qual = np.asarray(read["qual"], np.int64)
        ref_position, read_index = int(read["pos"]), 0
        for op, n in read["cigar"]:
            if ref_position > region_end:
                break
            if op in (OP_M, OP_EQ, OP_X):
                lo, hi = max(ref_position, region_start), min(ref_position + n - 1, region_end)
                if lo <= hi:
                    q = qual[read_index + lo - ref_position:read_index + hi - ref_position + 1]
                    cov[lo - region_start:hi - region_start + 1] += q >= min_snp_baseq
                ref_position += n
                read_index += n
            elif op == OP_I:
                if region_start <= ref_position - 1 <= region_end and read_index - 1 >= 0:
                    span = qual[read_index - 1:read_index + n]
                    if span.sum() >= min_indel_baseq * (n + 1) and span[0] < min_snp_baseq:
                        cov[ref_position - 1 - region_start] += 1
                read_index += n
            elif op == OP_D:
                ref_position += n
            elif op in (OP_N, OP_P):
                ref_position += n
                read_index += n
            elif op == OP_S:
                read_index += n
    return cov
