"""Target regions of a run (options.region_bed): a BED file read into one disjoint, ascending table per contig.

The reference's call_variant and make_images take --region_bed and read the resulting list only while training; at
inference the flag does nothing there.  Here it restricts the candidates: a candidate whose position p (0-based: the base of
a SNP, the anchor of an insert or a deletion) lies in a target -- start <= p < end for some interval of its contig, BED
coordinates being 0-based and half-open -- is kept, every other one does not exist.  Windows are gathered from the whole
summary matrix as before.  The table of a contig goes to the encoder (pa_encoder_set_targets), where target_rows_kernel
turns it into one verdict per matrix row; `contains` is the same rule in numpy.
"""
import re

import numpy as np

_INTEGER = re.compile(r"[+-]?[0-9]+", re.ASCII)


def _merge(pairs):
    """[(start, end)] with start < end, any order -> (starts, ends) int64: disjoint, ascending, non-touching."""
    pairs.sort()
    starts, ends = [], []
    for s, e in pairs:
        if ends and s <= ends[-1]:              # overlapping or touching
            ends[-1] = max(ends[-1], e)
        else:
            starts.append(s)
            ends.append(e)
    return np.array(starts, np.int64), np.array(ends, np.int64)


def parse_bed(path, contig_lengths):
    """-> ({contig: [(start, end)]} unmerged, the number of intervals on contigs that contig_lengths does not have).

    contig_lengths: {contig: length}.  Fields are split on any whitespace; blank lines and lines starting with `#`, `track` or
    `browser` are skipped; start and end are base-10 integers with 0 <= start <= end; start == end is empty and ignored; ends
    beyond the contig are clamped; contigs without a length are counted and ignored.  A malformed line raises ValueError with
    the file and the 1-based line number.  (Shared with Ploidy.parse: the PAR BED has the same syntax.)"""
    per_contig, unknown = {}, 0
    with open(path, "r") as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split()
            if not fields or fields[0].startswith("#") or fields[0] in ("track", "browser"):
                continue

            def bad(why):
                return ValueError("%s: line %d: %s" % (path, number, why))
            if len(fields) < 3:
                raise bad("a BED line needs contig, start and end")
            if not (_INTEGER.fullmatch(fields[1]) and _INTEGER.fullmatch(fields[2])):
                raise bad("start and end must be base-10 integers")
            start, end = int(fields[1]), int(fields[2])
            if start < 0:
                raise bad("negative start")
            if end < start:
                raise bad("end before start")
            length = contig_lengths.get(fields[0])
            if length is None:
                unknown += 1
                continue
            end = min(end, int(length))
            if start < end:
                per_contig.setdefault(fields[0], []).append((start, end))
    return per_contig, unknown


def read_bed(path, contig_lengths, log=None):
    """-> {contig: (starts int64[n], ends int64[n])}, merged; only contigs that keep at least one target.

    contig_lengths: {contig: length} of the FASTA.  The syntax is parse_bed's; contigs the FASTA does not have are ignored (log,
    if given, gets one line that counts them).  A malformed line raises ValueError with the file and the 1-based line number,
    and so does a file that leaves no target at all."""
    per_contig, unknown = parse_bed(path, contig_lengths)
    if unknown and log is not None:
        log("INFO: REGION BED: " + str(unknown) + " INTERVALS ON CONTIGS THE FASTA DOES NOT HAVE ARE IGNORED")
    if not per_contig:
        raise ValueError("%s: no target interval on any contig of the FASTA" % path)
    return {contig: _merge(pairs) for contig, pairs in per_contig.items()}


def contains(starts, ends, positions):
    """bool per position: start <= p < end for some interval of the (merged) table."""
    positions = np.asarray(positions, np.int64)
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    if len(starts) == 0:
        return np.zeros(positions.shape, bool)
    k = np.searchsorted(starts, positions, side="right") - 1        # the last interval that starts at or before p
    return (k >= 0) & (positions < ends[np.maximum(k, 0)])


def overlaps(starts, ends, s, e):
    """Does some target position p have s <= p <= e?  (An interval of the planner: closed at both ends.)"""
    k = int(np.searchsorted(np.asarray(ends, np.int64), s, side="right"))     # the first interval that ends behind s
    return k < len(starts) and int(starts[k]) <= e


def target_bases(starts, ends, s, e):
    """Target positions p with s <= p <= e."""
    lo, hi = np.maximum(np.asarray(starts, np.int64), s), np.minimum(np.asarray(ends, np.int64), e + 1)
    return int(np.maximum(hi - lo, 0).sum())


def table(bed_list, contig):
    """The table of `contig` as pa_encoder_set_targets takes it.  A contig without a target has no interval the planner kept,
    so a worker never asks for one: an empty table would mean `no restriction` to the encoder, hence the error."""
    entry = bed_list.get(contig)
    if entry is None or len(entry[0]) == 0:
        raise ValueError("region_bed: no target on contig " + str(contig))
    return np.ascontiguousarray(entry[0], np.int64), np.ascontiguousarray(entry[1], np.int64)


def filter_intervals(all_intervals, bed_list):
    """The planner's step behind split_intervals: (kept intervals, dropped count, dropped bases); an interval (contig, s, e)
    is kept iff a target position lies in [s, e].  Raises ValueError when nothing is left."""
    kept, dropped, dropped_bases = [], 0, 0
    for contig, s, e in all_intervals:
        entry = bed_list.get(contig)
        if entry is not None and overlaps(entry[0], entry[1], s, e):
            kept.append((contig, s, e))
        else:
            dropped += 1
            dropped_bases += e - s
    if not kept:
        raise ValueError("region_bed: no target position on the contigs and spans of this run")
    return kept, dropped, dropped_bases
