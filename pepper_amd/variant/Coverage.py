"""Depth classes of the positions a run looked at (options.coverage_bed): the callable-regions track beside the VCF.

A position without a record in the VCF may have reads that agree with the reference, or too few reads to propose anything.
The encoder decides that for every position -- tile_count_kernel refuses a site whose coverage is below
min_coverage_threshold -- and with depth bins set (pa_encoder_set_depth_bins) it reports the coverage it saw, binned and
run-length encoded on the device (depth_runs_kernel, pepper_amd/csrc/encoder.hip).  The depth of a position is the
reference's coverage_vector (region_summary.cpp:379, :454): aligned bases with quality >= min_snp_baseq, insert anchors
rescued by the indel quality rule, of reads that pass min_mapq and have mapping quality > 0, after the reservoir sample where
one was drawn; deleted bases do not count.

Bins are ascending lower bounds b[0] = 0 < b[1] < ... (at most 8): bin k holds the depths in [b[k], b[k + 1]), the last bin
is open above.  `runs_numpy` is the device's rule in numpy; `CoverageTrack` collects the workers' runs and writes
PEPPER_VARIANT_COVERAGE.bed: contig, start, end (0-based, half-open), label.
"""
import math
import threading

import numpy as np

MAX_BINS = 8
OFF_TARGET = -1                      # the bin of a position outside every target (pa_encoder_set_targets): never written
BED_NAME = "PEPPER_VARIANT_COVERAGE.bed"


def default_bins(min_coverage_threshold):
    """-> (bounds, labels): NO_COVERAGE from 0, LOW_COVERAGE from 1, CALLABLE from ceil(min_coverage_threshold), without the
    classes that are empty (a threshold of 1 leaves no LOW_COVERAGE, one of 0 or less only CALLABLE)."""
    callable_from = max(0, int(math.ceil(float(min_coverage_threshold))))
    if callable_from <= 0:
        return (0,), ["CALLABLE"]
    if callable_from == 1:
        return (0, 1), ["NO_COVERAGE", "CALLABLE"]
    return (0, 1, callable_from), ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]


def parse_bins(bins=None, min_coverage_threshold=None):
    """-> (int32 lower bounds, labels).  bins: None (the default classes of `min_coverage_threshold`), a sequence of integers or
    their text "0,1,5,20"; such bins get mosdepth's labels lo:hi, the last one lo:inf.  ValueError, naming the entry: more than
    8 bins, none at all, a first bound that is not 0, a bound that is not above the one before it or not an integer below 2^31."""
    if bins is None or (isinstance(bins, str) and bins.strip() == ""):
        if min_coverage_threshold is None:
            raise ValueError("coverage bins: neither bins nor min_coverage_threshold given")
        bounds, labels = default_bins(min_coverage_threshold)
        return np.array(bounds, np.int32), labels
    fields = [f.strip() for f in bins.split(",")] if isinstance(bins, str) else list(bins)
    if len(fields) == 0:
        raise ValueError("coverage bins: no bin")
    if len(fields) > MAX_BINS:
        raise ValueError("coverage bins: entry %d is one more than the %d bins a table may have" % (MAX_BINS, MAX_BINS))
    bounds = []
    for k, field in enumerate(fields):
        try:
            if isinstance(field, (float, np.floating)) and float(field) != int(field):
                raise ValueError
            value = int(field)
        except (TypeError, ValueError):
            raise ValueError("coverage bins: entry %d (%r) is not an integer" % (k, field)) from None
        if k == 0 and value != 0:
            raise ValueError("coverage bins: entry 0 must be 0, not %d" % value)
        if k > 0 and value <= bounds[-1]:
            raise ValueError("coverage bins: entry %d (%d) is not above the one before it (%d)" % (k, value, bounds[-1]))
        if value >= 1 << 31:
            raise ValueError("coverage bins: entry %d (%d) does not fit 31 bits" % (k, value))
        bounds.append(value)
    labels = ["%d:%d" % (lo, hi) for lo, hi in zip(bounds, bounds[1:])] + ["%d:inf" % bounds[-1]]
    return np.array(bounds, np.int32), labels


def runs_numpy(depths, first_position, bins, on_target=None):
    """The rule of depth_runs_kernel: depths[i] is the depth of position first_position + i -> (starts, ends, bins) of the
    maximal runs of equal bin, int64 / int64 / int32, ends half-open.  on_target (bool per position; None: all): a position
    outside has the bin OFF_TARGET, and its runs are reported like any other."""
    depths = np.asarray(depths, np.int64)
    bounds = np.asarray(bins, np.int64)
    which = (np.searchsorted(bounds, depths, side="right") - 1).astype(np.int32)
    if on_target is not None:
        which = np.where(np.asarray(on_target, bool), which, np.int32(OFF_TARGET)).astype(np.int32)
    n = len(which)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    heads = np.flatnonzero(np.concatenate([[True], which[1:] != which[:-1]]))
    starts = heads.astype(np.int64) + int(first_position)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64) + int(first_position)
    return starts, ends, which[heads]


def totals_numpy(depths, bins, on_target=None):
    """-> (bases per bin int64 [8], sum of depths): what pa_encoder_depth_totals reports for a region with these depths."""
    depths = np.asarray(depths, np.int64)
    keep = np.ones(len(depths), bool) if on_target is None else np.asarray(on_target, bool)
    which = np.searchsorted(np.asarray(bins, np.int64), depths[keep], side="right") - 1
    return np.bincount(which, minlength=MAX_BINS).astype(np.int64)[:MAX_BINS], int(depths[keep].sum())


class CoverageTrack(object):
    """The runs of a whole job, collected from its workers in any order (add) and finished once (finish / write).

    contigs: the FASTA's contig names in its order; bins, labels: what parse_bins returned."""

    def __init__(self, contigs, bins, labels):
        self.order = {name: k for k, name in enumerate(contigs)}
        self.bins = np.asarray(bins, np.int32)
        self.labels = list(labels)
        if len(self.labels) != len(self.bins):
            raise ValueError("coverage track: one label per bin")
        self._lock = threading.Lock()
        self._pieces = []
        self.depth_sum = 0
        self.depth_bases = 0

    def add(self, contig, interval, runs, totals=None):
        """One interval of the planner: interval = (pos_start, pos_end), both inclusive; runs = (starts, ends, bins) of its
        window in contig coordinates, ascending; totals = (bases per bin, sum of depths) or None."""
        if contig not in self.order:
            raise ValueError("coverage track: contig %r is not in the FASTA" % (contig,))
        starts, ends, which = (np.array(v, dtype) for v, dtype in zip(runs, (np.int64, np.int64, np.int32)))
        if not (len(starts) == len(ends) == len(which)):
            raise ValueError("coverage track: runs of unequal lengths")
        with self._lock:
            self._pieces.append((self.order[contig], int(interval[0]), int(interval[1]), contig, starts, ends, which))
            if totals is not None:
                self.depth_bases += int(np.asarray(totals[0], np.int64).sum())
                self.depth_sum += int(totals[1])

    def finish(self):
        """-> [(contig, start, end, bin)] in FASTA order: the pieces ordered by contig and start; the position two consecutive
        intervals of split_intervals share (pos_end of one == pos_start of the next) belongs to the one that starts there -- the
        earlier interval's runs are cut at the next interval's start and dropped when nothing is left; off-target runs dropped;
        touching runs of equal bin merged."""
        with self._lock:
            pieces = sorted(self._pieces, key=lambda p: p[:3])
        out = []
        for k, (_rank, _s, _e, contig, starts, ends, which) in enumerate(pieces):
            if k + 1 < len(pieces) and pieces[k + 1][0] == pieces[k][0]:
                ends = np.minimum(ends, pieces[k + 1][1])          # the next interval of the contig owns everything from its start
            for s, e, b in zip(starts.tolist(), ends.tolist(), which.tolist()):
                if s >= e or b == OFF_TARGET:
                    continue
                if out and out[-1][0] == contig and out[-1][2] == s and out[-1][3] == b:
                    out[-1] = (contig, out[-1][1], e, b)
                else:
                    out.append((contig, s, e, b))
        return out

    def write(self, path):
        """The BED -> the finished runs."""
        runs = self.finish()
        with open(path, "w") as fh:
            for contig, s, e, b in runs:
                fh.write("%s\t%d\t%d\t%s\n" % (contig, s, e, self.labels[b]))
        return runs

    def summary(self, runs=None):
        """-> (bases per label in bin order, mean depth).  The bases are those of the finished track; the mean is taken over
        the positions as the intervals reported them, where a position two intervals share counts for both."""
        runs = self.finish() if runs is None else runs
        bases = [0] * len(self.labels)
        for _contig, s, e, b in runs:
            bases[b] += e - s
        return bases, (self.depth_sum / self.depth_bases if self.depth_bases else 0.0)

    def log_line(self, runs=None):
        bases, mean = self.summary(runs)
        total = sum(bases)
        parts = ["%s %d (%.4f)" % (label, n, n / total if total else 0.0) for label, n in zip(self.labels, bases)]
        return "COVERAGE BED: " + str(total) + " BASES: " + ", ".join(parts) + "; MEAN DEPTH %.2f" % mean
