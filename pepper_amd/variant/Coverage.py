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

import numpy as np

from pepper_amd.variant import RunTracks
from pepper_amd.variant.RunTracks import OFF_TARGET        # the bin of a position outside every target: never written

MAX_BINS = RunTracks.MAX_CLASSES
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
    bounds = RunTracks.parse_bounds(bins, "coverage bins", "bin", lambda v: "does not fit 31 bits" if v >= 1 << 31 else None).tolist()
    labels = ["%d:%d" % (lo, hi) for lo, hi in zip(bounds, bounds[1:])] + ["%d:inf" % bounds[-1]]
    return np.array(bounds, np.int32), labels


def runs_numpy(depths, first_position, bins, on_target=None):
    """The rule of depth_runs_kernel: depths[i] is the depth of position first_position + i -> (starts, ends, bins) of the
    maximal runs of equal bin, int64 / int64 / int32, ends half-open.  on_target (bool per position; None: all): a position
    outside has the bin OFF_TARGET, and its runs are reported like any other."""
    return RunTracks.class_runs(depths, first_position, bins, on_target)


def totals_numpy(depths, bins, on_target=None):
    """-> (bases per bin int64 [8], sum of depths): what pa_encoder_depth_totals reports for a region with these depths."""
    depths = np.asarray(depths, np.int64)
    keep = np.ones(len(depths), bool) if on_target is None else np.asarray(on_target, bool)
    which = RunTracks.classes_of(depths[keep], bins)
    return np.bincount(which, minlength=MAX_BINS).astype(np.int64)[:MAX_BINS], int(depths[keep].sum())


class CoverageTrack(RunTracks.RunTrack):
    """The runs of a whole job, collected from its workers in any order (add) and finished once (finish / write): finish ->
    [(contig, start, end, bin)] in FASTA order.

    contigs: the FASTA's contig names in its order; bins, labels: what parse_bins returned."""
    what = "coverage track"

    def __init__(self, contigs, bins, labels):
        super().__init__(contigs)
        self.bins = np.asarray(bins, np.int32)
        self.labels = list(labels)
        if len(self.labels) != len(self.bins):
            raise ValueError("coverage track: one label per bin")
        self.depth_sum = 0
        self.depth_bases = 0

    def add(self, contig, interval, runs, totals=None):
        """One interval of the planner: interval = (pos_start, pos_end), both inclusive; runs = (starts, ends, bins) of its
        window in contig coordinates, ascending; totals = (bases per bin, sum of depths) or None."""
        super().add(contig, interval, runs)
        if totals is not None:
            with self._lock:
                self.depth_bases += int(np.asarray(totals[0], np.int64).sum())
                self.depth_sum += int(totals[1])

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
