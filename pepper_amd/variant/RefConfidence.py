"""Reference confidence of the positions a run looked at (options.gvcf): the non-variant blocks of the gVCF.

A position without a record in the VCF may be one where the reads agree with the reference, or one where nothing could be
seen.  The encoder holds what tells them apart once per run: with a reference-confidence table set
(pa_encoder_set_ref_confidence) tile_count_kernel turns the counters of every position into a GQ byte and ref_blocks_kernel
(pepper_amd/csrc/encoder.hip) run-length encodes the GQ bands of every candidate window, with the smallest depth and the
smallest GQ of each run.  This module states the rule once, in numpy, builds the table the device looks up, and collects the
workers' blocks (BlockTrack); pepper_amd/variant/Gvcf.py writes the file.

Evidence of a position, from the tile kernel's counters before the int8 clamp (F[s] / R[s]: forward / reverse slot of symbol s):
    cov      the coverage, the number the depth track reports (pepper_amd/variant/Coverage.py)
    ref_col  F + R of the reference letter, 0 where the reference base is not one of ACGT
    ins      F + R of the insert anchor,  star  F + R of `*`
    n_ref = max(0, ref_col - ins),  n_alt = max(0, cov - ref_col) + min(ins, ref_col) + star
Reads that show the reference letter and open no insert behind it speak for the reference; other letters, insert anchors and
deleted bases (which are not part of cov) against it.  With n = n_ref + n_alt > 100 both are rescaled as DeepVariant does,
n_ref' = (100 n_ref + n - 1) // n, n_alt' = 100 - n_ref'.

GQ is DeepVariant's published reference-confidence model with its defaults: the log10 likelihoods of hom-ref, het and hom-alt
under a per-read error rate p, normalised, GQ = floor(min(max_gq, -10 log10(1 - P(hom-ref)))).  It is a model of read counts
and not the network's output, and nobody has calibrated p for nanopore reads here: it is a parameter (options.gvcf_error_rate).

With options.haploid_contigs (pepper_amd/variant/Ploidy.py) the blocks of a haploid stretch keep this DIPLOID GQ: there is no
haploid table.  Dropping the het hypothesis removes a term from the normaliser and leaves the hom-ref term as it is, so it can
only raise P(hom-ref): the diploid GQ is a lower bound of the haploid one.  Gvcf.py writes such a block with GT 0.
"""
import math

import numpy as np

from pepper_amd.variant import RunTracks
from pepper_amd.variant.RunTracks import OFF_TARGET        # the band of a position outside every target: never written

MAX_BANDS = RunTracks.MAX_CLASSES
TABLE_SIDE = 101                     # counts 0 .. 100 after the rescale
RESCALE_TO = 100
DEFAULT_ERROR_RATE = 0.001
DEFAULT_MAX_GQ = 50
DEFAULT_BANDS = (0, 1, 10, 20, 30, 40, 50)


def _log10_sum(*terms):
    top = max(terms)
    return top + math.log10(sum(10.0 ** (t - top) for t in terms))


def gq_value(n_ref, n_alt, p=DEFAULT_ERROR_RATE, max_gq=DEFAULT_MAX_GQ):
    """The GQ of n_ref reads for the reference and n_alt against it (after the rescale), in f64.  (0, 0) -> 0."""
    if n_ref == 0 and n_alt == 0:
        return 0
    hom_ref = n_ref * math.log10(1.0 - p) + n_alt * math.log10(p)
    het = -(n_ref + n_alt) * math.log10(2.0)
    hom_alt = n_ref * math.log10(p) + n_alt * math.log10(1.0 - p)
    # log10(1 - P(hom-ref)) as the log-sum of the other two terms over the log-sum of all three: no subtraction from 1
    log_not_ref = _log10_sum(het, hom_alt) - _log10_sum(hom_ref, het, hom_alt)
    return int(math.floor(min(float(max_gq), -10.0 * log_not_ref)))


def build_table(p=DEFAULT_ERROR_RATE, max_gq=DEFAULT_MAX_GQ):
    """-> uint8 [101, 101], row n_ref, column n_alt: what the device looks up.  ValueError: p outside (0, 0.5), max_gq outside
    [0, 255]."""
    p = float(p)
    if not (0.0 < p < 0.5):
        raise ValueError("reference confidence: error rate %r is not inside (0, 0.5)" % (p,))
    if not (0 <= int(max_gq) <= 255) or int(max_gq) != max_gq:
        raise ValueError("reference confidence: max_gq %r is not an integer in [0, 255]" % (max_gq,))
    table = np.zeros((TABLE_SIDE, TABLE_SIDE), np.uint8)
    for r in range(TABLE_SIDE):
        for a in range(TABLE_SIDE):
            table[r, a] = max(0, gq_value(r, a, p, int(max_gq)))
    return table


def parse_bands(bands=None):
    """-> int32 lower bounds of GQ.  bands: None (DEFAULT_BANDS), a sequence of integers or their text "0,1,10,20".  ValueError,
    naming the entry: more than 8 bands, none at all, a first bound that is not 0, a bound that is not above the one before it,
    not an integer or above 255."""
    if bands is None or (isinstance(bands, str) and bands.strip() == ""):
        return np.array(DEFAULT_BANDS, np.int32)
    return RunTracks.parse_bounds(bands, "gvcf bands", "band",
                                  lambda v: "is above 255, the largest GQ a table holds" if v > 255 else None)


def band_labels(bands):
    bounds = [int(b) for b in bands]
    return ["GQ %d-%d" % (lo, hi - 1) for lo, hi in zip(bounds, bounds[1:])] + ["GQ %d+" % bounds[-1]]


def evidence(cov, ref_col, ins, star):
    """-> (n_ref, n_alt), int64, before the rescale."""
    cov, ref_col, ins, star = (np.asarray(v, np.int64) for v in (cov, ref_col, ins, star))
    n_ref = np.maximum(0, ref_col - ins)
    n_alt = np.maximum(0, cov - ref_col) + np.minimum(ins, ref_col) + star
    return n_ref, n_alt


def rescale(n_ref, n_alt):
    """Counts whose sum is above 100 brought to a sum of 100, in 64-bit integers, rounding n_ref up."""
    n_ref, n_alt = np.asarray(n_ref, np.int64), np.asarray(n_alt, np.int64)
    n = n_ref + n_alt
    big = n > RESCALE_TO
    safe = np.where(big, n, 1)
    scaled = (RESCALE_TO * n_ref + safe - 1) // safe
    return np.where(big, scaled, n_ref), np.where(big, RESCALE_TO - scaled, n_alt)


def gq_numpy(cov, ref_col, ins, star, ref_is_acgt, table):
    """The GQ byte of every position: the evidence, rescaled, looked up; 0 where the reference base is not one of ACGT."""
    n_ref, n_alt = rescale(*evidence(cov, ref_col, ins, star))
    gq = np.asarray(table, np.uint8)[n_ref, n_alt].astype(np.int32)
    return np.where(np.asarray(ref_is_acgt, bool), gq, 0).astype(np.int32)


def blocks_numpy(cov, gq, first_position, bands, on_target=None):
    """The rule of ref_blocks_kernel without its tile borders: cov[i], gq[i] speak of position first_position + i ->
    (starts, ends, band, min_dp, min_gq) of the maximal runs of equal band, ends half-open, each with the smallest cov and the
    smallest gq of its positions.  on_target (bool per position; None: all): a position outside has the band OFF_TARGET."""
    return RunTracks.class_runs(gq, first_position, bands, on_target, minimise=(cov, gq))


def merge_blocks(region, starts, ends, band, min_dp, min_gq):
    """Touching records of one region and equal band joined, with the smaller of their minima: what the device reports one
    record per tile for.  Records in region and position order -> the same six arrays, shorter."""
    types = (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32)
    cols = RunTracks.merge_touching(*(np.asarray(v, t) for v, t in zip((region, starts, ends, band, min_dp, min_gq), types)))
    return tuple(np.asarray(c, t) for c, t in zip(cols, types))


class BlockTrack(RunTracks.RunTrack):
    """The blocks of a whole job, collected from its workers in any order (add: blocks = (starts, ends, band, min_dp, min_gq))
    and finished once (finish_arrays; finish -> [(contig, start, end, band, min_dp, min_gq)]).

    contigs: the FASTA's contig names in its order; bands: what parse_bands returned; table: what build_table returned."""
    what, noun, columns = "block track", "blocks", (np.int32, np.int32, np.int32)

    def __init__(self, contigs, bands, table):
        super().__init__(contigs)
        self.bands = np.asarray(bands, np.int32)
        self.table = np.ascontiguousarray(table, np.uint8)

    def add_empty(self, contig, interval, on_target=None):
        """An interval no encoder call covered because no read lies in it: depth 0 and GQ 0 at every position."""
        zeros = np.zeros(int(interval[1]) - int(interval[0]) + 1, np.int64)
        self.add(contig, interval, blocks_numpy(zeros, zeros, int(interval[0]), self.bands, on_target))

    def log_line(self, arrays=None):
        _rank, starts, ends, band, _dp, _gq = self.finish_arrays() if arrays is None else arrays
        bases = np.bincount(band, weights=(ends - starts).astype(np.float64), minlength=len(self.bands)).astype(np.int64).tolist()
        total = sum(bases)
        parts = ["%s %d (%.4f)" % (label, n, n / total if total else 0.0) for label, n in zip(band_labels(self.bands), bases)]
        return "GVCF: " + str(total) + " BASES IN " + str(len(band)) + " BLOCKS BEFORE THE RECORDS ARE CUT OUT: " + ", ".join(parts)
