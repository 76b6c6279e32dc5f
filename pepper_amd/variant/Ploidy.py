"""Ploidy of what a run calls (options.haploid_contigs, options.par_regions_bed): which positions are genotyped as haploid.

The model has three classes (HOM-REF, HET-ALT, HOM-ALT) and the candidate finder turns them into 0/0, 0/1 and 1/1.  On a
haploid contig -- a bacterial or viral genome, chrM, chrX / chrY of a male sample outside the pseudo-autosomal regions -- a
0/1 is a contradiction.  Position p of contig c is haploid iff c is listed in haploid_contigs and no interval of the PAR BED
holds start <= p < end (0-based, half-open, as Targets.read_bed reads a BED); `is_haploid` is that rule in numpy, the twin of
Targets.contains.

At a haploid position the model's float32 triple (p0, p1, p2) is PRIMED before anything reads it: the mass on HET is dropped
and the rest renormalised,

    s   = (double)p0 + (double)p2
    p0' = (float)((double)p0 / s),  p1' = 0.0f,  p2' = (float)((double)p2 / s)     if s != 0
    p0' = 0.5f,                     p1' = 0.0f,  p2' = 0.5f                         if s == 0

and the genotype (first maximum: 0 or 2, never 1), non_alt = max(p1', p2'), the deletion swap, GQ / QUAL, the AP field and the
QUAL cutoff read the primed triple exactly where they read the model's.  `prime` states it in numpy float64; candidates.cpp
(pa_candidates_select_format_ploidy) and select.hip (k_select_decide) restate it, with the same IEEE double quotient.
A haploid record's GT is one number: 0 (refCall) or the 1-based index of the called ALT.
"""
import os
import sys

import numpy as np

from pepper_amd.variant import Targets

ENV_CONTIGS = "PEPPER_AMD_HAPLOID_CONTIGS"
ENV_PAR = "PEPPER_AMD_PAR_REGIONS_BED"

_NO_TABLE = (np.zeros(0, np.int64), np.zeros(0, np.int64))


class Ploidy(object):
    """given: haploid_contigs as the user wrote it; contigs: the haploid contig names; par: {contig: (starts, ends)} merged
    (Targets._merge), haploid contigs only; par_name: the basename of the PAR BED or None.  Plain attributes: it pickles."""

    def __init__(self, given, contigs, par=None, par_name=None):
        self.given = str(given)
        self.contigs = frozenset(contigs)
        self.par = {c: (np.ascontiguousarray(s, np.int64), np.ascontiguousarray(e, np.int64)) for c, (s, e) in (par or {}).items()
                    if c in self.contigs and len(s)}
        self.par_name = par_name

    def table(self, contig):
        """(haploid contig?, PAR starts int64 [k], PAR ends int64 [k]) as pa_selector_set_ploidy takes them."""
        if contig not in self.contigs:
            return False, _NO_TABLE[0], _NO_TABLE[1]
        starts, ends = self.par.get(contig, _NO_TABLE)
        return True, starts, ends

    def is_haploid(self, contig, positions):
        """bool per position: contig is listed and no PAR interval holds the position."""
        positions = np.asarray(positions, np.int64)
        haploid, starts, ends = self.table(contig)
        if not haploid:
            return np.zeros(positions.shape, bool)
        return ~Targets.contains(starts, ends, positions)

    def boundaries(self, contig):
        """The positions at which the ploidy of `contig` changes, ascending (the edges of its PAR intervals)."""
        haploid, starts, ends = self.table(contig)
        return sorted(set(starts.tolist()) | set(ends.tolist())) if haploid else []

    def header_line(self):
        return "##pepper_amd_haploid_contigs=" + self.given + (";par_regions_bed=" + self.par_name if self.par_name else "")


def parse(haploid_contigs, par_regions_bed, contig_lengths, log=None):
    """The two options and {contig: length} of the FASTA -> a Ploidy, or None when neither is given."""
    given = (haploid_contigs or "").strip() if isinstance(haploid_contigs, str) else haploid_contigs
    if not given:
        if par_regions_bed:
            raise ValueError("par_regions_bed (" + str(par_regions_bed) + ") needs haploid_contigs: a PAR is a diploid stretch of a "
                             "haploid contig")
        return None
    if not isinstance(given, str):
        given = ",".join(str(c) for c in given)
    if given == "*":
        contigs = list(contig_lengths)
    else:
        contigs = [c.strip() for c in given.split(",") if c.strip()]
        for c in contigs:
            if c not in contig_lengths:
                raise ValueError("haploid_contigs: the FASTA has no contig " + repr(c))
    par = {}
    if par_regions_bed:
        per_contig, ignored = Targets.parse_bed(par_regions_bed, {c: contig_lengths[c] for c in contigs})
        if ignored and log is not None:
            log("INFO: PAR REGIONS BED: " + str(ignored) + " INTERVALS ON CONTIGS THAT ARE NOT HAPLOID OR THAT THE FASTA DOES NOT HAVE "
                "ARE IGNORED")
        par = {c: Targets._merge(pairs) for c, pairs in per_contig.items()}
    return Ploidy(given, contigs, par, os.path.basename(str(par_regions_bed)) if par_regions_bed else None)


def _stderr(message):
    sys.stderr.write(message + "\n")


def of(options, fasta_handler=None, log=_stderr):
    """The run's Ploidy from its options (options.ploidy when something resolved it already -- _plain_options does, for the
    spawned workers --, else options.haploid_contigs / options.par_regions_bed or their environment variables), or None."""
    held = getattr(options, "ploidy", None)
    if isinstance(held, Ploidy):
        return held
    names = getattr(options, "haploid_contigs", None) or os.environ.get(ENV_CONTIGS) or None
    bed = getattr(options, "par_regions_bed", None) or os.environ.get(ENV_PAR) or None
    if not names:
        return parse(None, bed, {})
    key = (str(names), str(bed), str(getattr(options, "fasta", None)))
    cached = getattr(options, "_ploidy_cache", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    if fasta_handler is None:
        from pepper_amd.variant.CandidateFinder import _fasta
        fasta_handler = _fasta(options)
    lengths = {c: int(fasta_handler.get_chromosome_sequence_length(c)) for c in fasta_handler.get_chromosome_names()}
    ploidy = parse(names, bed, lengths, log=log)
    try:
        options._ploidy_cache = (key, ploidy)
    except AttributeError:
        pass
    return ploidy


def prime(triples):
    """float32 [n, 3] -> the primed float32 [n, 3] of the module's rule (every row taken as haploid)."""
    t = np.asarray(triples, np.float32).reshape(-1, 3)
    p0, p2 = t[:, 0].astype(np.float64), t[:, 2].astype(np.float64)
    s = p0 + p2
    zero = s == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.zeros(t.shape, np.float32)
        out[:, 0] = np.where(zero, 0.5, p0 / np.where(zero, 1.0, s)).astype(np.float32)
        out[:, 2] = np.where(zero, 0.5, p2 / np.where(zero, 1.0, s)).astype(np.float32)
    return out


def prime_batch(ploidy, contigs, positions, triples):
    """A prediction batch's float32 triples [n, 3] with the rows at haploid positions primed -> (triples float32 [n, 3],
    mask bool [n]).  contigs: one name for all rows, or a name per row.  ploidy None: the triples as given, no row set."""
    t = np.asarray(triples, np.float32)
    if ploidy is None:
        return t, np.zeros(len(t), bool)
    if t.ndim == 2 and t.shape[1] != 3:
        raise ValueError("haploid_contigs: a prediction of %d classes, expected 3" % t.shape[1])
    t = t.reshape(-1, 3)
    n = len(t)
    mask = np.zeros(n, bool)
    if n == 0:
        return t, mask
    positions = np.asarray(positions, np.int64).reshape(n)
    if isinstance(contigs, str):
        mask = ploidy.is_haploid(contigs, positions)
    else:
        names = np.asarray(list(contigs), dtype=object)
        for contig in dict.fromkeys(names.tolist()):
            if contig in ploidy.contigs:
                rows = np.flatnonzero(names == contig)
                mask[rows] = ploidy.is_haploid(contig, positions[rows])
    if mask.any():
        t = t.copy()
        t[mask] = prime(t[mask])
    return t, mask
