"""Prediction HDF5 directory -> polished FASTA.

replaces: /root/reference/pepper/modules/python/perform_stitch.py:44-84 (`perform_stitch`): every
`*hdf` of the directory, contigs in natural order, one `>contig` record per non-empty consensus,
written to `<output_path>_pepper_polished.fa`.  (The reference's 5 s sleep is not reproduced.)
qualities=True (opt-in, not in the reference) also writes `<output_path>_pepper_polished.fastq`: the same records with the
phred of the prediction row that supplied each base, as Sanger text.
edits=<draft FASTA> (opt-in, not in the reference) also writes `<output_path>_pepper_polished.edits.tsv`: what the consensus
changed against the draft, hunk by hunk in both coordinate systems (pepper_amd/polish/Edits.py).
fill=<draft FASTA> (opt-in, not in the reference): every contig is merged as one piece and the draft's own letters stand where no
prediction covered a position, so the consensus is complete and does not depend on `threads`; unpolished_contigs=True also
writes the contigs of the draft that have no prediction, unchanged, in natural order among the rest.
min_quality=Q with draft=<draft FASTA> (opt-in, not in the reference): only the edits whose winning prediction has phred >= Q are
applied, the draft's letter stands elsewhere (pepper_amd/polish/Stitch.py gate_numpy); also writes
`<output_path>_pepper_polished.withheld.tsv`, the edits kept back.
vcf=<draft FASTA> with fill (opt-in, not in the reference) also writes `<output_path>_pepper_polished.vcf.gz` and its `.tbi`: the
hunks of the filled consensus trimmed and left-aligned against the draft (pepper_amd/polish/Variants.py).
"""
import contextlib
import re
import sys
from datetime import datetime
from os import listdir
from os.path import isfile, join
from pathlib import Path

from pepper_amd import h5
from pepper_amd.polish.Stitch import create_consensus_sequence, whole_draft


def natural_key(string_):
    return [int(s) if s.isdigit() else s for s in re.split(r'(\d+)', string_)]


def get_file_paths_from_directory(directory_path):
    return [join(directory_path, file) for file in sorted(listdir(directory_path))
            if isfile(join(directory_path, file)) and file[-3:] == 'hdf']


def _log(message):
    sys.stderr.write("[" + str(datetime.now().strftime('%m-%d-%Y %H:%M:%S')) + "] INFO: " + message + "\n")


def fastq_path(output_prefix):
    return output_prefix + '_pepper_polished.fastq'


def write_fastq_record(fastq, contig, sequence, quality):
    # (four writes: the record of a whole contig is not put together in memory first)
    fastq.write('@' + contig + "\n")
    fastq.write(sequence)
    fastq.write("\n+\n")
    fastq.write(quality + "\n")


def draft_lengths(draft_fasta):
    """{contig: length} of the draft FASTA the edits are taken against."""
    from pepper_amd.variant.fasta import FASTA_handler
    handler = FASTA_handler(draft_fasta)
    try:
        return {name: handler.get_chromosome_sequence_length(name) for name in handler.get_chromosome_names()}
    finally:
        handler.close()


def check_fill(edits, fill, unpolished_contigs):
    """What every stitch form asks of its fill arguments."""
    if unpolished_contigs and fill is None:
        raise ValueError("unpolished_contigs needs fill: the draft FASTA the contigs are taken from")
    if fill is not None and edits is not None and str(edits) != str(fill):
        raise ValueError("with fill the edits are taken against the draft that fills: %s is not %s" % (edits, fill))


def check_gate(min_quality, draft, edits, fill):
    """What every stitch form asks of its gate arguments -> min_quality as an integer 1..255, or None (off)."""
    from pepper_amd import _lib
    min_quality = _lib.min_quality_value(min_quality)
    if min_quality is None:
        return None
    if draft is None:
        raise ValueError("min_quality needs draft: the draft FASTA the edits are measured against")
    for other, what in ((edits, "the edits are taken against"), (fill, "fills")):
        if other is not None and str(other) != str(draft):
            raise ValueError("with min_quality the draft is the one that %s: %s is not %s" % (what, other, draft))
    return min_quality


class GateLog(object):
    """The withheld.tsv of a gated run and its one INFO line: the applied and the withheld edits by kind, over every contig."""

    def __init__(self, files, output_prefix):
        from pepper_amd.polish import Edits
        self.file = files.enter_context(open(Edits.withheld_path(output_prefix), 'w'))
        self.file.write(Edits.WITHHELD_HEADER)
        self.applied, self.withheld = [0, 0, 0], [0, 0, 0]

    def contig(self, contig, withheld, applied_counts):
        from pepper_amd.polish import Edits
        Edits.write_withheld(self.file, contig, withheld)
        self.applied = [a + b for a, b in zip(self.applied, applied_counts)]
        self.withheld = [a + b for a, b in zip(self.withheld, Edits.kind_counts(withheld))]

    def log(self, min_quality):
        _log("MIN QUALITY %d: APPLIED sub=%d del=%d ins=%d, WITHHELD sub=%d del=%d ins=%d." %
             ((min_quality,) + tuple(self.applied) + tuple(self.withheld)))


def write_unpolished(contig, fill, draft_length, fasta, fastq, edits_file, gated=False):
    """A contig of the draft without a prediction, as the filled consensus of nothing: its letters as stored, qualities '!',
    one `filled` hunk (gated: the run has a min_quality gate; the summary line says withheld=0)."""
    sequence, quality = whole_draft(fill, contig)
    _log("NO PREDICTION FOR " + contig + ", DRAFT SEQUENCE LENGTH: " + str(len(sequence)) + ".")
    if edits_file is not None:
        from pepper_amd.polish import Edits
        Edits.write_contig(edits_file, contig, [], [], draft_length, True, filled=True, withheld=0 if gated else None)
    if len(sequence) > 0:
        fasta.write('>' + contig + "\n")
        fasta.write(sequence + "\n")
        if fastq is not None:
            write_fastq_record(fastq, contig, sequence, quality)


def perform_stitch(hdf_file_path, output_path, threads, qualities=False, edits=None, fill=None, unpolished_contigs=False,
                   min_quality=None, draft=None, vcf=None):
    from pepper_amd.polish import Variants
    check_fill(edits, fill, unpolished_contigs)
    Variants.check_vcf(vcf, fill)
    min_quality = check_gate(min_quality, draft, edits, fill)
    all_prediction_files = get_file_paths_from_directory(hdf_file_path)
    all_contigs = set()
    for prediction_file in all_prediction_files:
        with h5.File(prediction_file, 'r') as hdf5_file:
            if 'predictions' in hdf5_file.keys():
                all_contigs.update(hdf5_file.keys('predictions'))

    output_prefix = output_path
    output_path = output_path + '_pepper_polished.fa'
    Path(output_path).resolve().parents[0].mkdir(parents=True, exist_ok=True)
    with contextlib.ExitStack() as files:
        consensus_fasta_file = files.enter_context(open(output_path, 'w'))
        fastq = files.enter_context(open(fastq_path(output_prefix), 'w')) if qualities else None
        edits_file = None
        if edits is not None or min_quality:
            from pepper_amd.polish import Edits
        if edits is not None:
            edits_file = files.enter_context(open(Edits.edits_path(output_prefix), 'w'))
            edits_file.write(Edits.HEADER)
        gate = GateLog(files, output_prefix) if min_quality else None
        draft_path = draft if min_quality else fill if fill is not None else edits
        lengths = draft_lengths(draft_path) if draft_path is not None else {}
        vcf_file = Variants.VcfOutput(files, output_prefix, lengths) if vcf is not None else None
        for contig in sorted(all_contigs | set(lengths if unpolished_contigs else ()), key=natural_key):
            if contig not in all_contigs:
                write_unpolished(contig, fill, lengths[contig], consensus_fasta_file, fastq, edits_file, gated=gate is not None)
                continue
            _log("PROCESSING CONTIG: " + contig)
            all_chunk_keys = []
            for prediction_file in all_prediction_files:
                with h5.File(prediction_file, 'r') as hdf5_file:
                    if 'predictions' not in hdf5_file.keys() or contig not in hdf5_file.keys('predictions'):
                        continue
                    # every region group with its contig_start / contig_end in one library call (names in sorted order)
                    all_chunk_keys.extend((prediction_file, name, start, end) for name, start, end in hdf5_file.list_polish_regions(contig))
            if draft_path is not None and contig not in lengths:
                raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
            if gate is not None:              # (the records are always made: their kinds are the applied edits the run logs)
                consensus_sequence, quality, records, pieces, withheld = create_consensus_sequence(
                    contig, all_chunk_keys, threads, qualities=qualities, edits=draft, fill=fill, min_quality=min_quality, draft=draft)
                gate.contig(contig, withheld, Edits.kind_counts(records))
                if edits is not None:
                    Edits.write_contig(edits_file, contig, records, pieces, lengths[contig], True, filled=fill is not None,
                                       withheld=len(withheld))
            elif edits is not None or vcf is not None:  # (the VCF is made of the filled consensus' edit records)
                consensus_sequence, quality, records, pieces = create_consensus_sequence(
                    contig, all_chunk_keys, threads, qualities=qualities, edits=edits if edits is not None else vcf, fill=fill)
                if edits is not None:
                    Edits.write_contig(edits_file, contig, records, pieces, lengths[contig], True, filled=fill is not None)
            elif qualities:
                consensus_sequence, quality = create_consensus_sequence(contig, all_chunk_keys, threads, qualities=True, fill=fill)
            else:
                consensus_sequence = create_consensus_sequence(contig, all_chunk_keys, threads, fill=fill)
            if vcf_file is not None:
                stored = whole_draft(fill, contig)[0]
                vcf_file.contig(contig, *Variants.records_numpy(records, stored, consensus_sequence, True), stored, consensus_sequence,
                                True)
            _log("FINISHED PROCESSING " + contig + ", POLISHED SEQUENCE LENGTH: " + str(len(consensus_sequence)) + ".")
            if consensus_sequence is not None and len(consensus_sequence) > 0:
                consensus_fasta_file.write('>' + contig + "\n")
                consensus_fasta_file.write(consensus_sequence + "\n")
                if qualities:
                    write_fastq_record(fastq, contig, consensus_sequence, quality)
        if gate is not None:
            gate.log(min_quality)
    return output_path
