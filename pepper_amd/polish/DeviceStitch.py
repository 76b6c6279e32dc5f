"""The polish stitch on the device (opt-in: polish(..., device_stitch=True) / PEPPER_AMD_DEVICE_STITCH=1).

replaces, for a run that opts in: pepper/modules/python/Stitch.py of the reference
    small_chunk_stitch        :36-94    the {(position, insert index): label} merge -> pa_stitcher_* (pepper_amd/csrc/stitch.hip)
    create_consensus_sequence :97-128   region order and pieces -> plan() below, pure host code
perform_stitch (the host form) is untouched and stays the default; what this module writes is byte for byte its FASTA, and with
qualities on (opt-in, not in the reference) byte for byte its FASTQ: the phred of a row travels through the merge with its label.

plan() restates the loop order of the reference: regions sorted by name, then stably by (start, end), cut into pieces of
max(2, int(n / threads) + 1) consecutive regions; inside a region the chunk ids in STRING order.  The device only needs, per
row, its piece and a rank that grows along that loop: the last write of a key is the one with the largest rank.

fill (opt-in, not in the reference; perform_stitch(..., fill=) is the host form): the contig is planned as ONE piece whatever
`threads` is and pa_stitcher_fill completes the consensus on the device with the draft's letters where no row covered a position;
the draft goes up once per contig, the edits read that copy.

min_quality (opt-in, not in the reference; perform_stitch(..., min_quality=, draft=) is the host form): pa_stitcher_gate runs between
the finish and the fill, over the winners on the device -- the edits whose phred is below it are withheld, the draft's letter
stands -- and the withheld records come back for the .withheld.tsv; the draft the gate uploaded serves the fill and the edits.

vcf (opt-in, with fill, not in the reference; perform_stitch(..., fill=, vcf=) is the host form): pa_stitcher_variants groups the
edit records of the filled consensus into hunks, trims and left-aligns them against the draft on the device, and 32 bytes per
record come back; pepper_amd/polish/Variants.py states the rule and writes the .vcf.gz from them.
"""
import collections
import contextlib
import ctypes
import threading
import time
from pathlib import Path

import numpy as np

from pepper_amd import _lib, h5
from pepper_amd.polish import Edits, Variants
from pepper_amd.polish.Options import ImageSizeOptions
from pepper_amd.polish.Stitch import MIN_SEQUENCE_REQUIRED_FOR_MULTITHREADING
from pepper_amd.polish.perform_stitch import (GateLog, _log, check_fill, check_gate, draft_lengths, fastq_path,
                                              get_file_paths_from_directory, natural_key, write_fastq_record, write_unpolished)

Plan = collections.namedtuple("Plan", "order piece rank n_pieces chunk_order")


def string_order(chunk_ids):
    """The place of every chunk id in sorted(ids as strings): ("0", "1", "10", "11", "2", ...) -> [0, 1, 4, ...]."""
    ids = [str(c) for c in chunk_ids]
    place = [0] * len(ids)
    for k, i in enumerate(sorted(range(len(ids)), key=lambda i: ids[i])):
        place[i] = k
    return place


def string_order_key(chunk_id):
    """An integer that orders decimal chunk ids as their strings order (for a caller that does not know a region's other ids
    yet): the digits, each plus one, as an 18-digit number in base 11."""
    text = str(int(chunk_id))
    if int(chunk_id) < 0 or len(text) > 18:
        raise ValueError("chunk id %r has no string-order key" % (chunk_id,))
    key = 0
    for k in range(18):
        key = key * 11 + (int(text[k]) + 1 if k < len(text) else 0)
    return key


def plan(region_keys, threads, chunk_ids=None):
    """region_keys: [(file name, region name, start, end)] as perform_stitch collects them (files in listing order, a file's
    regions by name).  -> Plan: order = indices into region_keys in the order create_consensus_sequence iterates them; piece[i] /
    rank[i] = the piece small_chunk_stitch gets region i in and its place in `order`; n_pieces; chunk_order[i] = the place of every
    id of chunk_ids[i] in the string order small_chunk_stitch reads them in (None without chunk_ids)."""
    n = len(region_keys)
    order = sorted(range(n), key=lambda i: region_keys[i][1])
    order = sorted(order, key=lambda i: (int(region_keys[i][2]), int(region_keys[i][3])))
    size = max(MIN_SEQUENCE_REQUIRED_FOR_MULTITHREADING, int(n / max(1, threads)) + 1)
    piece, rank = [0] * n, [0] * n
    for k, i in enumerate(order):
        rank[i] = k
        piece[i] = k // size
    n_pieces = (n + size - 1) // size
    chunk_order = None if chunk_ids is None else [string_order(ids) for ids in chunk_ids]
    return Plan(order, piece, rank, n_pieces, chunk_order)


def _labels_u8(labels):
    """Host labels of any integer type as uint8; what does not fit is 255 (no base either: KeyError if it survives)."""
    labels = np.asarray(labels)
    if labels.dtype == np.uint8:
        return np.ascontiguousarray(labels)
    return np.ascontiguousarray(np.where((labels < 0) | (labels > 255), 255, labels).astype(np.uint8))


class DeviceStitcher(object):
    """One pa_stitcher handle: add() while a run goes on, finish() per contig at its end.  Regions are named by the keys plan()
    takes -- (file name, region name, start, end) -- and kept per contig in the order they first arrive."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        self.device = int(device)
        self._lock = threading.Lock()
        self._contigs = {}                   # contig -> (id, {region key: id}, [region keys])
        self._plain = set()                  # contigs that had an add without phred
        self.last_pieces = []                # of the last finish: [(first, last, length)] by piece number
        self.last_edit_counts = None         # of the last edits(): records per kind, [0..5]
        # over every edits() of this handle; the seconds: the comparison with its copy back, and the text made of it
        self.edit_totals = {"records": 0, "bytes_returned": 0, "seconds_compare": 0.0, "seconds_text": 0.0}
        self.last_fill_counts = None         # of the last finish(fill=): [runs filled, letters filled]
        self.last_filled = False             # the last finish was one with fill
        # over every finish(fill=) of this handle; the seconds: pa_stitcher_fill alone (the upload of the draft, the scan, the wait)
        self.fill_totals = {"runs": 0, "letters": 0, "seconds": 0.0}
        self.last_gate_counts = None         # of the last finish(min_quality=): withheld edits [in all, SUB, DEL, INS]
        self.last_gated = False              # the last finish was one with min_quality
        self._withheld = None                # its withheld records, once withheld() took them
        # over every finish(min_quality=) of this handle; the seconds: pa_stitcher_gate and the records' copy back
        self.gate_totals = {"withheld": 0, "sub": 0, "del": 0, "ins": 0, "bytes_returned": 0, "seconds": 0.0}
        self.last_variant_counts = None      # of the last variants(): [records, no-ops, unanchored, shifted, letters shifted]
        # over every variants() of this handle; the seconds: pa_stitcher_variants with its copy back, and the text made of it
        self.variant_totals = {"records": 0, "noops": 0, "unanchored": 0, "shifted": 0, "bytes_returned": 0, "seconds_device": 0.0,
                               "seconds_text": 0.0}
        handle = ctypes.c_void_p()
        _lib.check(self._lib.pa_stitcher_create(self.device, ctypes.c_void_p(stream) if stream else None, ctypes.byref(handle)))
        self._handle = handle

    @staticmethod
    def limits():
        """{'max_position', 'max_index', 'scan_block' (elements per workgroup of the scans), 'slab_rows'}"""
        out = (ctypes.c_int64 * 4)()
        _lib.check(_lib.load().pa_stitcher_limits(out, 4))
        return dict(zip(("max_position", "max_index", "scan_block", "slab_rows"), (int(v) for v in out)))

    @property
    def handle(self):
        if self._handle is None:
            raise _lib.PepperAmdError("the stitcher is closed")
        return self._handle

    def contigs(self):
        return list(self._contigs)

    def regions(self, contig):
        return list(self._contigs[contig][2]) if contig in self._contigs else []

    def add(self, contig, region_keys, chunk_order, position, index, labels, phred=None):
        """Chunks of one contig: region_keys[k] = (file name, region name, start, end) of chunk k, chunk_order[k] = what orders it
        among its region's chunks (string_order / string_order_key), position / index [n, length] integers, labels [n, length]:
        a numpy array, or a uint8 torch tensor on this stitcher's device whose values are complete (the caller has waited for
        the stream that wrote them).  phred [n, length]: the rows' qualities, where and what labels is (a numpy array beside a
        numpy array, a uint8 device tensor beside a device tensor); a contig has qualities when every add of it had them."""
        n = len(region_keys)
        if n == 0:
            return
        position = np.ascontiguousarray(position, dtype=np.int64).reshape(n, -1)
        index = np.ascontiguousarray(index, dtype=np.int64).reshape(n, -1)
        length = position.shape[1]
        if index.shape != position.shape:
            raise ValueError("position and index differ in shape")
        on_device = hasattr(labels, "is_cuda") and labels.is_cuda and labels.device.index == self.device
        phred_ptr = None
        if phred is not None and (hasattr(phred, "is_cuda") and phred.is_cuda and phred.device.index == self.device) != on_device:
            raise ValueError("labels and phred must both be device tensors of this stitcher's device or both host arrays")
        if on_device:
            import torch
            if labels.dtype != torch.uint8 or labels.numel() != n * length:
                raise ValueError("device labels must be uint8 [n, length]")
            labels = labels.contiguous()
            labels_ptr = labels.data_ptr()
            if phred is not None:
                if phred.dtype != torch.uint8 or phred.numel() != n * length:
                    raise ValueError("device phred must be uint8 [n, length]")
                phred = phred.contiguous()
                phred_ptr = phred.data_ptr()
        else:
            if hasattr(labels, "detach"):
                labels = labels.detach().cpu().numpy()
            labels = _labels_u8(labels).reshape(n, -1)
            if labels.shape != position.shape:
                raise ValueError("labels and position differ in shape")
            labels_ptr = labels.ctypes.data
            if phred is not None:
                if hasattr(phred, "detach"):
                    phred = phred.detach().cpu().numpy()
                phred = np.ascontiguousarray(np.asarray(phred).astype(np.uint8, copy=False)).reshape(n, -1)
                if phred.shape != position.shape:
                    raise ValueError("phred and position differ in shape")
                phred_ptr = phred.ctypes.data
        buffer_positions = ImageSizeOptions.MIN_IMAGE_OVERLAP * 2
        with self._lock:
            entry = self._contigs.get(contig)
            if entry is None:
                entry = (len(self._contigs), {}, [])
            ids, new_keys = entry[1], []
            for k in region_keys:
                if k not in ids:
                    ids[k] = len(ids)
                    new_keys.append(k)
            try:
                region = np.array([ids[k] for k in region_keys], dtype=np.int32)
                drop = np.array([int(k[2]) + buffer_positions if int(k[2]) > 0 else -1 for k in region_keys], dtype=np.int64)
                order = np.ascontiguousarray(chunk_order, dtype=np.int64)
                if order.shape != (n,):
                    raise ValueError("chunk_order must have one value per chunk")
                if phred_ptr is None:
                    _lib.check(self._lib.pa_stitcher_add(self.handle, entry[0], n, length, position.ctypes.data, index.ctypes.data,
                                                         labels_ptr, 1 if on_device else 0, region.ctypes.data, order.ctypes.data,
                                                         drop.ctypes.data))
                else:
                    _lib.check(self._lib.pa_stitcher_add_qual(self.handle, entry[0], n, length, position.ctypes.data,
                                                              index.ctypes.data, labels_ptr, phred_ptr, 1 if on_device else 0,
                                                              region.ctypes.data, order.ctypes.data, drop.ctypes.data))
            except BaseException:
                for k in new_keys:           # a refused call has added nothing: its new regions are not recorded either
                    del ids[k]
                raise
            entry[2].extend(new_keys)
            self._contigs[contig] = entry
            if phred_ptr is None:
                self._plain.add(contig)

    def finish(self, contig, threads, region_keys=None, qualities=False, fill=None, min_quality=None, draft=None):
        """The consensus of one contig as create_consensus_sequence(contig, region_keys, threads) returns it; region_keys
        default to the contig's regions in the order they first arrived.  KeyError(label): a surviving label that is no base.
        qualities: (sequence, quality) as create_consensus_sequence(..., qualities=True) returns them; PepperAmdError where an
        add of the contig came without phred.
        fill (str or bytes, the whole contig of the draft as its file stores it): the FILLED consensus, as
        create_consensus_sequence(..., fill=) returns it -- one piece whatever `threads` is, the draft's letters where no row
        covered a position, their qualities '!'; pieces() is then the one piece with the filled length, and edits() gives the
        filled consensus' records.
        min_quality (1..255; None or 0: off) with draft (str or bytes, the whole contig of the draft; default: `fill`): the GATED
        consensus, as create_consensus_sequence(..., min_quality=, draft=) returns it -- the edits against the draft whose winner
        has a phred below min_quality are withheld (pa_stitcher_gate, before the fill); withheld() gives their records,
        last_gate_counts their numbers, and edits() the applied edits.  Every add of the contig must have come with phred."""
        min_quality = _lib.min_quality_value(min_quality)
        if min_quality and draft is None:
            draft = fill
        if min_quality and draft is None:
            raise ValueError("min_quality needs the draft: the whole contig the edits are measured against")
        gate_draft = None if not min_quality else draft.encode() if isinstance(draft, str) else bytes(draft)
        draft = None if fill is None else fill.encode() if isinstance(fill, str) else bytes(fill)
        if gate_draft is not None and draft is not None and gate_draft != draft:
            raise ValueError("with min_quality the draft is the one that fills")
        with self._lock:
            self.last_filled = draft is not None
            self.last_gated = gate_draft is not None
            self._withheld = np.zeros(0, Edits.EDIT_DTYPE) if self.last_gated else None
            self.last_gate_counts = [0, 0, 0, 0] if self.last_gated else None
            entry = self._contigs.get(contig)
            if entry is None:
                self.last_pieces = []
                if draft is not None:            # no row of the contig: the draft as it is
                    self.last_fill_counts = [1 if draft else 0, len(draft)]
                    self.fill_totals["runs"] += self.last_fill_counts[0]
                    self.fill_totals["letters"] += len(draft)
                    return (draft.decode(), "!" * len(draft)) if qualities else draft.decode()
                return ("", "") if qualities else ""
            keys = list(region_keys) if region_keys is not None else list(entry[2])
            p = plan(keys, 1 if draft is not None else threads)
            known = [i for i, k in enumerate(keys) if k in entry[1]]
            region = np.array([entry[1][keys[i]] for i in known], dtype=np.int32)
            piece = np.array([p.piece[i] for i in known], dtype=np.int32)
            rank = np.array([p.rank[i] for i in known], dtype=np.int64)
            n_pieces = max(1, p.n_pieces)
            first, last, length = (np.empty(n_pieces, np.int64) for _ in range(3))
            total, bad = ctypes.c_int64(), ctypes.c_int32()
            _lib.check(self._lib.pa_stitcher_finish(self.handle, entry[0], len(known), region.ctypes.data, piece.ctypes.data,
                                                    rank.ctypes.data, n_pieces, first.ctypes.data, last.ctypes.data,
                                                    length.ctypes.data, ctypes.byref(total), ctypes.byref(bad)))
            if bad.value:
                raise KeyError(int(bad.value))
            if gate_draft is not None:
                t0 = time.perf_counter()
                counts = (ctypes.c_int64 * 4)()
                _lib.check(self._lib.pa_stitcher_gate(self.handle, gate_draft, len(gate_draft), min_quality, length.ctypes.data,
                                                      ctypes.byref(total), counts))
                self.last_gate_counts = [int(v) for v in counts]
                self._withheld = None                                # (on the device until withheld() asks)
                for name, v in zip(("withheld", "sub", "del", "ins"), self.last_gate_counts):
                    self.gate_totals[name] += v
                self.gate_totals["seconds"] += time.perf_counter() - t0
            self.last_pieces = list(zip(first.tolist(), last.tolist(), length.tolist()))
            if draft is not None:
                t0 = time.perf_counter()
                counts = (ctypes.c_int64 * 2)()
                # (after a gate the draft is on the device already)
                _lib.check(self._lib.pa_stitcher_fill(self.handle, None if gate_draft is not None else draft, len(draft),
                                                      ctypes.byref(total), counts))
                self.last_pieces = [(f, l, total.value) for f, l, _ in self.last_pieces if f != -1 and l != -1]
                self.last_fill_counts = [int(v) for v in counts]
                self.fill_totals["runs"] += self.last_fill_counts[0]
                self.fill_totals["letters"] += self.last_fill_counts[1]
                self.fill_totals["seconds"] += time.perf_counter() - t0
            buf = ctypes.create_string_buffer(max(1, total.value))
            _lib.check(self._lib.pa_stitcher_take(self.handle, buf, total.value))
            sequence = buf.raw[:total.value].decode()
            if not qualities:
                return sequence
            _lib.check(self._lib.pa_stitcher_take_qualities(self.handle, buf, total.value))
            return sequence, buf.raw[:total.value].decode()

    def withheld(self):
        """After finish(min_quality=): the edits the gate kept back, as Edits.EDIT_DTYPE records in the order and with the bytes
        of Stitch.gate_numpy (through create_consensus_sequence); after finish(fill=, min_quality=) their offsets count the
        filled consensus."""
        with self._lock:
            if not self.last_gated:
                raise _lib.PepperAmdError("the last finish had no min_quality")
            if self._withheld is None:                               # (the gate made them and said how many)
                self._withheld, _ = self._records(None, self.last_gate_counts[0], self._lib.pa_stitcher_take_withheld, Edits.EDIT_DTYPE,
                                                  self.gate_totals, "seconds")
            return self._withheld

    def _records(self, make, n_counts, take, dtype, totals, seconds):
        """Under the lock: make(n, counts), the call that makes the records and counts them (None: they are made, n_counts of
        them); a buffer of that many; `take`; totals["bytes_returned"] and totals[seconds] grow.  -> (records, counts or None)"""
        t0 = time.perf_counter()
        n, counts = ctypes.c_int64(n_counts), None
        if make is not None:
            counts = (ctypes.c_int64 * n_counts)()
            _lib.check(make(ctypes.byref(n), counts))
        records = np.zeros(n.value, dtype)
        _lib.check(take(self.handle, records.ctypes.data, n.value))
        totals["bytes_returned"] += records.nbytes
        totals[seconds] += time.perf_counter() - t0
        return records, None if counts is None else [int(v) for v in counts]

    def applied_counts(self, draft_length):
        """After finish(min_quality=): the applied edits [SUB, DEL, INS], counted on the device against the draft the gate left
        there; no record comes back."""
        with self._lock:
            if not self.last_pieces or all(p[0] == -1 for p in self.last_pieces):
                return [0, 0, 0]
            n, counts = ctypes.c_int64(), (ctypes.c_int64 * 6)()
            _lib.check(self._lib.pa_stitcher_edits(self.handle, None, draft_length, ctypes.byref(n), counts))
            return [int(v) for v in counts[1:4]]

    def has_qualities(self, contig):
        """Every add of the contig came with phred."""
        return contig not in self._plain

    def pieces(self):
        """The pieces of the last finish that hold rows, [(first, last, length)], in the order of the consensus."""
        return sorted((p for p in self.last_pieces if p[0] != -1 and p[1] != -1), key=lambda e: (e[0], e[1]))

    def edits(self, draft_sequence):
        """After finish(): what the consensus changed against draft_sequence (str or bytes, the whole contig of the draft), as
        Edits.EDIT_DTYPE records in the order and with the bytes of Edits.records_numpy -- compared on the device, only the
        records come back.  Pieces go with them as pieces().  After finish(fill=): the records of the filled consensus (the
        draft is the one that filled, and is not uploaded again)."""
        draft = draft_sequence.encode() if isinstance(draft_sequence, str) else bytes(draft_sequence)
        with self._lock:
            if self.last_filled and not self.last_pieces:            # the draft as it is: nothing was merged, no record
                self.last_edit_counts = [0] * 6
                return np.zeros(0, Edits.EDIT_DTYPE)
            held = self.last_filled or (self.last_gated and bool(self.last_pieces))      # a fill or a gate left its copy of the draft
            make = lambda n, counts: self._lib.pa_stitcher_edits(self.handle, None if held else draft, len(draft), n, counts)
            records, self.last_edit_counts = self._records(make, 6, self._lib.pa_stitcher_take_edits, Edits.EDIT_DTYPE, self.edit_totals,
                                                           "seconds_compare")
            self.edit_totals["records"] += len(records)
        return records

    def variants(self, draft_sequence):
        """After finish(fill=): the hunks of the filled consensus trimmed and left-aligned against draft_sequence (str or bytes,
        the whole contig of the draft -- the one that filled, which is not uploaded again), as Variants.VARIANT_DTYPE records
        with the bytes of Variants.records_numpy; normalised on the device (pa_stitcher_variants), only the records come back.
        last_variant_counts: [records, no-ops, unanchored, shifted, letters shifted]."""
        from pepper_amd.polish import Variants
        draft = draft_sequence.encode() if isinstance(draft_sequence, str) else bytes(draft_sequence)
        with self._lock:
            if not self.last_filled:
                raise _lib.PepperAmdError("the last finish had no fill: the variants describe the filled consensus")
            if not self.last_pieces:                                 # the draft as it is: nothing was merged, no record
                self.last_variant_counts = [0] * 5
                return np.zeros(0, Variants.VARIANT_DTYPE)
            make = lambda n, counts: self._lib.pa_stitcher_variants(self.handle, None, len(draft), n, counts)
            records, self.last_variant_counts = self._records(make, 5, self._lib.pa_stitcher_take_variants, Variants.VARIANT_DTYPE,
                                                              self.variant_totals, "seconds_device")
            for name, v in zip(("records", "noops", "unanchored", "shifted"), self.last_variant_counts):
                self.variant_totals[name] += v
        return records

    def _write_variants(self, vcf_file, contig, stored, sequence):
        """One contig's records of the .vcf.gz, after its filled finish (stored: the draft it was filled with)."""
        records = self.variants(stored)
        t0 = time.perf_counter()
        vcf_file.contig(contig, records, self.last_variant_counts, stored, sequence, self.has_qualities(contig))
        self.variant_totals["seconds_text"] += time.perf_counter() - t0

    def _write_edits(self, edits_file, draft, lengths, contig, stored=None, filled=None, withheld=None):
        """One contig's lines of the .edits.tsv, after its finish (stored: the draft the finish was filled or gated with; filled:
        it was filled, default: whenever stored is given; withheld: Edits.write_edits')."""
        if contig not in lengths:
            raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
        records = self.edits(stored if stored is not None else draft.get_reference_bytes(contig, 0, lengths[contig]))
        t0 = time.perf_counter()
        Edits.write_contig(edits_file, contig, records, self.pieces(), lengths[contig], self.has_qualities(contig),
                           filled=stored is not None if filled is None else filled, withheld=withheld)
        self.edit_totals["seconds_text"] += time.perf_counter() - t0

    def _finish_and_write(self, contig, threads, keys, qualities, fasta, fastq, edits_file, draft, lengths, edits, fill, min_quality,
                          gate, vcf_file=None):
        """One held contig of a writer: its finish (filled, gated) and its records in every file that is open."""
        stored = _stored_draft(draft, lengths, contig) if fill is not None or min_quality else None
        result = self.finish(contig, threads, keys, qualities=qualities, fill=stored if fill is not None else None,
                             min_quality=min_quality, draft=stored if min_quality else None)
        sequence, quality = result if qualities else (result, None)
        withheld = self.withheld() if min_quality else None
        if edits is not None:
            self._write_edits(edits_file, draft, lengths, contig, stored, filled=fill is not None,
                              withheld=None if withheld is None else len(withheld))
        if min_quality:
            gate.contig(contig, withheld, self.last_edit_counts[1:4] if edits is not None else self.applied_counts(lengths[contig]))
        if vcf_file is not None:              # (behind the edits: it reads their records where they are)
            self._write_variants(vcf_file, contig, stored, sequence)
        _log("FINISHED PROCESSING " + contig + ", POLISHED SEQUENCE LENGTH: " + str(len(sequence)) + ".")
        if len(sequence) > 0:
            fasta.write('>' + contig + "\n")
            fasta.write(sequence + "\n")
            if qualities:
                write_fastq_record(fastq, contig, sequence, quality)

    def stats(self):
        """{'rows', 'slab_bytes'} held, and of the last finish {'slots', 'pieces', 'positions', 'table_bytes'}"""
        out = (ctypes.c_int64 * 6)()
        _lib.check(self._lib.pa_stitcher_stats(self.handle, out, 6))
        return dict(zip(("rows", "slab_bytes", "slots", "pieces", "positions", "table_bytes"), (int(v) for v in out)))

    def write_fasta(self, output_prefix, threads, edits=None, fill=None, unpolished_contigs=False, min_quality=None, draft=None,
                    vcf=None):
        """Every contig held, in natural order, to <output_prefix>_pepper_polished.fa (perform_stitch's file).  edits: the
        draft FASTA's path; <output_prefix>_pepper_polished.edits.tsv beside it (perform_stitch(..., edits=)'s file).
        fill / unpolished_contigs: perform_stitch's -- the draft FASTA's path, every contig filled; and the draft's other
        contigs written among them.  min_quality / draft: perform_stitch's -- the gate and the draft FASTA's path; also writes
        <output_prefix>_pepper_polished.withheld.tsv.  vcf: perform_stitch's -- the draft FASTA's path (the one that fills); also
        writes <output_prefix>_pepper_polished.vcf.gz and .tbi, normalised on the device (variants())."""
        return self._write(output_prefix, threads, False, edits, fill, unpolished_contigs, min_quality, draft, vcf)

    def write_fastq(self, output_prefix, threads, edits=None, fill=None, unpolished_contigs=False, min_quality=None, draft=None,
                    vcf=None):
        """write_fasta's file, and beside it <output_prefix>_pepper_polished.fastq with the same records and their qualities
        (perform_stitch(..., qualities=True)'s two files), from one finish per contig.  -> the FASTQ's path."""
        return self._write(output_prefix, threads, True, edits, fill, unpolished_contigs, min_quality, draft, vcf)

    def _write(self, output_prefix, threads, qualities, edits, fill=None, unpolished_contigs=False, min_quality=None, gate_draft=None,
               vcf=None):
        check_fill(edits, fill, unpolished_contigs)
        Variants.check_vcf(vcf, fill)
        min_quality = check_gate(min_quality, gate_draft, edits, fill)
        output_path = output_prefix + '_pepper_polished.fa'
        Path(output_path).resolve().parents[0].mkdir(parents=True, exist_ok=True)
        with contextlib.ExitStack() as files:
            fasta = files.enter_context(open(output_path, 'w'))
            fastq = files.enter_context(open(fastq_path(output_prefix), 'w')) if qualities else None
            draft, lengths, edits_file = _open_draft(files, output_prefix, edits, fill, gate_draft if min_quality else None)
            gate = GateLog(files, output_prefix) if min_quality else None
            vcf_file = Variants.VcfOutput(files, output_prefix, lengths) if vcf is not None else None
            held = set(self.contigs())
            for contig in sorted(held | set(lengths if unpolished_contigs else ()), key=natural_key):
                if contig not in held:
                    write_unpolished(contig, fill, lengths[contig], fasta, fastq, edits_file, gated=gate is not None)
                    continue
                self._finish_and_write(contig, threads, None, qualities, fasta, fastq, edits_file, draft, lengths, edits, fill,
                                       min_quality, gate, vcf_file)
            if gate is not None:
                gate.log(min_quality)
        return fastq_path(output_prefix) if qualities else output_path

    def close(self):
        if self._handle is not None:
            self._lib.pa_stitcher_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *args):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _open_draft(files, output_prefix, edits, fill, gate_draft=None):
    """What a writer needs of the draft FASTA (the one that fills, else the one the edits are taken against, else the one the
    gate measures against): (handler, {contig: length}, the open .edits.tsv with its header or None); (None, {}, None) without
    any."""
    path = fill if fill is not None else edits if edits is not None else gate_draft
    if path is None:
        return None, {}, None
    from pepper_amd.variant.fasta import FASTA_handler
    lengths = draft_lengths(path)
    draft = FASTA_handler(path)
    files.callback(draft.close)
    edits_file = None
    if edits is not None:
        edits_file = files.enter_context(open(Edits.edits_path(output_prefix), 'w'))
        edits_file.write(Edits.HEADER)
    return draft, lengths, edits_file


def _stored_draft(draft, lengths, contig):
    """The whole contig of the draft as the file stores it."""
    if contig not in lengths:
        raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
    return draft.get_reference_bytes(contig, 0, lengths[contig], stored_case=True)


def _read_region(hdf5_file, prefix, qualities=False):
    """The chunks of one region group in string order of their ids -> [(position, index, labels)] blocks of [n, length] rows
    (one block of all chunks where they have the pipeline's length, else one block per chunk); qualities: (position, index,
    labels, phred) blocks -- the region read's sibling that takes phred_score beside bases, one dataset more per chunk."""
    names = ('position', 'index', 'bases', 'phred_score') if qualities else ('position', 'index', 'bases')
    try:
        block = hdf5_file.read_polish_prediction_region(prefix, ImageSizeOptions.SEQ_LENGTH, qualities=True) if qualities else \
            hdf5_file.read_polish_prediction_region(prefix, ImageSizeOptions.SEQ_LENGTH)
        return [tuple(block)] if len(block[0]) else []
    except h5.H5Error:                  # chunks of another length, or more of them than one call takes: one by one
        blocks = []
        for chunk in sorted(set(hdf5_file.keys(prefix)) - {'contig_start', 'contig_end'}):
            row = [np.asarray(hdf5_file[prefix + '/' + chunk + '/' + name], dtype=np.int64).reshape(1, -1)
                   for name in names]
            if row[0].size:
                blocks.append(tuple(row))
        return blocks


class _Held(object):
    """Chunks of one contig read from the files, handed to the stitcher a few thousand at a time (an add() is two launches and
    two waits whatever its size)."""
    CHUNKS = 8192

    def __init__(self, stitcher, contig):
        self.stitcher, self.contig = stitcher, contig
        self.keys, self.order, self.blocks = [], [], []

    def take(self, key, first_order, positions, indices, bases, phred=None):
        n = len(positions)
        if self.blocks and self.blocks[0][0].shape[1] != positions.shape[1]:
            self.flush()
        self.keys.extend([key] * n)
        self.order.extend(range(first_order, first_order + n))
        self.blocks.append((positions, indices, bases) if phred is None else (positions, indices, bases, phred))
        if len(self.keys) >= self.CHUNKS:
            self.flush()

    def flush(self):
        if self.keys:
            columns = [np.concatenate([b[k] for b in self.blocks]) for k in range(len(self.blocks[0]))]
            self.stitcher.add(self.contig, self.keys, self.order, *columns)
        self.keys, self.order, self.blocks = [], [], []


def stitch_directory(hdf_file_path, output_path, threads, device=0, stats=None, qualities=False, edits=None, fill=None,
                     unpolished_contigs=False, min_quality=None, draft=None, vcf=None):
    """perform_stitch(hdf_file_path, output_path, threads, qualities, edits, fill, unpolished_contigs) with the merge on the
    device: the same files read, the same FASTA (and FASTQ, and .edits.tsv) written.  stats: a dict that receives the handle's
    stats() after the last contig (with fill: and `fill`, the handle's fill_totals; with min_quality: and `gate`, its gate_totals).
    min_quality / draft: perform_stitch's gate, on the device; the same .withheld.tsv.  vcf: perform_stitch's, normalised on the
    device; the same .vcf.gz (stats then also receives `variants`, the handle's variant_totals)."""
    check_fill(edits, fill, unpolished_contigs)
    Variants.check_vcf(vcf, fill)
    min_quality = check_gate(min_quality, draft, edits, fill)
    gate_draft = draft
    # the edit records, the gate and the variants read the winners' phred
    read_phred = qualities or edits is not None or bool(min_quality) or vcf is not None
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
        stitcher = files.enter_context(DeviceStitcher(device))
        fasta = files.enter_context(open(output_path, 'w'))
        fastq = files.enter_context(open(fastq_path(output_prefix), 'w')) if qualities else None
        draft, lengths, edits_file = _open_draft(files, output_prefix, edits, fill, gate_draft if min_quality else None)
        gate = GateLog(files, output_prefix) if min_quality else None
        vcf_file = Variants.VcfOutput(files, output_prefix, lengths) if vcf is not None else None
        for contig in sorted(all_contigs | set(lengths if unpolished_contigs else ()), key=natural_key):
            if contig not in all_contigs:
                write_unpolished(contig, fill, lengths[contig], fasta, fastq, edits_file, gated=gate is not None)
                continue
            _log("PROCESSING CONTIG: " + contig)
            all_chunk_keys = []
            held = _Held(stitcher, contig)
            for prediction_file in all_prediction_files:
                with h5.File(prediction_file, 'r') as hdf5_file:
                    if 'predictions' not in hdf5_file.keys() or contig not in hdf5_file.keys('predictions'):
                        continue
                    regions = hdf5_file.list_polish_regions(contig)
                    all_chunk_keys.extend((prediction_file, name, start, end) for name, start, end in regions)
                    for name, start, end in regions:
                        key, at = (prediction_file, name, start, end), 0
                        # (the group is read by the name small_chunk_stitch rebuilds: contig-start-end)
                        for block in _read_region(hdf5_file, 'predictions/' + contig + '/' + contig + '-' + str(start) + '-' +
                                                  str(end), read_phred):
                            held.take(key, at, *block)
                            at += len(block[0])
            held.flush()
            stitcher._finish_and_write(contig, threads, all_chunk_keys, qualities, fasta, fastq, edits_file, draft, lengths, edits, fill,
                                       min_quality, gate, vcf_file)
        if gate is not None:
            gate.log(min_quality)
        if stats is not None:
            stats.update(stitcher.stats())
            if fill is not None:
                stats["fill"] = dict(stitcher.fill_totals)
            if min_quality:
                stats["gate"] = dict(stitcher.gate_totals)
            if vcf is not None:
                stats["variants"] = dict(stitcher.variant_totals)
    return output_path
