"""The candidate finder's selection on the device (pa_selector_*, include/pepper_amd_encoder.h; csrc/select.hip).

FastCandidates.native_batch_arrays decides on a host thread, for EVERY candidate row of a prediction batch, whether the row
becomes a VCF record (pa_candidates_reference_flags + pa_candidates_select_format) -- after the row's window, lists and
probabilities have crossed PCIe.  A DeviceSelector takes that decision where the encoder left the lists and the model the
probabilities and brings back only the kept rows, compacted in row order.  segment() hands those to the SAME
pa_candidates_select_format, which must keep every one of them, for the record text (%g, round(x, 3), int(-10 log10(..)) stay
with the host's printf and libm) -- no record text is formatted anywhere new.

A run the kernels hand back (status != 0: a zero depth, a NaN probability, a candidate string the library does not take, a
context in front of the reference given) has no result: the caller does that call the host way.
"""
import ctypes

import numpy as np

from pepper_amd import _lib, h5
from pepper_amd.variant import FastCandidates

def _is_tensor(x):
    return hasattr(x, "data_ptr")


class Taken(object):
    """The kept rows of one run (numpy, row order): row int32 [m] (numbers in the run's lists), flags uint8 [m] (bit 0 SNP, bit 2
    swapped, bit 3 haploid, bits 4-5 genotype), letter / in_repeat uint8 [m], position / depth / support int64 [m], prediction float32 [m, 3],
    names (bytes: m NUL-terminated strings) and name_offsets int64 [m + 1]."""

    __slots__ = ("row", "flags", "letter", "in_repeat", "position", "depth", "support", "prediction", "names", "name_offsets")

    def __len__(self):
        return len(self.row)

    @classmethod
    def empty(cls):
        t = cls()
        t.row, t.flags, t.letter, t.in_repeat = np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        t.position, t.depth, t.support = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
        t.prediction, t.names, t.name_offsets = np.zeros((0, 3), np.float32), b"", np.zeros(1, np.int64)
        return t

    def nbytes(self):
        return sum(getattr(self, k).nbytes for k in self.__slots__ if k != "names") + len(self.names)


class DeviceSelector(object):
    """One per (thread, stream).  stream: a torch stream whose work the runs follow (None: a stream of the handle's own)."""

    def __init__(self, device=0, stream=None):
        self.lib = _lib.load()
        self.device = int(device)
        self.handle = ctypes.c_void_p()
        raw = None if stream is None else ctypes.c_void_p(int(getattr(stream, "cuda_stream", stream)))
        _lib.check(self.lib.pa_selector_create(self.device, raw, ctypes.byref(self.handle)))
        self.summary = _lib.Selection()

    def close(self):
        if self.handle:
            self.lib.pa_selector_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 -- interpreter shutdown
            pass

    @staticmethod
    def limits():
        """{"rows_per_workgroup", "scan_block", "max_name", "scan_level", "max_rows"} (pa_selector_limits)."""
        out = (ctypes.c_int64 * 5)()
        _lib.check(_lib.load().pa_selector_limits(out, 5))
        return dict(zip(("rows_per_workgroup", "scan_block", "max_name", "scan_level", "max_rows"), [int(v) for v in out]))

    def set_ploidy(self, haploid, par_starts=None, par_ends=None):
        """The ploidy of the contig the next runs are about (pa_selector_set_ploidy; Ploidy.table gives the three).  haploid
        false: every row diploid, as a new selector.  The table is uploaded here; a call with the table the selector already
        holds does nothing."""
        starts = np.ascontiguousarray(par_starts if haploid and par_starts is not None else [], np.int64)
        ends = np.ascontiguousarray(par_ends if haploid and par_ends is not None else [], np.int64)
        key = (bool(haploid), starts.tobytes(), ends.tobytes())
        if key == getattr(self, "_ploidy_key", (False, b"", b"")):
            return
        self._ploidy_key = None                                  # (a failed set leaves the handle diploid)
        _lib.check(self.lib.pa_selector_set_ploidy(self.handle, 1 if haploid else 0, len(starts),
                                                   ctypes.c_void_p(starts.ctypes.data if len(starts) else 0),
                                                   ctypes.c_void_p(ends.ctypes.data if len(ends) else 0)))
        self._ploidy_key = key

    def run(self, rules, position, depth, support, prediction, names, regions):
        """One call's rows.  Either every array is numpy / bytes (uploaded) or every array is a torch tensor on the selector's
        device (names: uint8).  regions: [(first_row, reference_start, reference)] with reference bytes (host form) or a uint8
        device tensor.  -> (status, kept rows, kept name bytes); status != 0: handed back, take() would raise."""
        on_device = _is_tensor(position)
        keep = []
        if on_device:
            n = int(position.shape[0])
            name_bytes = int(names.numel())
            ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)      # noqa: E731
            a_pos, a_dep, a_sup, a_pred, a_names = (ptr(t.contiguous()) for t in (position, depth, support, prediction, names))
            keep = [position, depth, support, prediction, names]
        else:
            pos = np.ascontiguousarray(position, np.int64)
            n = len(pos)
            dep, sup = np.ascontiguousarray(depth, np.int32), np.ascontiguousarray(support, np.int32)
            pred = np.ascontiguousarray(prediction, np.float32).reshape(n, 3)
            blob = bytes(names)
            name_bytes = len(blob)
            a_pos, a_dep, a_sup, a_pred = (ctypes.c_void_p(a.ctypes.data) for a in (pos, dep, sup, pred))
            a_names = ctypes.c_char_p(blob)
            keep = [pos, dep, sup, pred, blob]
        table = (_lib.SelectorRegion * max(1, len(regions)))()
        for k, (first_row, start, reference) in enumerate(regions):
            if _is_tensor(reference):
                table[k] = _lib.SelectorRegion(int(first_row), int(start), reference.data_ptr() if reference.numel() else 0,
                                               int(reference.numel()))
            else:
                text = bytes(reference)
                table[k] = _lib.SelectorRegion(int(first_row), int(start), ctypes.cast(ctypes.c_char_p(text), ctypes.c_void_p).value,
                                               len(text))
                keep.append(text)
            keep.append(reference)
        _lib.check(self.lib.pa_selector_run(self.handle, ctypes.byref(rules), n, a_pos, a_dep, a_sup, a_pred, a_names, name_bytes,
                                            len(regions), table, 1 if on_device else 0, ctypes.byref(self.summary)))
        del keep
        return self.summary.status, self.summary.kept_rows, self.summary.kept_name_bytes

    def run_encoder(self, encoder_handle, rules, probabilities):
        """The encoder's last variant run (its handle) with the probabilities [n, 3] float32 in a device tensor (or a device
        address): lists, references and regions are read where that run left them."""
        ptr = probabilities.data_ptr() if _is_tensor(probabilities) else int(probabilities or 0)
        _lib.check(self.lib.pa_encoder_select_candidates(encoder_handle, self.handle, ctypes.c_void_p(ptr), ctypes.byref(rules),
                                                         ctypes.byref(self.summary)))
        return self.summary.status, self.summary.kept_rows, self.summary.kept_name_bytes

    def take(self):
        """The kept rows of the last run -> Taken."""
        m, name_bytes = int(self.summary.kept_rows), int(self.summary.kept_name_bytes)
        if self.summary.status:
            m = name_bytes = 0                 # (the library refuses the call below with its reason)
        t = Taken()
        t.row, t.flags = np.empty(m, np.int32), np.empty(m, np.uint8)
        t.letter, t.in_repeat = np.empty(m, np.uint8), np.empty(m, np.uint8)
        t.position, t.depth, t.support = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64)
        t.prediction = np.empty((m, 3), np.float32)
        names = np.empty(name_bytes, np.uint8)
        t.name_offsets = np.empty(m + 1, np.int64)
        _lib.check(self.lib.pa_selector_take(self.handle, *[ctypes.c_void_p(a.ctypes.data) for a in (
            t.row, t.flags, t.letter, t.in_repeat, t.position, t.depth, t.support, t.prediction, names, t.name_offsets)]))
        t.names = names.tobytes()
        return t


def segment(rules, contig, taken):
    """A Taken -> the FastCandidates._Segment native_batch_arrays would have built from the call's full lists: the compacted
    arrays go through pa_candidates_select_format for the lines, len(REF), snp and sel.  contig: the call's one contig name
    (bytes or str).  The library must keep all m rows: any other count means the device and the host disagree about a row, which
    is an error and not a reason to fall back."""
    first = contig.encode() if isinstance(contig, str) else bytes(contig)
    m = len(taken)
    if m == 0:
        return _with_bytes(taken.nbytes(), FastCandidates._Segment(first.decode("UTF-8"), np.zeros(0, np.int64), np.zeros(0, np.int32),
                                                                   np.zeros(0, bool), np.zeros(0, bool), []))
    io = h5.load()
    row, ref_len, flags = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.uint8)
    offsets = np.empty(m + 1, np.int64)
    cap = len(taken.names) + m * (len(first) + 200)
    lines = np.empty(cap, np.uint8)
    # (flags bit 3: the rows the device decided as haploid.  The prediction is the model's triple: the library primes it again)
    haploid = np.ascontiguousarray((taken.flags >> 3) & 1)
    kept = io.pa_candidates_select_format_ploidy(
        ctypes.byref(rules), first, m, taken.position.ctypes.data, taken.depth.ctypes.data, taken.support.ctypes.data,
        taken.prediction.ctypes.data, taken.letter.ctypes.data, taken.in_repeat.ctypes.data, taken.names,
        taken.name_offsets.ctypes.data, 1, row.ctypes.data, ref_len.ctypes.data, flags.ctypes.data,
        ctypes.c_void_p(lines.ctypes.data), cap, offsets.ctypes.data, haploid.ctypes.data if haploid.any() else None)
    if kept == -1:
        raise h5.H5Error(io.pa_h5_last_error().decode())
    if kept != m or (flags & 0x3d != taken.flags).any():
        raise RuntimeError("device selection kept %d rows of a call and pa_candidates_select_format keeps %d of them (or their flags "
                           "differ): the device and the host disagree" % (m, kept))
    cut = offsets.tolist()
    raw_lines = lines[:cut[m]].tobytes()
    return _with_bytes(taken.nbytes(), FastCandidates._Segment(first.decode("UTF-8"), taken.position.copy(), ref_len, (flags & 1).astype(bool), (flags & 2).astype(bool),
                                   [raw_lines[cut[k]:cut[k + 1]] for k in range(m)],
                                   raw=(row, flags, taken.position, taken.depth, taken.support, taken.prediction, taken.letter,
                                        taken.in_repeat, taken.names, taken.name_offsets)))


def _with_bytes(nbytes, seg):
    seg.downloaded_bytes = nbytes      # what crossed PCIe for this segment (its summary's 24 bytes aside)
    return seg
