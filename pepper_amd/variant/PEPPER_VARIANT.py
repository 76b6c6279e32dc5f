"""Python shim with the names of the reference's pybind11 module for the summary encoder.

Mirrors the part of `from pepper_variant.build import PEPPER_VARIANT` that image generation uses
(/root/reference/pepper_variant/modules/cpp/pybind_api.h:55-62 RegionalSummaryGenerator, :73-101
CandidateImageSummary, :187-221 CigarOp / type_read_flags / type_read; call site
/root/reference/pepper_variant/modules/python/AlignmentSummarizer.py:220-238).  Reads may be any
objects with the type_read attributes (pos, flags.is_reverse, sequence, cigar_tuples[.cigar_op,
.cigar_len], mapping_quality, base_qualities); they are flattened once and encoded by
libpepper_amd.so (include/pepper_amd_encoder.h).  `generate_summary_arrays` returns the bulk
struct-of-arrays form (images already int8-packed on the device) for callers that do not need
per-candidate Python objects.
"""
import collections
import contextlib
import ctypes
import threading
import time

import numpy as np

from pepper_amd import _lib
from pepper_amd.variant.bam import RECORD_HEADER, BamError


class CigarOp(object):
    def __init__(self, cigar_op=-1, cigar_len=0):
        self.cigar_op = cigar_op
        self.cigar_len = cigar_len


class type_read_flags(object):
    def __init__(self):
        for name in ("is_paired", "is_proper_pair", "is_unmapped", "is_mate_unmapped", "is_reverse",
                     "is_mate_is_reverse", "is_read1", "is_read2", "is_secondary", "is_qc_failed",
                     "is_duplicate", "is_supplementary"):
            setattr(self, name, False)


class type_read(object):
    def __init__(self):
        self.pos = 0
        self.pos_end = 0
        self.query_name = ""
        self.read_id = 0
        self.flags = type_read_flags()
        self.hp_tag = 0
        self.sequence = ""
        self.cigar_tuples = []
        self.mapping_quality = 0
        self.base_qualities = []
        self.bad_indicies = []

    def set_read_id(self, read_id):
        self.read_id = read_id

    def __lt__(self, other):
        return (self.pos, self.pos_end) < (other.pos, other.pos_end)


class CandidateImageSummary(object):
    def __init__(self, contig="", position=0, depth=0, candidates=None, candidate_frequency=None,
                 image_matrix=None, base_label=0, type_label=0):
        self.contig = contig
        self.position = position
        self.depth = depth
        self.candidates = candidates if candidates is not None else []
        self.candidate_frequency = candidate_frequency if candidate_frequency is not None else []
        self.image_matrix = image_matrix if image_matrix is not None else []
        self.base_label = base_label
        self.type_label = type_label

    def __getstate__(self):
        return (self.contig, self.position, self.depth, self.candidates, self.candidate_frequency,
                self.image_matrix, self.base_label, self.type_label)

    def __setstate__(self, t):
        if len(t) != 8:
            raise RuntimeError("Invalid state!")
        (self.contig, self.position, self.depth, self.candidates, self.candidate_frequency,
         self.image_matrix, self.base_label, self.type_label) = t


class _Pileup(ctypes.Structure):
    _fields_ = [("region_start", ctypes.c_int64), ("region_end", ctypes.c_int64),
                ("reference", ctypes.c_char_p), ("reference_len", ctypes.c_int64), ("n_reads", ctypes.c_int32),
                ("read_pos", ctypes.c_void_p), ("read_reverse", ctypes.c_void_p), ("read_mapq", ctypes.c_void_p),
                ("seq_offset", ctypes.c_void_p), ("seq", ctypes.c_void_p), ("qual", ctypes.c_void_p),
                ("cigar_offset", ctypes.c_void_p), ("cigar_op", ctypes.c_void_p), ("cigar_len", ctypes.c_void_p)]


class _Params(ctypes.Structure):
    _fields_ = [("min_snp_baseq", ctypes.c_double), ("min_indel_baseq", ctypes.c_double),
                ("snp_freq_threshold", ctypes.c_double), ("insert_freq_threshold", ctypes.c_double),
                ("delete_freq_threshold", ctypes.c_double), ("min_coverage_threshold", ctypes.c_double),
                ("snp_candidate_freq_threshold", ctypes.c_double),
                ("indel_candidate_freq_threshold", ctypes.c_double),
                ("candidate_support_threshold", ctypes.c_double), ("skip_indels", ctypes.c_int32),
                ("candidate_region_start", ctypes.c_int64), ("candidate_region_end", ctypes.c_int64),
                ("candidate_window_size", ctypes.c_int32), ("feature_size", ctypes.c_int32)]


_encoders = {}


def _encoder(device):
    """One native encoder (stream + workspace) per device per THREAD, created on first use: a handle holds the
    results of its last call, so image-generation worker threads must not share one."""
    import threading
    lib = _lib.load()
    key = (device, threading.get_ident())
    if key not in _encoders:
        h = ctypes.c_void_p()
        _lib.check(lib.pa_encoder_create(device, None, ctypes.byref(h)))
        _encoders[key] = h
    return lib, _encoders[key]


def set_device_candidates(on, device=0):
    """Candidates of this thread's encoder on `device` enumerated on the device (pa_encoder_set_device_candidates) from its
    next call on: what RegionalSummaryGenerator, StagedBatch and generate_summary_arrays_batch run on."""
    lib, enc = _encoder(device)
    _lib.check(lib.pa_encoder_set_device_candidates(enc, 1 if on else 0))


def candidate_calls(device=0):
    """-> (calls enumerated on the device, calls handed back to the host) of this thread's encoder on `device`."""
    lib, enc = _encoder(device)
    return _calls_pair(lib.pa_encoder_candidate_calls, enc)


def _send_targets(lib, enc, table):
    """pa_encoder_set_targets: table = (starts, ends) of one contig, merged (pepper_amd/variant/Targets.py), or None: none."""
    if table is None:
        _lib.check(lib.pa_encoder_set_targets(enc, 0, None, None))
        return
    starts, ends = np.ascontiguousarray(table[0], np.int64), np.ascontiguousarray(table[1], np.int64)
    _lib.check(lib.pa_encoder_set_targets(enc, len(starts), starts.ctypes.data, ends.ctypes.data))


@contextlib.contextmanager
def thread_targets(table, device=0):
    """This thread's encoder on `device` -- what RegionalSummaryGenerator and generate_summary_arrays_batch run on -- restricted
    to the targets of one contig for the calls inside, and unrestricted again behind them: the handle outlives the job."""
    lib, enc = _encoder(device)
    _send_targets(lib, enc, table)
    try:
        yield
    finally:
        _send_targets(lib, enc, None)


def _send_depth_bins(lib, enc, bins):
    """pa_encoder_set_depth_bins: ascending lower bounds starting at 0 (pepper_amd/variant/Coverage.py parse_bins), None: off."""
    if bins is None or len(bins) == 0:
        _lib.check(lib.pa_encoder_set_depth_bins(enc, 0, None))
        return
    lower = np.ascontiguousarray(bins, np.int32)
    _lib.check(lib.pa_encoder_set_depth_bins(enc, len(lower), lower.ctypes.data))


def _send_ref_confidence(lib, enc, table, bands):
    """pa_encoder_set_ref_confidence: the 101 x 101 uint8 table of pepper_amd/variant/RefConfidence.py build_table and ascending
    lower bounds of GQ starting at 0 (parse_bands); bands None: off."""
    if bands is None or len(bands) == 0:
        _lib.check(lib.pa_encoder_set_ref_confidence(enc, None, 0, 0, None))
        return
    table = np.ascontiguousarray(table, np.uint8)
    if table.ndim != 2 or table.shape[0] != table.shape[1]:
        raise ValueError("reference confidence: the table must be square, not %r" % (table.shape,))
    lower = np.ascontiguousarray(bands, np.int32)
    _lib.check(lib.pa_encoder_set_ref_confidence(enc, table.ctypes.data, table.shape[0], len(lower), lower.ctypes.data))


def _fetch_records(fetch, enc, dtypes):
    """The records of the handle's last run from pa_encoder_depth_runs / pa_encoder_ref_blocks: asked for their number, then
    fetched into one array per column."""
    n = ctypes.c_int64()
    _lib.check(fetch(enc, 0, *([None] * len(dtypes)), ctypes.byref(n)))
    cols = [np.zeros(max(1, n.value), t) for t in dtypes]
    _lib.check(fetch(enc, len(cols[0]), *(c.ctypes.data for c in cols), ctypes.byref(n)))
    return tuple(c[:n.value] for c in cols)


def _calls_pair(calls, enc):
    """The two counters of pa_encoder_depth_calls, pa_encoder_ref_calls and their like."""
    first, second = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(calls(enc, ctypes.byref(first), ctypes.byref(second)))
    return first.value, second.value


class _TrackReads(object):
    """What a holder of an encoder handle (self.lib, self.enc) can ask about the per-position tracks of the handle's last run."""

    def depth_runs(self):
        """pa_encoder_depth_runs -> (region int32, start int64, end int64, bin int32): every region's runs in region and
        position order, contig coordinates, ends half-open, bin -1 outside the targets."""
        return _fetch_records(self.lib.pa_encoder_depth_runs, self.enc, (np.int32, np.int64, np.int64, np.int32))

    def depth_totals(self, n_regions):
        """pa_encoder_depth_totals -> (bases per bin int64 [n_regions, 8], sum of depths int64 [n_regions])."""
        bases, sums = np.zeros((max(1, n_regions), 8), np.int64), np.zeros(max(1, n_regions), np.int64)
        _lib.check(self.lib.pa_encoder_depth_totals(self.enc, n_regions, bases.ctypes.data, sums.ctypes.data))
        return bases[:n_regions], sums[:n_regions]

    def depth_calls(self):
        """-> (runs made with depth bins set, runs among them whose records were emitted twice) since the handle was created."""
        return _calls_pair(self.lib.pa_encoder_depth_calls, self.enc)

    def ref_blocks(self):
        """pa_encoder_ref_blocks -> (region int32, start int64, end int64, band int32, min_dp int32, min_gq int32): every
        region's records in region and position order, contig coordinates, ends half-open, band -1 outside the targets; a run
        that crosses a tile border comes as one record per tile (RefConfidence.merge_blocks joins them)."""
        return _fetch_records(self.lib.pa_encoder_ref_blocks, self.enc, (np.int32, np.int64, np.int64, np.int32, np.int32, np.int32))

    def ref_calls(self):
        """-> (runs made with a table set, runs among them whose records were emitted twice) since the handle was created."""
        return _calls_pair(self.lib.pa_encoder_ref_calls, self.enc)

    def ref_blocks_ms(self):
        """Event time of the reference-block kernels of the last run (pa_encoder_last_timing [14]; 0 without a table)."""
        ms = np.zeros(15, np.float64)
        _lib.check(self.lib.pa_encoder_last_timing(self.enc, ms.ctypes.data, 15))
        return float(ms[14])


class _ThreadTracks(_TrackReads):
    """What thread_depth_bins and thread_ref_confidence yield: this thread's encoder, under the names PackedEncoder gives."""

    def __init__(self, lib, enc):
        self.lib, self.enc = lib, enc


@contextlib.contextmanager
def _thread_track(send, device, *setting):
    """This thread's encoder on `device` -- what RegionalSummaryGenerator and generate_summary_arrays_batch run on -- with a
    track's setting sent for the calls inside and taken back behind them: the handle outlives the job."""
    lib, enc = _encoder(device)
    send(lib, enc, *setting)
    try:
        yield _ThreadTracks(lib, enc)
    finally:
        send(lib, enc, *([None] * len(setting)))


def thread_depth_bins(bins, device=0):
    """Depth bins (pa_encoder_set_depth_bins) on this thread's encoder for the calls inside.  Yields an object whose
    depth_runs() / depth_totals(n_regions) / depth_calls() speak of that handle's last run."""
    return _thread_track(_send_depth_bins, device, bins)


def thread_ref_confidence(table, bands, device=0):
    """A reference-confidence table (pa_encoder_set_ref_confidence) on this thread's encoder for the calls inside.  Yields an
    object whose ref_blocks() / ref_calls() / ref_blocks_ms() speak of that handle's last run."""
    return _thread_track(_send_ref_confidence, device, table, bands)


def flatten_reads(reads):
    """type_read-like objects -> the flat arrays of pa_pileup."""
    n = len(reads)
    read_pos = np.fromiter((r.pos for r in reads), np.int64, n)
    read_reverse = np.fromiter((1 if r.flags.is_reverse else 0 for r in reads), np.uint8, n)
    read_mapq = np.fromiter((r.mapping_quality for r in reads), np.int32, n)
    seq_offset = np.zeros(n + 1, np.int64)
    cigar_offset = np.zeros(n + 1, np.int64)
    np.cumsum([len(r.sequence) for r in reads], out=seq_offset[1:])
    np.cumsum([len(r.cigar_tuples) for r in reads], out=cigar_offset[1:])
    seq = np.frombuffer(("".join(r.sequence for r in reads)).encode("latin-1") + b"\0", np.uint8)
    qual = np.zeros(int(seq_offset[-1]) + 1, np.uint8)
    for i, r in enumerate(reads):
        qual[seq_offset[i]:seq_offset[i + 1]] = np.clip(np.asarray(r.base_qualities, np.int64), 0, 255)
    cigar_op = np.fromiter((c.cigar_op for r in reads for c in r.cigar_tuples), np.int32, int(cigar_offset[-1]))
    cigar_len = np.fromiter((c.cigar_len for r in reads for c in r.cigar_tuples), np.int32, int(cigar_offset[-1]))
    return dict(read_pos=read_pos, read_reverse=read_reverse, read_mapq=read_mapq, seq_offset=seq_offset,
                seq=seq, qual=qual, cigar_offset=cigar_offset, cigar_op=np.append(cigar_op, 0).astype(np.int32),
                cigar_len=np.append(cigar_len, 0).astype(np.int32), n_reads=n)


class RegionalSummaryGenerator(object):
    def __init__(self, contig, region_start, region_end, reference_sequence, device=0):
        self.contig = contig
        self.ref_start = int(region_start)
        self.ref_end = int(region_end)
        self.reference_sequence = reference_sequence
        self.device = device
        # GENERATE_INDELS == false in the reference (region_summary.h:50): no insert columns
        self.total_observered_insert_bases = 0

    def set_device_candidates(self, on):
        """The switch of the encoder this generator's calls run on (this thread's, on its device)."""
        set_device_candidates(on, self.device)

    def generate_max_insert_summary(self, reads):
        """Axes of the region.  With GENERATE_INDELS false every max_observed_insert entry is 0, so
        positions[i] = ref_start + i and index[i] = 0 (region_summary.cpp:19-96); nothing to compute."""
        return None

    def generate_summary_arrays(self, reads, min_snp_baseq, min_indel_baseq, snp_freq_threshold,
                                insert_freq_threshold, delete_freq_threshold, min_coverage_threshold,
                                snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                                candidate_support_threshold, skip_indels, candidate_region_start,
                                candidate_region_end, candidate_window_size, feature_size, train_mode=False,
                                want_int32=False):
        return generate_summary_arrays_batch([self], [reads], min_snp_baseq, min_indel_baseq, snp_freq_threshold,
                                             insert_freq_threshold, delete_freq_threshold, min_coverage_threshold,
                                             snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                                             candidate_support_threshold, skip_indels,
                                             [(candidate_region_start, candidate_region_end)], candidate_window_size,
                                             feature_size, train_mode, want_int32)[0]

    def generate_summary(self, reads, *args):
        """-> list[CandidateImageSummary], as the pybind method (region_summary.h:191-206)."""
        out = self.generate_summary_arrays(reads, *args, want_int32=True)
        res = []
        for i in range(len(out["candidates"])):
            res.append(CandidateImageSummary(self.contig, int(out["positions"][i]), int(out["depths"][i]),
                                             [out["candidates"][i]], [int(out["candidate_frequency"][i])],
                                             out["images_int32"][i].tolist(), 0, 0))
        return res


def _pileup_struct(gen, flat, keep):
    ref = gen.reference_sequence.encode("latin-1") if isinstance(gen.reference_sequence, str) else bytes(gen.reference_sequence)
    keep.append(ref)
    return _Pileup(gen.ref_start, gen.ref_end, ref, len(ref), flat["n_reads"],
                   flat["read_pos"].ctypes.data, flat["read_reverse"].ctypes.data, flat["read_mapq"].ctypes.data,
                   flat["seq_offset"].ctypes.data, flat["seq"].ctypes.data, flat["qual"].ctypes.data,
                   flat["cigar_offset"].ctypes.data, flat["cigar_op"].ctypes.data, flat["cigar_len"].ctypes.data)


class StagedBatch(_TrackReads):
    """A batch of regions uploaded once (pa_encoder_stage_batch) and encoded any number of times
    (pa_encoder_run_staged): what bench.py times with the inputs resident in HBM."""

    def __init__(self, generators, reads_list, params, candidate_regions, candidate_window_size=32, feature_size=26):
        device = generators[0].device if generators else 0
        self.lib, self.enc = _encoder(device)
        self.n_regions = len(generators)
        self.window, self.features = candidate_window_size + 1, feature_size
        self._keep = []
        self.flats = [r if isinstance(r, dict) else flatten_reads(r) for r in reads_list]
        self.piles = (_Pileup * max(1, self.n_regions))(*[_pileup_struct(g, f, self._keep) for g, f in zip(generators, self.flats)])
        (min_snp_baseq, min_indel_baseq, snp_freq_threshold, insert_freq_threshold, delete_freq_threshold,
         min_coverage_threshold, snp_candidate_freq_threshold, indel_candidate_freq_threshold,
         candidate_support_threshold, skip_indels) = params
        self.params = (_Params * max(1, self.n_regions))(*[
            _Params(min_snp_baseq, min_indel_baseq, snp_freq_threshold, insert_freq_threshold, delete_freq_threshold,
                    min_coverage_threshold, snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                    candidate_support_threshold, 1 if skip_indels else 0, int(lo), int(hi), int(candidate_window_size),
                    int(feature_size)) for lo, hi in candidate_regions])
        _lib.check(self.lib.pa_encoder_stage_batch(self.enc, self.n_regions, ctypes.cast(self.piles, ctypes.c_void_p),
                                                   ctypes.cast(self.params, ctypes.c_void_p)))
        self.counts = np.zeros(max(1, self.n_regions), np.int64)

    def run(self):
        """-> candidates per region"""
        _lib.check(self.lib.pa_encoder_run_staged(self.enc, self.counts.ctypes.data))
        return self.counts[:self.n_regions]

    def timing(self):
        ms = np.zeros(13, np.float64)
        _lib.check(self.lib.pa_encoder_last_timing(self.enc, ms.ctypes.data, 13))
        return dict(records_ms=ms[0], tile_count_ms=ms[1], compact_votes_ms=ms[2], gather_windows_ms=ms[3],
                    host_enumeration_ms=ms[4], run_ms=ms[5], host_bucket_ms=ms[6], host_bucket_and_threads_ms=ms[7],
                    upload_ms=ms[8], unpack_clip_ms=ms[9], device_enumeration_ms=ms[12])

    def depth_runs_ms(self):
        """Event time of the depth-class kernels of the last run (pa_encoder_last_timing [13]; 0 without depth bins)."""
        ms = np.zeros(14, np.float64)
        _lib.check(self.lib.pa_encoder_last_timing(self.enc, ms.ctypes.data, 14))
        return float(ms[13])

    def stats(self):
        v = np.zeros(6, np.int64)
        _lib.check(self.lib.pa_encoder_batch_stats(self.enc, v.ctypes.data, 6))
        return dict(bases=int(v[0]), rows=int(v[1]), reads=int(v[2]), cigar_ops=int(v[3]), tiles=int(v[4]), regions=int(v[5]))

    def results(self, want_int32=False):
        """-> one dict per region (the arrays of generate_summary_arrays)"""
        n = int(self.counts[:self.n_regions].sum())
        W, F = self.window, self.features
        positions = np.zeros(n, np.int64)
        depths = np.zeros(n, np.int32)
        freqs = np.zeros(n, np.int32)
        img8 = np.zeros((n, W, F), np.int8)
        img32 = np.zeros((n, W, F), np.int32) if want_int32 else None
        needed = ctypes.c_int64()
        lib, enc = self.lib, self.enc
        _lib.check(lib.pa_encoder_get_results(enc, None, None, None, None, None, None, 0, ctypes.byref(needed)))
        names = ctypes.create_string_buffer(max(1, needed.value))
        _lib.check(lib.pa_encoder_get_results(enc, positions.ctypes.data, depths.ctypes.data, freqs.ctypes.data,
                                              img32.ctypes.data if want_int32 else None, img8.ctypes.data,
                                              ctypes.cast(names, ctypes.c_void_p), needed.value, ctypes.byref(needed)))
        raw = names.raw[:needed.value]
        cands = [s.decode("latin-1") for s in raw.split(b"\0")[:n]]
        # the same strings as the library left them (NUL-terminated, back to back) with their offsets: what the image writer
        # takes without going through n Python strings again (DataStore.write_summary_packed)
        ends = np.flatnonzero(np.frombuffer(raw, np.uint8) == 0)[:n].astype(np.int64) + 1
        starts = np.concatenate([[0], ends]) if n else np.zeros(1, np.int64)
        out, at = [], 0
        for k in self.counts[:self.n_regions]:
            k = int(k)
            lo, hi = int(starts[at]), int(starts[at + k])
            out.append(dict(positions=positions[at:at + k], depths=depths[at:at + k], candidate_frequency=freqs[at:at + k],
                            images=img8[at:at + k], images_int32=img32[at:at + k] if want_int32 else None,
                            candidates=cands[at:at + k], candidates_blob=raw[lo:hi], candidates_offsets=starts[at:at + k + 1] - lo))
            at += k
        return out


class _PackedRegion(ctypes.Structure):
    _fields_ = [("region_start", ctypes.c_int64), ("region_end", ctypes.c_int64), ("reference", ctypes.c_char_p),
                ("reference_len", ctypes.c_int64)]


# PackedEncoder._fit_span: the n regions whose file span was read (first: where its first record starts, final: none of the
# contig behind it) or holds no record; _walk_on_device: one of four outcomes, what comes with it, whether the pack came back
_Span = collections.namedtuple("_Span", "n first final n_blocks comp_bytes out_bytes")
_EmptySpan = collections.namedtuple("_EmptySpan", "n")
_Walked = collections.namedtuple("_Walked", "outcome detail handed_back")
PACKED_ON_DEVICE, HEADERS_ON_HOST, HOST_MUST_WALK, STALE_INDEX = "packed on device", "headers on host", "host must walk", "stale index"


def _lap(laps, key, t0):
    """laps[key] += the time since t0 (laps None: nobody asked) -> now"""
    now = time.perf_counter()
    if laps is not None:
        laps[key] = laps.get(key, 0.0) + now - t0
    return now


class PackedEncoder(_TrackReads):
    """The packed form of a batch (pa_encoder_stage_packed): the reads of a run of regions as pa_bam_pack_regions leaves them
    in this object's page-locked arena -- CIGAR words, 4-bit bases, qualities, once per read -- clipped to each region and
    decoded by the device.  One object per worker thread: it owns its encoder handle (stream, workspace, arena)."""

    _split_walk = False             # what pa_encoder_set_split_slices was last told (off on a new handle)
    host_walk_spans = 0             # pack_device calls that asked for the device's record walk and walked the span on the host after all
    _device_packed = False          # the last pack / pack_device left its tables on the device (pa_encoder_pack_records): encode stages from there
    pack_handbacks = 0              # pack_device(device_pack=True) calls whose span the device handed back to the host's pack_headers
    _idle = []                      # encoders returned by release(): a later job's workers take them instead of pinning new arenas
    _idle_lock = threading.Lock()

    @classmethod
    def acquire(cls, device=0, arena_bytes=192 << 20, host_threads=1, torch_stream=False):
        """An encoder from the process-wide pool (or a new one): pinning a 256 MB arena and the first device allocations cost
        ~0.15 s per worker, which a long-running process pays once.  Under a memlock / cgroup limit the page-locked arena may
        not be had at that size: the request is halved down to 16 MB before the error is passed on (a smaller arena means
        fewer intervals per call, nothing else); the callers fall back to the host-clipped form when even that fails."""
        with cls._idle_lock:
            for k, enc in enumerate(cls._idle):
                if (enc.device == device and enc.arena is not None and enc.arena.nbytes <= arena_bytes and enc.arena.nbytes >= min(arena_bytes, 16 << 20)
                        and (enc.stream is not None) == bool(torch_stream)):
                    enc = cls._idle.pop(k)
                    enc.set_targets(None)        # (whatever job had it last: its targets are not this one's)
                    enc.set_depth_bins(None)     # (... nor its depth bins)
                    enc.set_ref_confidence(None, None)       # (... nor its reference-confidence table)
                    return enc
        size = arena_bytes
        while True:
            try:
                return cls(device, size, host_threads=host_threads, torch_stream=torch_stream)
            except _lib.PepperAmdError:
                if size <= 16 << 20:
                    raise
                size >>= 1

    def release(self):
        with self._idle_lock:
            self._idle.append(self)

    def __init__(self, device=0, arena_bytes=192 << 20, max_reads=1 << 18, max_pairs=1 << 19, host_threads=0, torch_stream=False):
        from pepper_amd.variant.bam import PACKED_READ
        self.lib = _lib.load()
        self.device = device
        self.enc = ctypes.c_void_p()
        # torch_stream: the encoder works on a stream torch made (self.stream) instead of one of its own, so that a caller can queue
        # torch operations -- a copy of the results the encoder left on the device -- right behind the encoder's kernels, in the same
        # hardware queue (polish/fused.py: a copy on any other stream waits behind whatever shares that stream's queue)
        self.stream = None
        if torch_stream:
            import torch
            self.stream = torch.cuda.Stream(device=device)
        _lib.check(self.lib.pa_encoder_create(device, ctypes.c_void_p(self.stream.cuda_stream) if self.stream is not None else None,
                                              ctypes.byref(self.enc)))
        _lib.check(self.lib.pa_encoder_set_host_threads(self.enc, host_threads))
        ptr = self.lib.pa_encoder_host_arena(self.enc, arena_bytes)
        if not ptr:
            raise _lib.PepperAmdError("page-locked arena of %d bytes could not be allocated" % arena_bytes)
        self.arena = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(arena_bytes,))
        self.reads = np.zeros(max_reads, PACKED_READ)
        self.pair_read = np.zeros(max_pairs, np.int32)
        self.span = None                # page-locked block for a file span's BGZF members (pack_device), allocated on first use
        self.tables = None
        self.headers = None             # record headers of a span as the device's walk returns them
        self.entries = None
        self.inflate_ms = 0.0           # device time of the inflate kernels of this object's pack_device calls
        self.inflated_bytes = 0
        self.seq_off = None             # pack_device(long_cigars=True): where the reads with a CIGAR in the CG tag keep their bases
        self.long_cigar_reads = 0       # such reads kept on the device path, counted once per pack_device call that kept them
        self._split_walk = False
        self.host_walk_spans = 0
        self._device_packed = False
        self.pack_handbacks = 0
        self._targets_contig = None

    def close(self):
        if self.enc:
            self.arena = None
            self.lib.pa_encoder_destroy(self.enc)
            self.enc = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sampling(self, sampling):
        """(seed, max_reads[, rate]) for this handle's next runs, None: off (pa_encoder_set_sampling)."""
        if sampling is None:
            seed, cap, rate = 0, 0, 1.0
        else:
            seed, cap = int(sampling[0]), int(sampling[1])
            rate = float(sampling[2]) if len(sampling) > 2 else 1.0
        _lib.check(self.lib.pa_encoder_set_sampling(self.enc, seed, cap, rate))

    def set_device_candidates(self, on):
        """Candidates of this handle's next runs enumerated on the device (pa_encoder_set_device_candidates)."""
        _lib.check(self.lib.pa_encoder_set_device_candidates(self.enc, 1 if on else 0))

    def set_targets(self, table, contig=None):
        """The targets of this handle's next runs (pa_encoder_set_targets): (starts, ends) of one contig, None: no restriction.
        contig: the table's contig; a call that names the contig the handle already has sends nothing (a worker's groups are
        runs of one contig)."""
        if table is not None and contig is not None and contig == self._targets_contig:
            return
        _send_targets(self.lib, self.enc, table)
        self._targets_contig = contig if table is not None else None

    def set_depth_bins(self, bins):
        """Depth classes of this handle's next runs (pa_encoder_set_depth_bins): ascending lower bounds starting at 0, None: off."""
        _send_depth_bins(self.lib, self.enc, bins)

    def set_ref_confidence(self, table, bands):
        """Reference blocks of this handle's next runs (pa_encoder_set_ref_confidence): RefConfidence.build_table's table and
        ascending lower bounds of GQ starting at 0; bands None: off."""
        _send_ref_confidence(self.lib, self.enc, table, bands)

    # depth_runs / depth_totals / depth_calls / ref_blocks / ref_calls / ref_blocks_ms of the last run: _TrackReads

    def candidate_calls(self):
        """-> (runs enumerated on the device, runs handed back to the host) since this handle was created."""
        return _calls_pair(self.lib.pa_encoder_candidate_calls, self.enc)

    def pack_calls(self):
        """-> (calls packed on the device, calls the device handed back) since this handle was created (pa_encoder_pack_calls)."""
        return _calls_pair(self.lib.pa_encoder_pack_calls, self.enc)

    def packed_tables(self, n_reads, n_pairs):
        """-> (reads, pair_read, seq_off): the tables the last device pack built, copied out (pa_encoder_packed_tables)."""
        from pepper_amd.variant.bam import PACKED_READ
        reads = np.zeros(max(1, int(n_reads)), PACKED_READ)
        pair_read = np.zeros(max(1, int(n_pairs)), np.int32)
        seq_off = np.zeros(max(1, int(n_reads)), np.int64)
        _lib.check(self.lib.pa_encoder_packed_tables(self.enc, reads.ctypes.data, pair_read.ctypes.data, seq_off.ctypes.data))
        return reads[:int(n_reads)], pair_read[:int(n_pairs)], seq_off[:int(n_reads)]

    def sampled(self):
        """-> (intervals the device sampled down, reads it dropped) since this handle was created."""
        regions, dropped = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self.lib.pa_encoder_sampled_regions(self.enc, ctypes.byref(regions), ctypes.byref(dropped)))
        return regions.value, dropped.value

    def pair_live(self, n_pairs):
        """uint8 [n_pairs]: 1 where the pair of the last packed batch is a read of its interval (pa_encoder_pair_live)."""
        keep = np.zeros(max(1, int(n_pairs)), np.uint8)
        _lib.check(self.lib.pa_encoder_pair_live(self.enc, keep.ctypes.data, int(n_pairs)))
        return keep[:int(n_pairs)]

    @property
    def device_packed(self):
        """True when the last pack / pack_device left its tables on the device (pack_device(device_pack=True), not handed
        back): encode(..., resident=True) stages from there, and the driver counts the call as device-packed."""
        return self._device_packed

    def pack(self, bam_handler, contig, starts, stops, include_supplementary, min_mapq):
        """-> (n_done, region_pairs, (n_reads, n_pairs, arena_bytes)): BAM_handler.pack_regions into this object's buffers."""
        self.seq_off = None
        self._device_packed = False
        return bam_handler.pack_regions(contig, starts, stops, include_supplementary, min_mapq, self.arena, self.reads, self.pair_read)

    def send_seq_offsets(self, n_reads, resident):
        """Before a staging call: the base offsets of the packed reads pack_device(long_cigars=True) left, if any (they describe
        the span resident on the device, so nothing is sent for the host arena)."""
        if resident and self.seq_off is not None and n_reads > 0:
            _lib.check(self.lib.pa_encoder_set_seq_offsets(self.enc, self.seq_off.ctypes.data, int(n_reads)))
        else:
            _lib.check(self.lib.pa_encoder_set_seq_offsets(self.enc, None, 0))

    def pack_device(self, bam_handler, contig, starts, stops, include_supplementary, min_mapq, lookahead_windows=4, laps=None,
                    long_cigars=False, device_pack=False):
        """The same tables with the BGZF members inflated ON THE DEVICE into the encoder's arena and the records left in place
        there -> (n_done, region_pairs, counts) for encode(..., resident=True), or None when the batch has to take pack().
        One step per rung: _fit_span, _inflate, _walk_on_device (PEPPER_AMD_DEVICE_WALK=0: skipped), _pack_on_host.
        long_cigars: records with their CIGAR in the CG tag stay in the span too -- operations read from the tag, bases from the
        core (self.seq_off); self.long_cigar_reads adds them up per call, so a read that reaches two calls counts twice.
        device_pack (with the device's walk): the tables are built where the headers lie and stay there; self.reads /
        self.pair_read are not filled, self.seq_off stays None, encode(..., resident=True) stages from the device tables."""
        self.seq_off, self._device_packed = None, False
        span = self._fit_span(bam_handler, contig, starts, stops, lookahead_windows, laps) if bam_handler.has_index() else None
        if span is None:
            return None
        if isinstance(span, _EmptySpan):             # no record of the contig: every region is done, with nothing in it
            return span.n, np.zeros(span.n + 1, np.int32), (0, 0, 0)
        batch = (contig, starts[:span.n], stops[:span.n], include_supplementary, min_mapq)
        t0 = time.perf_counter()
        device_walk = _lib.device_walk()
        self._inflate(span, host_copy=not device_walk)
        t0 = _lap(laps, "bam_inflate_device", t0)
        n_headers = None                             # (None: the host walks the span in self.arena)
        if device_walk:
            walked = self._walk_on_device(bam_handler, span, batch, long_cigars, device_pack)
            self.pack_handbacks += int(walked.handed_back)
            if walked.outcome == STALE_INDEX:
                return None                          # (the host packer reads the file itself)
            if walked.outcome == PACKED_ON_DEVICE:
                _lap(laps, "bam_walk_device", t0)
                summary, region_pairs = walked.detail
                self._device_packed = True
                self.long_cigar_reads += summary.n_split if long_cigars else 0
                return summary.n_done, region_pairs, (summary.n_reads, summary.n_pairs, int(span.out_bytes))
            if walked.outcome == HOST_MUST_WALK:
                self._inflate(span, host_copy=True)
                self.host_walk_spans += 1
            else:
                n_headers = walked.detail
            t0 = _lap(laps, "bam_walk_device", t0)
        try:
            packed = self._pack_on_host(bam_handler, span, batch, n_headers, long_cigars)
        finally:
            _lap(laps, "bam_walk", t0)
        if packed is None:
            return None
        n_done, region_pairs, counts = packed
        if long_cigars and counts[0] > 0:
            seq_off, n_split = bam_handler.split_offsets(counts[0])
            if n_split:
                self.seq_off = seq_off
                self.long_cigar_reads += n_split
        return n_done, region_pairs, (counts[0], counts[1], int(span.out_bytes))

    def _fit_span(self, bam_handler, contig, starts, stops, lookahead_windows, laps):
        """The largest run of regions -- all, half, a quarter, ... -- whose file span (BAM index) is complete and fits the arena,
        read into the page-locked span block (allocated on first use) -> _Span (bam_span_read is lapped), _EmptySpan, or None:
        no such block under this memlock limit, or no fit even for one region."""
        if self.span is None:
            cap = self.arena.nbytes + (1 << 20)
            ptr = self.lib.pa_encoder_host_span(self.enc, cap)
            if not ptr:
                return None
            self.span = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(cap,))
            nb = max(4096, self.arena.nbytes // 4096)
            self.tables = (np.zeros(nb, np.int64), np.zeros(nb, np.int32), np.zeros(nb, np.int64), np.zeros(nb, np.int32))
        t0 = time.perf_counter()
        n = len(starts)
        while n >= 1:
            begin, first, end, final = bam_handler.region_span(contig, int(starts[0]), int(stops[n - 1]), lookahead_windows)
            if end <= begin:
                return _EmptySpan(n)
            n_blocks, comp_bytes, out_bytes, complete, at_eof = bam_handler.read_span(begin, end, self.span, self.tables, 1)
            if complete and out_bytes + 256 <= self.arena.nbytes:
                _lap(laps, "bam_span_read", t0)
                return _Span(n, first, final or at_eof, n_blocks, comp_bytes, out_bytes)
            n //= 2
        return None

    def _inflate(self, span, host_copy):
        """pa_encoder_inflate_bgzf: the span's members into the device arena, one wavefront per member; host_copy: and down into
        self.arena for a walk on the host.  Kernel time and bytes add to inflate_ms / inflated_bytes, twice for a span inflated twice."""
        _lib.check(self.lib.pa_encoder_inflate_bgzf(self.enc, self.span.ctypes.data, span.comp_bytes, span.n_blocks,
                                                    *(table.ctypes.data for table in self.tables), span.out_bytes,
                                                    self.arena.ctypes.data if host_copy else None))
        ms = np.zeros(12, np.float64)
        _lib.check(self.lib.pa_encoder_last_timing(self.enc, ms.ctypes.data, 12))
        self.inflate_ms += float(ms[10])
        self.inflated_bytes += int(span.out_bytes)

    def _walk_on_device(self, bam_handler, span, batch, long_cigars, device_pack):
        """The record headers of the inflated span read out on the device -> _Walked: PACKED_ON_DEVICE (device_pack and a contig
        the header names: walk and pa_encoder_pack_records in one submission, one wait; detail = (summary, region_pairs)),
        HEADERS_ON_HOST (40 bytes per record came back instead of the span; detail = their number), HOST_MUST_WALK (a window of
        more records than a lane's slots, a tag walk that lost its way) or STALE_INDEX (entries outside the span)."""
        contig, starts, stops, include_supplementary, min_mapq = batch
        if self.headers is None:
            self.headers = np.zeros(max(1 << 16, self.arena.nbytes // 512), RECORD_HEADER)
            self.entries = np.zeros(8192, np.int64)
        n_entries = bam_handler.span_entries(contig, span.first, self.tables[2], span.n_blocks, self.entries)
        n_headers, flags = ctypes.c_int64(), np.zeros(2, np.int32)
        # slots per entry: 2 048 records of one 16 kb window, fewer when a span has very many windows (low coverage): the
        # device keeps two 40-byte tables of entries x slots; a window that overflows its slots takes the host walk
        walk = (self.enc, span.out_bytes, self.entries.ctypes.data, n_entries, max(64, min(2048, (32 << 20) // (40 * max(1, n_entries)))))
        download = (self.headers.ctypes.data, len(self.headers), ctypes.byref(n_headers), flags.ctypes.data)
        if bool(long_cigars) != self._split_walk:
            _lib.check(self.lib.pa_encoder_set_split_slices(self.enc, 1 if long_cigars else 0))
            self._split_walk = bool(long_cigars)
        tid = bam_handler.contig_index(contig) if device_pack else None
        summary, handed_back = None, False
        try:
            if tid is not None and tid >= 0:
                summary, region_pairs = _lib.DevicePack(), np.zeros(span.n + 1, np.int32)
                d_starts, d_stops = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(stops, np.int64)
                _lib.check(self.lib.pa_encoder_submit_walk(*walk))
                _lib.check(self.lib.pa_encoder_pack_records(self.enc, None, 0, int(bool(span.final)), int(tid), span.n, d_starts.ctypes.data,
                                                            d_stops.ctypes.data, int(bool(include_supplementary)), int(min_mapq),
                                                            len(self.reads), len(self.pair_read), region_pairs.ctypes.data,
                                                            ctypes.byref(summary)))
                flags[0], flags[1] = summary.walk_flags[0], summary.walk_flags[1]
                handed_back = flags[0] == 0 and summary.status != 0
                if handed_back:                      # the headers come down after all and the host's pack_headers decides
                    _lib.check(self.lib.pa_encoder_walk_headers(self.enc, *download))
            else:
                _lib.check(self.lib.pa_encoder_walk_records(*walk, *download))
        except _lib.PepperAmdError as err:
            if getattr(err, "code", 0) != _lib.PA_ERR_INVALID:
                raise
            return _Walked(STALE_INDEX, None, handed_back)
        if flags[0] != 0:
            return _Walked(HOST_MUST_WALK, None, handed_back)
        if summary is not None and not handed_back:
            return _Walked(PACKED_ON_DEVICE, (summary, region_pairs), False)
        return _Walked(HEADERS_ON_HOST, n_headers.value, handed_back)

    def _pack_on_host(self, bam_handler, span, batch, n_headers, long_cigars):
        """pack_headers over the n_headers the device read out, or -- None -- pack_inflated over the span in self.arena ->
        (n_done, region_pairs, counts).  What a BamError means: -7 / -8 / -9 (the reads outgrow the tables or the span's
        lookahead): None, the batch takes pack(); -6 from the headers under long_cigars (state 2 may be an auxiliary field the
        device's tag walk could not follow): the host's walk decides, which keeps such a record with its core CIGAR; else raised."""
        try:
            if n_headers is not None:
                return bam_handler.pack_headers(self.headers, n_headers, span.final, *batch, self.reads, self.pair_read, long_cigars=long_cigars)
            return bam_handler.pack_inflated(self.arena, span.out_bytes, span.first, span.final, *batch, self.reads, self.pair_read,
                                             long_cigars=long_cigars)
        except BamError as err:
            code = getattr(err, "code", 0)
            if code in (-7, -8, -9):
                return None
            if not (code == -6 and long_cigars and n_headers is not None):
                raise
        self._inflate(span, host_copy=True)
        self.host_walk_spans += 1
        return self._pack_on_host(bam_handler, span, batch, None, long_cigars)

    def fetch(self, bam_handler, contig, starts, stops, include_supplementary, min_mapq, device_inflate, laps, lap_resident,
              long_cigars=False, device_pack=False):
        """A group's reads for the image drivers: pack_device where the device inflate is on and takes the batch, else pack
        -> (resident, n_done, region_pairs, counts); resident: for encode(..., resident=True) / PolishChain.run.  n_done 0:
        the first region's reads outgrow the arena (pack's -7) and it has to take the driver's host form.  laps["bam_pack"]
        gets the time of a fetch that ended in pack, and with lap_resident that of one that stayed on the device too."""
        t0 = time.perf_counter()
        on_device = self.pack_device(bam_handler, contig, starts, stops, include_supplementary, min_mapq, laps=laps,
                                     long_cigars=long_cigars, device_pack=device_pack) if device_inflate else None
        if on_device is not None:
            if lap_resident:
                _lap(laps, "bam_pack", t0)
            return (True,) + on_device
        n_done, region_pairs, counts = 0, None, None
        try:
            n_done, region_pairs, counts = self.pack(bam_handler, contig, starts, stops, include_supplementary, min_mapq)
        except Exception as err:
            if getattr(err, "code", 0) != -7:
                raise
        _lap(laps, "bam_pack", t0)
        return False, n_done, region_pairs, counts

    def encode(self, regions, references, region_pairs, counts, params, candidate_regions, candidate_window_size=32, feature_size=26,
               want_int32=False, resident=False, sampling=None, fetch=True):
        """regions: [(ref_start, ref_end)] of the packed run (the fetch ranges), references: their sequences (bytes / str),
        region_pairs / counts: what pack() returned, params: the ten thresholds of generate_summary in order,
        candidate_regions: [(start, end)].  sampling: (seed, max_reads, downsample_rate) -- intervals with more reads than
        int(min(max_reads, rate * n)) are sampled down on the device as the reference does on the host
        (pa_encoder_set_sampling); None: not.  -> (one dict of arrays per region as generate_summary_arrays, reads per
        region -- after sampling).  fetch=False: no list and no image is downloaded -- the first value is then the candidates per
        region (int64 [n]), and the results stay on the device for pa_variant_forward_device and pa_encoder_select_candidates
        (self.last.results() still fetches them, e.g. for a call the device selection hands back)."""
        n = len(regions)
        self.set_sampling(sampling)
        refs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in references]
        regs = (_PackedRegion * max(1, n))(*[_PackedRegion(int(a), int(b), ref, len(ref)) for (a, b), ref in zip(regions, refs)])
        (min_snp_baseq, min_indel_baseq, snp_freq_threshold, insert_freq_threshold, delete_freq_threshold,
         min_coverage_threshold, snp_candidate_freq_threshold, indel_candidate_freq_threshold,
         candidate_support_threshold, skip_indels) = params
        pars = (_Params * max(1, n))(*[
            _Params(min_snp_baseq, min_indel_baseq, snp_freq_threshold, insert_freq_threshold, delete_freq_threshold,
                    min_coverage_threshold, snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                    candidate_support_threshold, 1 if skip_indels else 0, int(lo), int(hi), int(candidate_window_size),
                    int(feature_size)) for lo, hi in candidate_regions])
        region_pairs = np.ascontiguousarray(region_pairs[:n + 1], np.int32)
        n_reads, _n_pairs, arena_bytes = counts
        # resident: the arena is the inflated span pack_device left on the device
        if resident and self._device_packed:
            # the tables the last pack_device(device_pack=True) built are on the device, beside the span
            self.send_seq_offsets(0, False)
            _lib.check(self.lib.pa_encoder_stage_packed_device(self.enc, n, ctypes.cast(regs, ctypes.c_void_p),
                                                               ctypes.cast(pars, ctypes.c_void_p)))
        else:
            self.send_seq_offsets(n_reads, resident)
            _lib.check(self.lib.pa_encoder_stage_packed(self.enc, n, ctypes.cast(regs, ctypes.c_void_p), ctypes.cast(pars, ctypes.c_void_p),
                                                        None if (resident and n_reads > 0) else self.arena.ctypes.data,
                                                        int(arena_bytes), self.reads.ctypes.data, int(n_reads),
                                                        self.pair_read.ctypes.data, region_pairs.ctypes.data))
        batch = StagedBatch.__new__(StagedBatch)
        batch.lib, batch.enc, batch.n_regions = self.lib, self.enc, n
        batch.window, batch.features = candidate_window_size + 1, feature_size
        batch.counts = np.zeros(max(1, n), np.int64)
        batch._keep = (regs, pars, refs)
        batch.run()
        live = np.zeros(max(1, n), np.int32)
        _lib.check(self.lib.pa_encoder_region_reads(self.enc, live.ctypes.data, n))
        self.last = batch
        if not fetch:
            return batch.counts[:n].copy(), live[:n]
        return batch.results(want_int32), live[:n]


def adjacent_run(intervals, g0, batch, slack):
    """-> g1: intervals[g0:g1] is what one fetch of an image driver takes -- at most `batch` ADJACENT intervals (contig, start,
    end) of one contig, ascending: each starts no earlier than the one before it and at most `slack` bases behind its end, and
    ends no earlier.  (The packer walks every record between the first and the last region of a call: a group must not bridge
    the gap to the worker's next run of intervals.)"""
    g1 = g0 + 1
    while (g1 < len(intervals) and g1 - g0 < batch and intervals[g1][0] == intervals[g0][0]
           and intervals[g1 - 1][1] <= intervals[g1][1] <= intervals[g1 - 1][2] + slack
           and intervals[g1][2] >= intervals[g1 - 1][2]):
        g1 += 1
    return g1


_STATS_LOCK = threading.Lock()


def merge_stats(stats, mine):
    """A worker's stage times and counts added to the dict its caller shares among the workers (None: nobody asked)."""
    if stats is not None:
        with _STATS_LOCK:
            for key, v in mine.items():
                stats[key] = stats.get(key, 0.0) + v


@contextlib.contextmanager
def worker_counters(enc, mine, release_on_error, inflate_figures=False, candidates=False):
    """Around an image worker's loop over its groups: what the worker's PackedEncoder counted meanwhile -- intervals sampled
    down on the device, reads kept with their CIGAR in the CG tag -- is added to `mine`, the handle's switches are cleared and
    it goes back to the pool.  release_on_error: also when the loop raises (the polish driver; the variant driver leaves a
    handle that failed out of the pool).  inflate_figures: the inflate kernels' time and bytes go into `mine` as well (the
    variant driver's stage times have the two keys, the polish driver's do not); they are reset either way.  candidates: the
    handle enumerates candidates where PEPPER_AMD_DEVICE_CANDIDATES says, and its calls are counted by where they ran."""
    sampled_before, long_before = enc.sampled()[0], enc.long_cigar_reads
    if candidates:
        enc.set_device_candidates(_lib.device_candidates())
        calls_before = enc.candidate_calls()
    failed = True
    try:
        yield
        failed = False
    finally:
        if not failed or release_on_error:
            if inflate_figures and enc.inflated_bytes:
                mine["inflate_kernel"] = mine.get("inflate_kernel", 0.0) + enc.inflate_ms / 1e3
                mine["inflated_bytes"] = mine.get("inflated_bytes", 0.0) + enc.inflated_bytes
            enc.inflate_ms, enc.inflated_bytes = 0.0, 0
            mine["sampled_on_device"] += enc.sampled()[0] - sampled_before
            mine["long_cigar_reads_on_device"] += enc.long_cigar_reads - long_before
            if candidates:
                calls = enc.candidate_calls()
                mine["device_enumerated_calls"] += calls[0] - calls_before[0]
                mine["host_enumerated_calls"] += calls[1] - calls_before[1]
            enc.set_sampling(None)
            if candidates:
                enc.set_device_candidates(False)
            enc.release()


def generate_summary_arrays_batch(generators, reads_list, min_snp_baseq, min_indel_baseq, snp_freq_threshold,
                                  insert_freq_threshold, delete_freq_threshold, min_coverage_threshold,
                                  snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                                  candidate_support_threshold, skip_indels, candidate_regions, candidate_window_size,
                                  feature_size, train_mode=False, want_int32=False):
    """Many regions through one set of launches (pa_encoder_generate_summary_batch): generators[i] with reads_list[i]
    (type_read-like objects or the flat arrays of flatten_reads) and candidate_regions[i] = (start, end); the other
    arguments are those of RegionalSummaryGenerator.generate_summary.  -> one dict of arrays per region."""
    if train_mode:
        raise NotImplementedError("train_mode label generation (truth VCF haplotypes) is outside the inference path")
    batch = StagedBatch(generators, reads_list,
                        (min_snp_baseq, min_indel_baseq, snp_freq_threshold, insert_freq_threshold, delete_freq_threshold,
                         min_coverage_threshold, snp_candidate_freq_threshold, indel_candidate_freq_threshold,
                         candidate_support_threshold, skip_indels), candidate_regions, candidate_window_size, feature_size)
    batch.run()
    return batch.results(want_int32)
