"""Image generation driver (pileup -> images HDF5), inference mode.

Mirrors /root/reference/pepper_variant/modules/python/ImageGenerationUI.py:18-71 (ImageGenerator),
:79-91 (handle_output_directory), :93-96 (natural_key), :141-176 (region string parsing),
:191-274 (generate_image_and_save_to_file), :277-345 (generate_images): the genome is cut into
`options.region_size` intervals, interval i belongs to worker i % options.threads, every worker
writes one `pepper_variants_images_thread_<id>_<time>.hdf5` with one summaries/<chr>_<start>_<end>
group per interval that produced candidates.  BAM/FASTA access goes through `options.bam_handler_factory`
/ `options.fasta_handler_factory` (callables path -> handler object with the reference's handler
methods); reading BAM/FASTA files needs htslib and is the "next" row N3, so without factories this
raises.  Workers run sequentially in-process (one GPU encoder), not in a ProcessPoolExecutor.
"""
import contextlib
import os
import re
import sys
import time
from datetime import datetime

import numpy as np

from pepper_amd.variant import Coverage, RefConfidence, Targets
from pepper_amd.variant.AlignmentSummarizer import AlignmentSummarizer
from pepper_amd.variant.DataStore import DataStore


def _log(msg):
    sys.stderr.write("[" + datetime.now().strftime('%m-%d-%Y %H:%M:%S') + "] " + msg + "\n")
    sys.stderr.flush()


def _on_device(options, device):
    """`options` as the host-clipped form reads them, with .device = this worker's device."""
    if int(getattr(options, "device", 0) or 0) == device:
        return options
    import copy
    clone = copy.copy(options)
    clone.device = device
    return clone


def worker_device(options, process_id):
    """The device of image-generation worker `process_id`: options.image_device_ids ("0,1,...", a list) or -- what call_variant's
    callers already give for the inference step -- options.device_ids, dealt round robin; options.device (default 0) without them.
    The reference's image generation is CPU work (ImageGenerationUI.py:326-339 starts one process per thread); its run_inference
    deals callers over device_ids the same way (RunInference.py:101-116)."""
    ids = getattr(options, "image_device_ids", None)
    if ids in (None, ""):
        ids = getattr(options, "device_ids", None)
    if ids in (None, ""):
        return int(getattr(options, "device", 0) or 0)
    if isinstance(ids, str):
        ids = [int(d) for d in ids.split(",") if d.strip() != ""]
    elif isinstance(ids, int):
        ids = [ids]
    ids = [int(d) for d in ids]
    return ids[process_id % len(ids)] if ids else 0


def _handlers(options, bam_path, fasta_path):
    """Injected factories win (tests, other readers); otherwise the package's own BAM (zlib, bamio.cpp) and
    indexed-FASTA readers -- htslib is not needed."""
    bf = getattr(options, "bam_handler_factory", None)
    ff = getattr(options, "fasta_handler_factory", None)
    if bf is None:
        from pepper_amd.variant.bam import BAM_handler as bf
    if ff is None:
        from pepper_amd.variant.fasta import FASTA_handler as ff
    return bf(bam_path), ff(fasta_path)


def _live_rows(probs, outs, live):
    """The probabilities of a call's rows without those of intervals that have no read (which write nothing)."""
    keep, at = [], 0
    for out, n_reads in zip(outs, live):
        k = len(out["positions"])
        if n_reads > 0:
            keep.append(probs[at:at + k])
        at += k
    return np.concatenate(keep) if keep else probs[:0]


class ImageGenerator:
    def __init__(self, chromosome_name, bam_file_path, fasta_file_path, options=None):
        self.bam_handler, self.fasta_handler = _handlers(options, bam_file_path, fasta_file_path)
        self.chromosome_name = chromosome_name

    def generate_summary(self, options, start_position, end_position, bed_list, thread_id, as_arrays=False):
        if getattr(options, "use_hp_info", False):
            raise NotImplementedError("--use_hp_info image generation feeds a predictor that is non-functional "
                                      "in the reference at this commit (SURVEY.md 2.1 V13)")
        summarizer = AlignmentSummarizer(self.bam_handler, self.fasta_handler, self.chromosome_name,
                                         start_position, end_position)
        return summarizer.create_summary(options, bed_list, thread_id, as_arrays=as_arrays)

    def prepare(self, options, start_position, end_position):
        """The part of generate_summary in front of the encoder call (reads + reference of the interval), for the callers
        that encode several intervals per call."""
        if getattr(options, "use_hp_info", False):
            raise NotImplementedError("--use_hp_info image generation feeds a predictor that is non-functional "
                                      "in the reference at this commit (SURVEY.md 2.1 V13)")
        return AlignmentSummarizer(self.bam_handler, self.fasta_handler, self.chromosome_name, start_position,
                                   end_position).prepare(options)


class ImageGenerationUtils:
    @staticmethod
    def handle_output_directory(output_dir):
        if not os.path.exists(output_dir):
            os.makedirs(output_dir, exist_ok=True)
        if output_dir[-1] != '/':
            output_dir += '/'
        return output_dir

    @staticmethod
    def natural_key(string_):
        return [int(s) if s.isdigit() else s for s in re.split(r'(\d+)', string_)]

    @staticmethod
    def get_chromosome_list(chromosome_names, fasta_handler, bam_handler):
        """'chr20', 'chr20:1000-2000', 'chr1-3' or a comma list -> [(name, region or None)];
        empty -> contigs common to BAM and FASTA in natural order."""
        if not chromosome_names:
            common = sorted(set(fasta_handler.get_chromosome_names()) & set(bam_handler.get_chromosome_sequence_names()),
                            key=ImageGenerationUtils.natural_key)
            if not common:
                raise RuntimeError("ERROR: NO COMMON CONTIGS FOUND BETWEEN THE BAM FILE AND THE FASTA FILE.")
            return [(c, None) for c in common]
        out = []
        for name in [n.strip() for n in chromosome_names.strip().split(',')]:
            region = None
            if ':' in name:
                parts = name.split(':')
                if len(parts) != 2:
                    raise ValueError("ERROR: --region INVALID value.")
                name, region = parts
                region = [int(p) for p in region.strip().split('-')]
                if len(region) != 2 or not region[0] <= region[1]:
                    raise ValueError("ERROR: --region INVALID value.")
            range_split = name.split('-')
            if len(range_split) > 1:
                prefix = ''
                for ch in name:
                    if ch.isdigit():
                        break
                    prefix += ch
                ints = sorted(int(''.join(c for c in item if c.isdigit())) for item in range_split)
                for k in range(ints[0], ints[-1] + 1):
                    out.append((prefix + str(k), region))
            else:
                out.append((name, region))
        return out

    @staticmethod
    def split_intervals(chr_list, fasta_handler, region_size):
        """generate_images:289-317: [(chr, pos_start, pos_end)] of at most region_size bases."""
        all_intervals, total_bases = [], 0
        for chr_name, region in chr_list:
            last = fasta_handler.get_chromosome_sequence_length(chr_name) - 1
            if not region:
                interval_start, interval_end = 0, last
            else:
                interval_start, interval_end = max(0, region[0]), min(region[1], last)
            for pos in range(interval_start, interval_end, region_size):
                pos_start, pos_end = max(interval_start, pos), min(interval_end, pos + region_size)
                all_intervals.append((chr_name, pos_start, pos_end))
                total_bases += pos_end - pos_start
        return all_intervals, total_bases

    @staticmethod
    def generate_image_and_save_to_file(options, all_intervals, bed_list, process_id):
        timestr = time.strftime("%m%d%Y_%H%M%S")
        file_name = options.image_output_directory + "pepper_variants_images_thread_" + str(process_id) + "_" + str(timestr) + ".hdf5"
        # intervals are encoded ENCODER_BATCH at a time: the reads of a group are fetched (BAM reader, outside the GIL), then one
        # encoder call covers the group; summaries are written per interval under the reference's group names.  A worker takes
        # whole groups of CONSECUTIVE intervals (the reference deals single intervals round robin, ImageGenerationUI.py:262-274;
        # which worker's file an interval lands in is not read by anything downstream): the reads of an interval start up to
        # a read length + 16 kb (the BAM index's window) in front of it, so consecutive fetches through one handle find most of
        # their BGZF blocks already inflated in the handle's cache -- the BAM reader is 93 % of this loop's time.
        device = worker_device(options, process_id)
        wopts = _on_device(options, device)          # (what the host-clipped form reads .device from)
        batch = max(1, int(getattr(options, "encoder_batch", 0) or os.environ.get("PEPPER_AMD_ENCODER_BATCH", 16)))
        # a worker takes whole runs of consecutive intervals; large jobs are cut so that every worker gets several runs
        run = max(1, min(batch, -(-len(all_intervals) // max(1, options.threads * 4))))
        intervals = [r for i, r in enumerate(all_intervals) if (i // run) % options.threads == process_id]
        if process_id == 0:
            _log("INFO: STARTING PROCESS: " + str(process_id) + " FOR " + str(len(intervals)) + " INTERVALS")
        from pepper_amd.variant.AlignmentSummarizer import create_summaries, targets_of
        from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder, adjacent_run, merge_stats, worker_counters
        generators = {}
        stats = getattr(options, "stage_seconds", None)      # a dict the caller wants the stage times of this worker added to
        # ... and two counts: intervals the device sampled down, intervals that took the host-clipped form for any reason
        # ... and the encoder calls of the packed form (one per group of intervals), with those whose candidates were enumerated
        # on the device / handed back to the host (both 0 unless PEPPER_AMD_DEVICE_CANDIDATES=1), and those whose read and pair
        # tables were built on the device (PEPPER_AMD_DEVICE_PACK=1) / on the host
        # ... and, in a fused run with device_selection, the encoder calls whose candidates were selected on the device (one
        # segment per call, pepper_amd/variant/fused.py: forward_select) / the calls and host-clipped groups selected the host way
        # ... and, with options.region_bed (bed_list: its tables, Targets.read_bed), the encoder calls of either form that ran
        # with a contig's targets set (the intervals the planner dropped are counted by generate_images)
        mine = {"sampled_on_device": 0, "host_form_intervals": 0, "long_cigar_reads_on_device": 0,
                "encoder_calls": 0, "device_enumerated_calls": 0, "host_enumerated_calls": 0,
                "device_packed_calls": 0, "host_packed_calls": 0, "device_selected_calls": 0, "host_selected_calls": 0,
                "target_calls": 0}

        # ... and, with options.coverage_bed (track: the job's Coverage.CoverageTrack), the encoder calls of either form that
        # ran with depth bins set, the depth runs they reported and the calls whose runs outgrew the device's buffer
        track = getattr(options, "coverage_track", None)
        if track is not None:
            mine.update(coverage_calls=0, coverage_runs=0, coverage_overflows=0)

        # ... and, with options.gvcf (gtrack: the job's RefConfidence.BlockTrack), the encoder calls of either form that ran with
        # a reference-confidence table set, the block records they reported, the calls whose records outgrew the device's
        # buffer and the event time of the block kernels
        gtrack = getattr(options, "gvcf_track", None)
        if gtrack is not None:
            mine.update(gvcf_calls=0, gvcf_records=0, gvcf_overflows=0, gvcf_kernel_ms=0.0)

        def lap(key, t0):
            now = time.perf_counter()
            mine[key] = mine.get(key, 0.0) + now - t0
            return now

        def collect(source, group, into, fetch):
            """The records of the encoder call that covered `group`, interval by interval into a track -> their number.  source:
            the PackedEncoder, or what thread_depth_bins / thread_ref_confidence yield; fetch(source, n) -> (the records, their
            region first, and None or the (bases, sums) of the n intervals)."""
            (region, *cols), totals = fetch(source, len(group))
            cut = np.searchsorted(region, np.arange(len(group) + 1))          # (the records come in region order)
            for r, (chr_name, _start, _end) in enumerate(group):
                a, b = int(cut[r]), int(cut[r + 1])
                into.add(chr_name, (_start, _end), tuple(c[a:b] for c in cols), *([] if totals is None else [(totals[0][r], totals[1][r])]))
            return len(region)

        def collect_depth(source, group):
            mine["coverage_runs"] += collect(source, group, track, lambda s, n: (s.depth_runs(), s.depth_totals(n)))

        def collect_blocks(source, group):
            """(the gVCF's track merges the records of a run that crossed a tile border)"""
            mine["gvcf_records"] += collect(source, group, gtrack, lambda s, n: (s.ref_blocks(), None))
            mine["gvcf_kernel_ms"] += source.ref_blocks_ms()

        def empty_on_target(chr_name, _start, _end):
            """An interval without a read is never encoded by the host-clipped form: every position of it has depth 0 and GQ 0.
            -> which of them lie inside a target (None: no BED, all)."""
            if bed_list is None:
                return None
            return Targets.contains(*Targets.table(bed_list, chr_name), np.arange(_start, _end + 1, dtype=np.int64))

        @contextlib.contextmanager
        def counting(prefix, calls, switch_off=None):
            """While the block runs: the encoder calls made with a track's setting and those among them whose records outgrew
            the buffer (calls() -> both, since the handle was created) into `mine`; behind it the setting off the handle."""
            before = calls()
            yield
            after = calls()
            mine[prefix + "_calls"] += after[0] - before[0]
            mine[prefix + "_overflows"] += after[1] - before[1]
            if switch_off is not None:
                switch_off()

        def summaries_of(prepared, group):
            """create_summaries of one host-clipped call; with a track, under this thread's depth bins and collected, with a
            gVCF track under this thread's reference-confidence table likewise."""
            if track is None and gtrack is None:
                return create_summaries(prepared)
            from pepper_amd.variant.PEPPER_VARIANT import thread_depth_bins, thread_ref_confidence
            live = [g for g, p in zip(group, prepared) if p is not None]
            with contextlib.ExitStack() as stack:
                if track is not None:
                    depth = stack.enter_context(thread_depth_bins(track.bins, device))
                    stack.enter_context(counting("coverage", depth.depth_calls))
                if gtrack is not None:
                    conf = stack.enter_context(thread_ref_confidence(gtrack.table, gtrack.bands, device))
                    stack.enter_context(counting("gvcf", conf.ref_calls))
                outs = create_summaries(prepared)
                if live and track is not None:
                    collect_depth(depth, live)
                if live and gtrack is not None:
                    collect_blocks(conf, live)
            for (chr_name, _start, _end), p in zip(group, prepared):
                if p is None and track is not None:
                    zeros, on_target = np.zeros(_end - _start + 1, np.int64), empty_on_target(chr_name, _start, _end)
                    track.add(chr_name, (_start, _end), Coverage.runs_numpy(zeros, _start, track.bins, on_target),
                              Coverage.totals_numpy(zeros, track.bins, on_target))
                if p is None and gtrack is not None:
                    gtrack.add_empty(chr_name, (_start, _end), empty_on_target(chr_name, _start, _end))
            return outs

        sink = getattr(options, "fused_sink", None)         # call_variant's fused form: predictions straight from the encoder's windows
        # ... with the selection on the device behind the model: segments instead of probabilities, and neither HDF5 file unless
        # options.keep_images / options.keep_predictions ask for them
        selecting = sink is not None and sink.device_selection
        keep_images = not selecting or bool(getattr(options, "keep_images", False))
        keep_predictions = sink is not None and sink.keep_predictions

        def write(output_hdf_file, chr_name, _start, _end, out, probs=None, selected=False):
            """selected: the interval's call has been through the model and the selection already (probs None: and nobody wants
            its probabilities)."""
            n = len(out["candidates"])
            if sink is not None:
                if probs is None and not selected:
                    probs = sink.forward_host(device, out["images"])
                    if selecting:                        # a host-clipped interval: selected the present way
                        sink.select_host(chr_name, [out], probs)
                if probs is not None:
                    sink.submit(chr_name, out, probs)
            if output_hdf_file is None:
                return
            summary_name = chr_name + "_" + str(_start) + "_" + str(_end)
            if output_hdf_file.write_summary_packed(summary_name, chr_name, out):
                return
            output_hdf_file.write_summary(summary_name, [chr_name] * n, out["positions"], out["depths"],
                                          np.array(out["candidates"], dtype=object).reshape(n, 1),
                                          out["candidate_frequency"].reshape(n, 1), out["images"],
                                          [0] * n, [0] * n, False)

        def host_clipped(output_hdf_file, group):
            """The form in which the host clips every read to its interval (BAM_handler.get_reads): injected handlers,
            operations the device-side clip refuses, intervals whose reads outgrow the arena (and, under
            PEPPER_AMD_DEVICE_SAMPLING=0, intervals whose reads are sampled down)."""
            prepared = []
            mine["host_form_intervals"] += len(group)
            for chr_name, _start, _end in group:
                if chr_name not in generators:
                    generators.clear()               # one contig's handles at a time per worker
                    generators[chr_name] = ImageGenerator(chr_name, options.bam, options.fasta, wopts)
                prepared.append(generators[chr_name].prepare(wopts, _start, _end))
            t0 = time.perf_counter()
            if bed_list is None:
                summaries = summaries_of(prepared, group)
            else:
                # one encoder call per run of one contig, with that contig's targets on this thread's handle for its duration
                summaries, k0 = [], 0
                while k0 < len(group):
                    k1 = k0 + 1
                    while k1 < len(group) and group[k1][0] == group[k0][0]:
                        k1 += 1
                    with targets_of(bed_list, group[k0][0], device):
                        summaries += summaries_of(prepared[k0:k1], group[k0:k1])
                    mine["target_calls"] += 1 if any(p is not None for p in prepared[k0:k1]) else 0
                    k0 = k1
            for (chr_name, _start, _end), out in zip(group, summaries):
                if out is not None:
                    write(output_hdf_file, chr_name, _start, _end, out)
            if selecting:
                mine["host_selected_calls"] += 1
                lap("fused_select", t0)

        packed = (getattr(options, "bam_handler_factory", None) is None and getattr(options, "fasta_handler_factory", None) is None
                  and os.environ.get("PEPPER_AMD_PACKED_READS", "1") != "0" and not getattr(options, "train_mode", False))
        if getattr(options, "use_hp_info", False):
            packed = False                           # (host_clipped raises the reference's message for it)
        with (DataStore(file_name, 'w') if keep_images else contextlib.nullcontext()) as output_hdf_file:
            if not packed:
                for g0 in range(0, len(intervals), batch):
                    host_clipped(output_hdf_file, intervals[g0:g0 + batch])
                merge_stats(stats, mine)
                return process_id
            # The packed form: per group of consecutive intervals ONE call of the BAM reader (inflate, header walk, filters; no
            # clipping, no decoding: the reads cross PCIe as BAM stores them, once per group) and ONE of the encoder (clip +
            # decode + summary + windows on the device); both run outside the GIL, each worker on its own handles.
            from pepper_amd import _lib
            from pepper_amd.variant.AlignmentSummarizer import AlingerOptions, ConsensCandidateFinder
            from pepper_amd.variant.Options import ImageSizeOptions
            t_setup = time.perf_counter()
            # (every CPU the process has is inflating BGZF blocks in some worker: the encoder's host part runs on this thread)
            try:
                enc = PackedEncoder.acquire(device, int(os.environ.get("PEPPER_AMD_ARENA_MB", 256)) << 20, host_threads=1)
            except _lib.PepperAmdError:
                # no page-locked arena to be had (memlock / cgroup limit): the host-clipped form needs none
                for g0 in range(0, len(intervals), batch):
                    host_clipped(output_hdf_file, intervals[g0:g0 + batch])
                merge_stats(stats, mine)
                return process_id
            bam_handler, fasta_handler = _handlers(options, options.bam, options.fasta)
            lap("setup", t_setup)
            safe = ConsensCandidateFinder.REGION_SAFE_BASES
            params = (options.min_snp_baseq, options.min_indel_baseq, options.snp_frequency, options.insert_frequency,
                      options.delete_frequency, options.min_coverage_threshold, options.snp_candidate_frequency_threshold,
                      options.indel_candidate_frequency_threshold, options.candidate_support_threshold, options.skip_indels)
            # the BGZF members inflated on the device where the BAM has an index (PEPPER_AMD_DEVICE_INFLATE=0: on the host)
            device_inflate = _lib.device_inflate()
            # the reference samples an interval's reads down to min(MAX_READS_IN_REGION, downsample_rate * n)
            # (AlignmentSummarizer.py:192-199) in read order: drawn on the device between the clip and the summary
            # (reservoir_keep_kernel); PEPPER_AMD_DEVICE_SAMPLING=0: such intervals take the host-clipped form
            device_sampling = _lib.device_sampling()
            sampling = ((AlingerOptions.RANDOM_SEED, AlingerOptions.MAX_READS_IN_REGION, float(options.downsample_rate))
                        if device_sampling else None)
            # a read whose CIGAR travels in the CG tag stays in the span inflated on the device (operations from the tag, bases
            # from the core); PEPPER_AMD_DEVICE_LONG_CIGARS=0: its group of intervals takes the host packer
            long_cigars = _lib.device_long_cigars()
            # the read and pair tables built behind the device's record walk (pa_encoder_pack_records): the lap bam_walk_device
            # is then walk + pack with their one wait, and bam_walk only the spans the device handed back
            device_pack = _lib.device_pack()
            # what the encoder counts while this worker runs goes into `mine`; candidates enumerated between the count kernels
            # and the window gather where PEPPER_AMD_DEVICE_CANDIDATES=1 (pa_encoder_set_device_candidates).  A worker that
            # raises leaves its handle out of the pool
            # The job's bins and reference-confidence table on the handle while this worker runs: it goes back to the pool without them
            with worker_counters(enc, mine, release_on_error=False, inflate_figures=True, candidates=True), contextlib.ExitStack() as stack:
                g0 = 0
                if track is not None:
                    enc.set_depth_bins(track.bins)
                    stack.enter_context(counting("coverage", enc.depth_calls, lambda: enc.set_depth_bins(None)))
                if gtrack is not None:
                    enc.set_ref_confidence(gtrack.table, gtrack.bands)
                    stack.enter_context(counting("gvcf", enc.ref_calls, lambda: enc.set_ref_confidence(None, None)))
                while g0 < len(intervals):
                    group = intervals[g0:adjacent_run(intervals, g0, batch, 2 * safe)]
                    chr_name = group[0][0]
                    regions = [(max(0, s - safe), e + safe) for _, s, e in group]
                    # a batch the device form cannot take (pack_device's docstring) goes through the host packer; bam_pack is the
                    # host packer's time alone (lap_resident=False: what the device form takes is in its own laps)
                    resident, n_done, region_pairs, counts = enc.fetch(
                        bam_handler, chr_name, [r[0] for r in regions], [r[1] for r in regions], options.include_supplementary,
                        options.min_mapq, device_inflate, mine, lap_resident=False, long_cigars=long_cigars, device_pack=device_pack)
                    t0 = time.perf_counter()
                    if n_done == 0:
                        host_clipped(output_hdf_file, group[:1])
                        g0 += 1
                        continue
                    group, regions = group[:n_done], regions[:n_done]
                    per_region = np.diff(region_pairs[:n_done + 1])
                    if not device_sampling and (options.downsample_rate < 1.0
                                                or int(per_region.max(initial=0)) > AlingerOptions.MAX_READS_IN_REGION):
                        host_clipped(output_hdf_file, group)
                        g0 += n_done
                        continue
                    # one fetch for the group's whole stretch of the contig (adjacent intervals), sliced per interval
                    lo, hi = regions[0][0], max(b for _, b in regions) + 1
                    whole = fasta_handler.get_reference_bytes(chr_name, lo, hi)
                    references = [whole[a - lo:b + 1 - lo] for a, b in regions]
                    t0 = lap("fasta", t0)
                    # (the lean form of device_selection fetches no list and no image: outs are then the counts per interval)
                    fetch = keep_images or keep_predictions
                    if bed_list is not None:             # (sent when the contig changes: a worker's groups are runs of one contig)
                        enc.set_targets(Targets.table(bed_list, chr_name), chr_name)
                    try:
                        outs, live = enc.encode(regions, references, region_pairs, counts, params, [(s, e) for _, s, e in group],
                                                ImageSizeOptions.CANDIDATE_WINDOW_SIZE, ImageSizeOptions.IMAGE_HEIGHT, resident=resident,
                                                sampling=sampling, fetch=fetch)
                    except _lib.PepperAmdError as err:
                        if getattr(err, "code", 0) != _lib.PA_ERR_UNSUPPORTED:
                            raise
                        host_clipped(output_hdf_file, group)
                        g0 += n_done
                        continue
                    if track is not None:
                        collect_depth(enc, group)
                    if gtrack is not None:
                        collect_blocks(enc, group)
                    t0 = lap("encode", t0)
                    mine["encoder_calls"] += 1
                    mine["target_calls"] += 1 if bed_list is not None else 0
                    mine["device_packed_calls" if (resident and enc.device_packed) else "host_packed_calls"] += 1
                    probs, at = None, 0
                    if selecting:
                        # model and selection back to back on the device; what comes back is the call's segment
                        per_interval = [len(o["positions"]) for o in outs] if fetch else [int(k) for k in outs]
                        total = sum(per_interval)
                        if any(k > 0 and n_reads <= 0 for k, n_reads in zip(per_interval, live)):
                            raise RuntimeError("fused device selection: candidates in an interval without reads")
                        segment, probs = sink.forward_select(device, enc, total, chr_name, want_probs=keep_predictions)
                        if segment is None:              # handed back: this call the present way
                            if not fetch:
                                outs = enc.last.results()
                            sink.select_host(chr_name, [o for o, n_reads in zip(outs, live) if n_reads > 0], _live_rows(probs, outs, live))
                            mine["host_selected_calls"] += 1
                        else:
                            sink.add_segment(segment)
                            mine["device_selected_calls"] += 1
                            # rows the device looked at / kept, and the bytes of the kept rows that came back
                            mine["device_selection_rows"] = mine.get("device_selection_rows", 0) + total
                            mine["device_selection_kept"] = mine.get("device_selection_kept", 0) + len(segment)
                            mine["device_selection_bytes"] = mine.get("device_selection_bytes", 0) + getattr(segment, "downloaded_bytes", 0)
                        t0 = lap("fused_select", t0)
                        if not fetch:
                            g0 += n_done
                            continue
                    elif sink is not None:
                        # the group's windows are still where the encoder left them on the device: the model reads them there
                        total = sum(len(o["positions"]) for o in outs)
                        probs = sink.forward_device(device, enc.lib.pa_encoder_device_images(enc.enc), total)
                        t0 = lap("fused_forward", t0)
                    for (chr_name, _start, _end), out, n_reads in zip(group, outs, live):
                        k = len(out["positions"])
                        if n_reads > 0:                  # (no read with a base inside, or an empty sample: create_summary returns None, nothing is written)
                            write(output_hdf_file, chr_name, _start, _end, out, None if probs is None else probs[at:at + k], selected=selecting)
                        at += k
                    lap("hdf5", t0)
                    g0 += n_done
            t_close = time.perf_counter()
        lap("close", t_close)
        merge_stats(stats, mine)
        return process_id

    @staticmethod
    def generate_images(options):
        options.image_output_directory = ImageGenerationUtils.handle_output_directory(
            os.path.abspath(options.image_output_directory))
        start_time = time.time()
        bam_handler, fasta_handler = _handlers(options, options.bam, options.fasta)
        chr_list = ImageGenerationUtils.get_chromosome_list(options.region, fasta_handler, bam_handler)
        all_intervals, total_bases = ImageGenerationUtils.split_intervals(chr_list, fasta_handler, options.region_size)
        _log("INFO: TOTAL CONTIGS: " + str(len(chr_list)) + " TOTAL INTERVALS: " + str(len(all_intervals))
             + " TOTAL BASES: " + str(total_bases))
        # options.region_bed: candidates only inside the BED's intervals (the reference parses the file and reads the list
        # while training only).  The intervals stay on split_intervals' grid; one without a target position is never fetched
        bed_list = None
        region_bed = getattr(options, "region_bed", None)
        if region_bed:
            lengths = {name: fasta_handler.get_chromosome_sequence_length(name) for name in fasta_handler.get_chromosome_names()}
            bed_list = Targets.read_bed(region_bed, lengths, log=_log)
            all_intervals, dropped, dropped_bases = Targets.filter_intervals(all_intervals, bed_list)
            _log("INFO: REGION BED: " + str(dropped) + " INTERVALS (" + str(dropped_bases) + " BASES) WITHOUT A TARGET DROPPED, "
                 + str(len(all_intervals)) + " INTERVALS KEPT")
            from pepper_amd.variant.PEPPER_VARIANT import merge_stats
            merge_stats(getattr(options, "stage_seconds", None), {"target_intervals_dropped": dropped})
        # the reference forks options.threads processes; here they are threads of one process sharing the GPU: the
        # BAM reader, the encoder's host pass and libhdf5 run outside the GIL, each worker has its own BAM / FASTA
        # handles, encoder workspace and output file (interval i goes to worker i % threads, as in the reference)
        # options.coverage_bed (or PEPPER_AMD_COVERAGE_BED=1): the depth classes of every position the run looks at, reported by
        # the encoder beside its candidates and written as PEPPER_VARIANT_COVERAGE.bed (pepper_amd/variant/Coverage.py); the
        # workers find the track on the options while they run
        track = None
        if getattr(options, "coverage_bed", None) or os.environ.get("PEPPER_AMD_COVERAGE_BED") == "1":
            bins, labels = Coverage.parse_bins(getattr(options, "coverage_bins", None), options.min_coverage_threshold)
            track = Coverage.CoverageTrack(fasta_handler.get_chromosome_names(), bins, labels)
            options.coverage_track = track
        # options.gvcf (or PEPPER_AMD_GVCF=1): the reference blocks of every position the run looks at, reported by the encoder
        # beside its candidates (pepper_amd/variant/RefConfidence.py); the workers find the track on the options while they
        # run, call_variant finds it there afterwards and writes the gVCF behind step 3 (pepper_amd/variant/Gvcf.py)
        gtrack = None
        if getattr(options, "gvcf", None) or os.environ.get("PEPPER_AMD_GVCF") == "1":
            rate = getattr(options, "gvcf_error_rate", None)
            table = RefConfidence.build_table(RefConfidence.DEFAULT_ERROR_RATE if rate is None else rate)
            gtrack = RefConfidence.BlockTrack(fasta_handler.get_chromosome_names(), RefConfidence.parse_bands(getattr(options, "gvcf_bands", None)),
                                              table)
            options.gvcf_track = gtrack
        try:
            if options.threads <= 1:
                ImageGenerationUtils.generate_image_and_save_to_file(options, all_intervals, bed_list, 0)
            else:
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=options.threads) as pool:
                    futures = [pool.submit(ImageGenerationUtils.generate_image_and_save_to_file, options, all_intervals, bed_list,
                                           process_id) for process_id in range(options.threads)]
                    for fut in futures:
                        fut.result()
        finally:
            if track is not None:
                del options.coverage_track
            if gtrack is not None:
                del options.gvcf_track
        if track is not None:
            coverage_dir = getattr(options, "coverage_output_directory", None) or options.image_output_directory
            runs = track.write(ImageGenerationUtils.handle_output_directory(coverage_dir) + Coverage.BED_NAME)
            _log("INFO: " + track.log_line(runs))
        if gtrack is not None:
            _log("INFO: " + gtrack.log_line())
            take = getattr(options, "gvcf_take", None)       # call_variant's: it writes the gVCF behind step 3
            if take is not None:
                take(gtrack)
        _log("INFO: FINISHED IMAGE GENERATION")
        secs = int(time.time() - start_time)
        _log("INFO: TOTAL ELAPSED TIME FOR GENERATING IMAGES: " + str(secs // 60) + " Min " + str(secs % 60) + " Sec")
