"""`polish(bam, fasta, output_path, threads, region, model_path, batch_size, gpu_mode, device_ids, num_workers)`:
images -> consensus -> stitched FASTA (/root/reference/pepper/modules/python/polish.py:14-125).  The three steps are
the package's make_images / call_consensus / perform_stitch; argument checks raise instead of exiting."""
import os
import sys
import time
from datetime import datetime

from pepper_amd.polish.ImageGenerationUI import UserInterfaceSupport, parse_device_ids
from pepper_amd.polish.call_consensus import call_consensus
from pepper_amd.polish.make_images import make_images
from pepper_amd.polish.perform_stitch import perform_stitch


def _log(message):
    sys.stderr.write("[" + datetime.now().strftime('%m-%d-%Y %H:%M:%S') + "] " + message + "\n")
    sys.stderr.flush()


def polish(bam_filepath, fasta_filepath, output_path, threads, region, model_path, batch_size, gpu_mode, device_ids,
           num_workers, stage_walls=None, fused_inference=None, batch_invariant=None, downsample_rate=1.0, device_stitch=None,
           keep_predictions=None, qualities=None, edits=None, fill=None, min_quality=None, vcf=None):
    """The reference's ten arguments; stage_walls: a dict that receives the three steps' wall times; fused_inference (default:
    PEPPER_AMD_FUSED_POLISH=1): the image workers hand their chunks to the model on the device instead of call_consensus reading
    the image files back (pepper_amd/polish/fused.py); both stores are still written.  batch_invariant (default:
    PEPPER_AMD_BATCH_INVARIANT=1): the model handles of either form run in batch-invariant mode, so both forms, and any
    device_ids, give the same predictions bit for bit.  downsample_rate: make_images' (no effect on the output).
    device_stitch (default: PEPPER_AMD_DEVICE_STITCH=1): step 3 merges the predictions on the device
    (pepper_amd/polish/DeviceStitch.py) and writes the FASTA perform_stitch would; in the fused form the labels go from the model
    to the stitcher without leaving the device, and the prediction files are written only with keep_predictions (default: not).
    qualities (default: PEPPER_AMD_POLISH_QUALITIES=1): step 3 also writes <output>_pepper_polished.fastq, every base with the
    phred of the prediction row that supplied it as Sanger text, chr(33 + min(phred, 93)); the FASTA is the same either way.
    edits (default: PEPPER_AMD_POLISH_EDITS=1): step 3 also writes <output>_pepper_polished.edits.tsv, what the consensus changed
    against fasta_filepath hunk by hunk in both coordinate systems (pepper_amd/polish/Edits.py; not in the reference); in the
    fused device-stitch form the comparison runs on the device and the phred goes to the stitcher as with qualities
    (stage_walls["device_stitch_edits"]: the records, the bytes that came back, the seconds of the comparison and of the text).
    fill (default: PEPPER_AMD_POLISH_FILL=1): step 3 writes a COMPLETE consensus -- every contig merged as one piece, so the files
    do not depend on `threads`, the letters of fasta_filepath (as stored, quality '!') where no prediction covered a position, and
    without a region the contigs no prediction names, unchanged (perform_stitch(..., fill=, unpolished_contigs=); not in the
    reference).  In the device forms the filling runs on the device (stage_walls["device_stitch_fill"] in the fused form: the runs
    and letters filled, the seconds).
    min_quality (default: PEPPER_AMD_POLISH_MIN_QUALITY; an integer 1..255, 0 or None: off): step 3 applies only the edits against
    fasta_filepath whose winning prediction has phred >= min_quality -- a substitution or deletion below it keeps the draft's
    letter (upper-cased, quality '!'), an insertion below it is left out; positions whose draft letter is not ACGT are the model's
    (pepper_amd/polish/Stitch.py gate_numpy; not in the reference) -- and writes <output>_pepper_polished.withheld.tsv, the edits it
    kept back.  In the device forms the gate runs on the device (stage_walls["device_stitch_gate"] in the fused form: the edits
    withheld by kind, the bytes that came back, the seconds).
    vcf (default: PEPPER_AMD_POLISH_VCF=1; needs fill, ValueError before any work without it): step 3 also writes
    <output>_pepper_polished.vcf.gz and its .tbi -- one record per hunk of the filled consensus, trimmed and left-aligned against
    fasta_filepath, QUAL and GQ the lowest phred of the hunk, so that replaying the records over the draft gives the FASTA
    (pepper_amd/polish/Variants.py; not in the reference).  With min_quality it holds exactly the applied edits.  In the device
    forms the hunks are normalised on the device (stage_walls["device_stitch_vcf"] in the fused form: the records, no-ops,
    unanchored and shifted hunks, the bytes that came back, the seconds of the device call and of the text)."""
    from pepper_amd import _lib
    batch_invariant = _lib.batch_invariant_default(batch_invariant)
    if qualities is None:
        qualities = _lib.polish_qualities()
    qualities = bool(qualities)
    if edits is None:
        edits = _lib.polish_edits()
    draft_fasta = fasta_filepath if edits else None
    if fill is None:
        fill = _lib.polish_fill()
    fill_kw = dict(fill=fasta_filepath, unpolished_contigs=region is None) if fill else {}
    min_quality = _lib.min_quality_value(_lib.polish_min_quality() if min_quality is None else min_quality)
    if min_quality:
        fill_kw.update(min_quality=min_quality, draft=fasta_filepath)
    if vcf is None:
        vcf = _lib.polish_vcf()
    if vcf:
        if not fill:
            raise ValueError("vcf needs fill: the records describe one complete consensus per contig")
        fill_kw.update(vcf=fasta_filepath)
    for path, what in ((bam_filepath, "BAM"), (fasta_filepath, "FASTA"), (model_path, "MODEL")):
        if not os.path.isfile(path):
            raise FileNotFoundError("CAN NOT LOCATE " + what + " FILE: " + str(path))
    if threads <= 0:
        raise ValueError("THREAD NEEDS TO BE >=0.")
    if batch_size <= 0:
        raise ValueError("batch_size NEEDS TO BE >0.")
    if num_workers < 0:
        raise ValueError("num_workers NEEDS TO BE >=0.")
    if not gpu_mode:
        raise RuntimeError("pepper_amd has no CPU inference path: gpu_mode must be set")
    timestr = time.strftime("%m%d%Y_%H%M%S")
    output_dir = UserInterfaceSupport.handle_output_directory(output_path)
    image_output_directory = output_dir + "images_" + str(timestr) + "/"
    prediction_output_directory = output_dir + "predictions_" + str(timestr) + "/"
    _log("INFO: RUN-ID: " + str(timestr))
    _log("STEP 1: GENERATING IMAGES -> " + image_output_directory)
    image_stats = {} if stage_walls is not None else None       # the image workers' stage times, summed over the workers
    t0 = time.perf_counter()
    if fused_inference is None:
        fused_inference = os.environ.get("PEPPER_AMD_FUSED_POLISH") == "1"
    if device_stitch is None:
        device_stitch = _lib.device_stitch()
    stitcher = None
    if fused_inference:
        from pepper_amd.polish.fused import FusedConsensus
        UserInterfaceSupport.handle_output_directory(prediction_output_directory)
        _log("STEP 1+2: GENERATING IMAGES AND RUNNING INFERENCE (FUSED) -> " + prediction_output_directory)
        sink = FusedConsensus(model_path, prediction_output_directory, batch_invariant=batch_invariant, device_stitch=device_stitch,
                              keep_predictions=bool(keep_predictions) or not device_stitch,
                              stitch_device=parse_device_ids(device_ids)[0], qualities=qualities or bool(edits) or bool(min_quality) or bool(vcf))
        try:
            make_images(bam_filepath, fasta_filepath, region, image_output_directory, threads, device_ids=device_ids, fused=sink,
                        stats=image_stats, downsample_rate=downsample_rate)
        finally:
            sink.close()
        stitcher = sink.stitcher
        t1 = t2 = time.perf_counter()
    else:
        make_images(bam_filepath, fasta_filepath, region, image_output_directory, threads, device_ids=device_ids, stats=image_stats,
                    downsample_rate=downsample_rate)
        t1 = time.perf_counter()
        _log("STEP 2: RUNNING INFERENCE -> " + prediction_output_directory)
        call_consensus(image_output_directory, model_path, batch_size, num_workers, prediction_output_directory, device_ids,
                       gpu_mode, threads, batch_invariant=batch_invariant)
        t2 = time.perf_counter()
    _log("STEP 3: RUNNING STITCH -> " + output_dir)
    if not device_stitch:
        perform_stitch(prediction_output_directory, output_dir, threads, qualities=qualities, edits=draft_fasta, **fill_kw)
    elif not fused_inference:
        from pepper_amd.polish.DeviceStitch import stitch_directory
        stitch_directory(prediction_output_directory, output_dir, threads, device=parse_device_ids(device_ids)[0], qualities=qualities,
                         edits=draft_fasta, **fill_kw)
    elif stitcher is None and fill:          # (no chunk was predicted: the draft's contigs as they are, or nothing of a region)
        perform_stitch(prediction_output_directory, output_dir, threads, qualities=qualities, edits=draft_fasta, **fill_kw)
    elif stitcher is None:                   # (no chunk was predicted: perform_stitch over no files writes an empty FASTA)
        open(output_dir + '_pepper_polished.fa', 'w').close()
        if qualities:
            open(output_dir + '_pepper_polished.fastq', 'w').close()
        if edits:
            from pepper_amd.polish import Edits
            with open(Edits.edits_path(output_dir), 'w') as edits_file:
                edits_file.write(Edits.HEADER)
        if min_quality:                      # (nothing to gate: the header alone, as perform_stitch over no files writes it)
            from pepper_amd.polish import Edits
            with open(Edits.withheld_path(output_dir), 'w') as withheld_file:
                withheld_file.write(Edits.WITHHELD_HEADER)
    else:
        try:
            if qualities:
                stitcher.write_fastq(output_dir, threads, edits=draft_fasta, **fill_kw)
            else:
                stitcher.write_fasta(output_dir, threads, edits=draft_fasta, **fill_kw)
            if stage_walls is not None:
                stage_walls["device_stitch_stats"] = stitcher.stats()
                if edits:
                    stage_walls["device_stitch_edits"] = dict(stitcher.edit_totals)
                if fill:
                    stage_walls["device_stitch_fill"] = dict(stitcher.fill_totals)
                if min_quality:
                    stage_walls["device_stitch_gate"] = dict(stitcher.gate_totals)
                if vcf:
                    stage_walls["device_stitch_vcf"] = dict(stitcher.variant_totals)
        finally:
            stitcher.close()
    if stage_walls is not None:
        stage_walls.update(make_images=t1 - t0, call_consensus=t2 - t1, perform_stitch=time.perf_counter() - t2)
        stage_walls["image_stage_seconds_summed_over_workers"] = image_stats
