"""make_images -> run_inference -> find_candidates in one call.

replaces: /root/reference/pepper_variant/modules/python/CallVariant.py:12-109 (`call_variant`).
Same option names and the same three output locations (images_<run>/, predictions_<run>/, VCFs in
output_dir).  Input checks raise instead of calling exit().  `options.bam` / `options.fasta` are read by the package's
own readers (pepper_amd.variant.bam: BGZF members inflated on the device, records walked there;
pepper_amd.variant.fasta); `options.bam_handler_factory` / `options.fasta_handler_factory`, when given,
replace them (objects with the reference handlers' methods: tests inject synthetic read sets that way).
"""
import os
import sys
import time
from datetime import datetime

from pepper_amd.variant.FindCandidates import process_candidates
from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
from pepper_amd.variant.RunInference import run_inference


def _log(message):
    sys.stderr.write("[" + str(datetime.now().strftime('%m-%d-%Y %H:%M:%S')) + "] INFO: " + message + "\n")


def call_variant(options):
    start_time = time.time()
    if getattr(options, "bam_handler_factory", None) is None and not os.path.isfile(options.bam):
        raise FileNotFoundError("ERROR: CAN NOT LOCATE BAM FILE.")
    if getattr(options, "fasta_handler_factory", None) is None and not os.path.isfile(options.fasta):
        raise FileNotFoundError("ERROR: CAN NOT LOCATE FASTA FILE.")
    if not os.path.isfile(options.model_path):
        raise FileNotFoundError("ERROR: CAN NOT LOCATE MODEL FILE.")
    if options.threads <= 0:
        raise ValueError("ERROR: THREAD NEEDS TO BE >=0.")
    if options.batch_size <= 0:
        raise ValueError("ERROR: batch_size NEEDS TO BE >0.")
    if options.num_workers < 0:
        raise ValueError("ERROR: num_workers NEEDS TO BE >=0.")

    # options.haploid_contigs / options.par_regions_bed (pepper_amd/variant/Ploidy.py): read once, before any work, so that a
    # contig name the FASTA does not have stops the run here instead of calling it diploid
    from pepper_amd.variant import Ploidy
    Ploidy.of(options)

    timestr = time.strftime("%m%d%Y_%H%M%S")
    # batch-invariant mode (options.batch_invariant, default PEPPER_AMD_BATCH_INVARIANT): resolved once here, the options object
    # carries it to every handle of the run -- three-step or fused, the lanes' second handle, every process of device_ids
    from pepper_amd import _lib
    options.batch_invariant = _lib.batch_invariant_default(getattr(options, "batch_invariant", None))
    output_dir = ImageGenerationUtils.handle_output_directory(options.output_dir)
    image_output_directory = output_dir + "images_" + str(timestr) + "/"
    prediction_output_directory = output_dir + "predictions_" + str(timestr) + "/"
    candidate_output_directory = output_dir

    _log("RUN-ID: " + str(timestr))
    _log("IMAGE OUTPUT: " + str(image_output_directory))
    _log("STEP 1/3 GENERATING IMAGES:")
    options.image_output_directory = image_output_directory
    # (options.coverage_bed: image generation writes PEPPER_VARIANT_COVERAGE.bed beside the VCFs, not among the images)
    options.coverage_output_directory = output_dir
    # (options.gvcf: image generation hands the run's reference blocks over here; the gVCF is written behind step 3.  The
    # hook is taken off the options again before anything pickles them for another process)
    gvcf_tracks = []
    options.gvcf_take = gvcf_tracks.append
    walls = getattr(options, "stage_walls", None)           # a dict the caller wants the three steps' wall times in
    precomputed = None
    t0 = time.perf_counter()
    fused = bool(getattr(options, "fused_inference", False)) or os.environ.get("PEPPER_AMD_FUSED_CALL_VARIANT") == "1"
    # the candidate finder's selection on the device behind the model (options.device_selection / PEPPER_AMD_DEVICE_SELECTION=1;
    # DESIGN.md 4.13).  Its forms: fused + device_selection = lean (no image file, no prediction file, step 3 from the workers'
    # segments); + keep_images / keep_predictions = the files written as always beside it; without the fused run there is
    # nothing on the device to select from, and the switch is refused
    device_selection = bool(getattr(options, "device_selection", False)) or _lib.device_selection()
    if device_selection and not fused:
        raise ValueError("ERROR: device_selection (PEPPER_AMD_DEVICE_SELECTION=1) NEEDS fused_inference: THE THREE-STEP RUN SELECTS "
                         "FROM ITS PREDICTION FILES ON THE HOST.")
    options.device_selection = device_selection
    segments = None
    if fused:
        # opt-in: the encoder's windows go to the model where they lie on the device; both HDF5 files are still written
        # (pepper_amd/variant/fused.py).  Steps 1 and 2 are then one step.
        from pepper_amd.variant.fused import FusedPredictor
        os.makedirs(prediction_output_directory, exist_ok=True)
        _log("STEP 1+2/3 GENERATING IMAGES AND RUNNING INFERENCE (FUSED)")
        _log("OUTPUT: " + str(prediction_output_directory))
        options.fused_sink = FusedPredictor(options, prediction_output_directory)
        precomputed = None
        try:
            ImageGenerationUtils.generate_images(options)
        finally:
            del options.gvcf_take
            sink, options.fused_sink = options.fused_sink, None
            # (an image worker that raised: the predictions written so far are withdrawn, not published under the final name)
            sink.close(failed=sys.exc_info()[0] is not None)
            precomputed = sink.segments or None
            if device_selection:
                segments = sink.device_segments
            if walls is not None:
                walls["fused_writer_drain"] = getattr(sink, "drain_seconds", 0.0)
                walls["fused_forward_summed_over_handles"] = sink.forward_seconds
                walls["fused_writer_busy_summed"], walls["fused_selection_busy_summed"] = sink.write_seconds, sink.select_seconds
            if sink.select_error is not None:
                _log("INFO: THE FUSED RUN'S CANDIDATE SELECTION STOPPED (" + repr(sink.select_error) + "): STEP 3 DOES THE REST FROM THE FILE")
            if device_selection:
                _log("INFO: FUSED: " + str(len(sink.device_segments)) + " SEGMENTS SELECTED BEHIND THE MODEL")
            else:
                _log("INFO: FUSED: " + str(len(sink.segments)) + " OF " + str(sink.batch_no) + " BATCHES SELECTED AHEAD OF STEP 3")
        t1 = t2 = time.perf_counter()
    else:
        try:
            ImageGenerationUtils.generate_images(options)
        finally:
            del options.gvcf_take
        t1 = time.perf_counter()

        _log("STEP 2/3 RUNNING INFERENCE")
        _log("OUTPUT: " + str(prediction_output_directory))
        run_inference(options, image_output_directory, prediction_output_directory)
        t2 = time.perf_counter()

    _log("STEP 3/3 FINDING CANDIDATES")
    _log("OUTPUT: " + str(candidate_output_directory))
    totals = process_candidates(options, prediction_output_directory, candidate_output_directory,
                                precomputed=precomputed if fused else None, segments=segments)
    if gvcf_tracks:
        from pepper_amd.variant import Gvcf
        from pepper_amd.variant.fasta import FASTA_handler
        t3 = time.perf_counter()
        Gvcf.write_gvcf(candidate_output_directory + "PEPPER_VARIANT_FULL.vcf.gz", candidate_output_directory + Gvcf.GVCF_NAME,
                        gvcf_tracks[0], FASTA_handler(options.fasta), log=_log, ploidy=Ploidy.of(options))
        if walls is not None:
            walls["gvcf"] = time.perf_counter() - t3
    if walls is not None:
        walls.update(make_images=t1 - t0, run_inference=t2 - t1, find_candidates=time.perf_counter() - t2)

    elapsed = time.time() - start_time
    _log("TOTAL ELAPSED TIME FOR FINDING CANDIDATES: " + str(int(elapsed / 60)) + " Min " + str(int(elapsed) % 60) + " Sec")
    return image_output_directory, prediction_output_directory, totals
