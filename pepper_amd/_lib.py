"""ctypes binding of include/pepper_amd.h (the C-ABI drop-in boundary).

The product path has NO CPU fallback: if the HIP extension is missing or no gfx950 device is
visible, calls raise -- they never route through oracle/ or torch CPU ops.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpepper_amd.so")

PA_OK = 0

c_void_p, c_int32, c_int64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
c_char_p, c_double = ctypes.c_char_p, ctypes.c_double


class VariantConfig(ctypes.Structure):
    _fields_ = [("image_features", c_int32), ("window", c_int32), ("gru_layers", c_int32),
                ("num_classes_type", c_int32), ("device", c_int32), ("max_chunk", c_int32)]


class DevicePack(ctypes.Structure):
    """pa_device_pack (include/pepper_amd_encoder.h): the summary of pa_encoder_pack_records."""
    _fields_ = [("status", c_int32), ("n_done", c_int32), ("n_reads", c_int32), ("n_pairs", c_int32), ("n_split", c_int32),
                ("walk_flags", c_int32 * 2), ("reserved", c_int32), ("n_headers", c_int64), ("slice_bytes", c_int64),
                ("total_bases", c_int64), ("total_ops", c_int64)]


class SelectorRegion(ctypes.Structure):
    """pa_selector_region (include/pepper_amd_encoder.h)."""
    _fields_ = [("first_row", c_int64), ("reference_start", c_int64), ("reference", c_void_p), ("reference_len", c_int64)]


class Selection(ctypes.Structure):
    """pa_selection: the summary of pa_selector_run / pa_encoder_select_candidates."""
    _fields_ = [("kept_rows", c_int64), ("kept_name_bytes", c_int64), ("status", c_int32), ("reserved", c_int32)]


class PolishConfig(ctypes.Structure):
    _fields_ = [("image_features", c_int32), ("hidden_size", c_int32), ("gru_layers", c_int32),
                ("num_classes", c_int32), ("seq_length", c_int32), ("window", c_int32),
                ("jump", c_int32), ("overlap", c_int32), ("device", c_int32), ("max_chunk", c_int32)]


# (name, restype, argtypes) for every symbol include/pepper_amd.h declares
SYMBOLS = [
    ("pa_last_error", c_char_p, []),
    ("pa_version", c_char_p, []),
    ("pa_device_count", ctypes.c_int, []),
    ("pa_variant_create", ctypes.c_int, [ctypes.POINTER(VariantConfig), ctypes.POINTER(c_char_p),
                                         ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), c_int32,
                                         c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_variant_destroy", None, [c_void_p]),
    ("pa_variant_overflow_rows", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64)]),
    ("pa_variant_split_fallbacks", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64)]),
    ("pa_variant_set_batch_invariant", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_variant_get_batch_invariant", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int32)]),
    ("pa_variant_forward_device", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    ("pa_variant_forward_device_f32", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    ("pa_variant_forward_host", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    ("pa_polish_create", ctypes.c_int, [ctypes.POINTER(PolishConfig), ctypes.POINTER(c_char_p),
                                        ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), c_int32,
                                        c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_polish_destroy", None, [c_void_p]),
    ("pa_polish_forward_device", ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                                c_void_p, c_void_p]),
    ("pa_polish_predict_device", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_predict_host", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_predict_host_parts", ctypes.c_int, [c_void_p, ctypes.c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_set_batch_invariant", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_polish_get_batch_invariant", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int32)]),
    ("pa_profile_enable", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_profile_count", ctypes.c_int, [c_void_p]),
    ("pa_profile_get", ctypes.c_int, [c_void_p, c_int32, c_char_p, c_int32, ctypes.POINTER(c_double),
                                      ctypes.POINTER(c_int64), ctypes.POINTER(c_double)]),
    ("pa_synchronize", ctypes.c_int, [c_void_p]),
    ("pa_host_register", ctypes.c_int, [c_void_p, c_int64]),
    ("pa_host_unregister", ctypes.c_int, [c_void_p]),
    # include/pepper_amd_encoder.h (struct pointers passed as void*; typed structs live in
    # pepper_amd/variant/PEPPER_VARIANT.py)
    ("pa_encoder_create", ctypes.c_int, [c_int32, c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_encoder_destroy", None, [c_void_p]),
    ("pa_encoder_generate_summary", ctypes.c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    ("pa_encoder_generate_summary_batch", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("pa_encoder_stage_batch", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    ("pa_encoder_run_staged", ctypes.c_int, [c_void_p, c_void_p]),
    ("pa_encoder_host_arena", c_void_p, [c_void_p, c_int64]),
    ("pa_encoder_stage_packed", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32,
                                               c_void_p, c_void_p]),
    ("pa_encoder_host_span", c_void_p, [c_void_p, c_int64]),
    ("pa_encoder_inflate_bgzf", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                               c_void_p]),
    ("pa_encoder_walk_records", ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_int64,
                                               ctypes.POINTER(c_int64), c_void_p]),
    ("pa_encoder_submit_walk", ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int32, c_int32]),
    ("pa_encoder_walk_headers", ctypes.c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    ("pa_encoder_pack_records", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                               c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    ("pa_encoder_stage_packed_device", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    ("pa_encoder_packed_tables", ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    ("pa_encoder_pack_calls", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    ("pa_encoder_set_split_slices", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_encoder_set_seq_offsets", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_encoder_region_reads", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_encoder_set_host_threads", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_encoder_set_sampling", ctypes.c_int, [c_void_p, ctypes.c_uint32, c_int32, c_double]),
    ("pa_encoder_sampled_regions", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    ("pa_encoder_pair_live", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_encoder_set_device_candidates", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_encoder_candidate_calls", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    ("pa_encoder_set_targets", ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    ("pa_encoder_set_depth_bins", ctypes.c_int, [c_void_p, c_int32, c_void_p]),
    ("pa_encoder_depth_runs", ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int64)]),
    ("pa_encoder_depth_totals", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    ("pa_encoder_depth_calls", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    ("pa_encoder_set_ref_confidence", ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("pa_encoder_ref_blocks", ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             ctypes.POINTER(c_int64)]),
    ("pa_encoder_ref_calls", ctypes.c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    ("pa_encoder_last_timing", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_encoder_batch_stats", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_encoder_get_results", ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int64, ctypes.POINTER(c_int64)]),
    ("pa_encoder_device_images", c_void_p, [c_void_p]),
    ("pa_polish_encoder_generate_summary", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int64,
                                                          ctypes.POINTER(c_int64)]),
    ("pa_polish_encoder_generate_summary_batch", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_encoder_stage_batch", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_encoder_run_staged", ctypes.c_int, [c_void_p, c_void_p]),
    ("pa_polish_encoder_batch_stats", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_polish_encoder_get_results", ctypes.c_int, [c_void_p, c_void_p, c_void_p]),
    ("pa_polish_encoder_last_timing", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_polish_chain_run", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p,
                                           c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_chain_chunks", ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    ("pa_polish_chain_device_chunks", ctypes.c_int, [c_void_p, c_void_p]),
    ("pa_polish_chain_last_timing", ctypes.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32]),
    ("pa_stitcher_create", ctypes.c_int, [c_int32, c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_stitcher_destroy", None, [c_void_p]),
    ("pa_stitcher_limits", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_stitcher_add", ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                       c_void_p]),
    ("pa_stitcher_add_qual", ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                            c_void_p, c_void_p]),
    ("pa_stitcher_finish", ctypes.c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                          ctypes.POINTER(c_int64), ctypes.POINTER(c_int32)]),
    ("pa_stitcher_take", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_stitcher_take_qualities", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_stitcher_stats", ctypes.c_int, [c_void_p, c_void_p, c_int32]),
    ("pa_stitcher_edits", ctypes.c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    ("pa_stitcher_take_edits", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_stitcher_fill", ctypes.c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    ("pa_stitcher_gate", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    ("pa_stitcher_take_withheld", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_stitcher_variants", ctypes.c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    ("pa_stitcher_take_variants", ctypes.c_int, [c_void_p, c_void_p, c_int64]),
    ("pa_selector_create", ctypes.c_int, [c_int32, c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_selector_destroy", None, [c_void_p]),
    ("pa_selector_limits", ctypes.c_int, [c_void_p, c_int32]),
    ("pa_selector_run", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                       c_void_p, c_int32, c_void_p]),
    ("pa_selector_set_ploidy", ctypes.c_int, [c_void_p, c_int32, c_int64, c_void_p, c_void_p]),
    ("pa_selector_take", ctypes.c_int, [c_void_p] * 11),
    ("pa_encoder_select_candidates", ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # include/pepper_amd_realign.h
    ("pa_realigner_create", ctypes.c_int, [c_int32, c_void_p, ctypes.POINTER(c_void_p)]),
    ("pa_realigner_destroy", None, [c_void_p]),
    ("pa_realigner_align", ctypes.c_int, [c_void_p, c_char_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          ctypes.POINTER(c_int64)]),
    ("pa_realigner_align_windows", ctypes.c_int, [c_void_p, c_int32, c_char_p, c_void_p, c_void_p, c_int32] + [c_void_p] * 10 +
                                                  [ctypes.POINTER(c_int64)]),
    ("pa_realigner_copy_cigars", ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("pa_realigner_stage_ticks", ctypes.c_int, [c_void_p, c_void_p]),
    # include/pepper_amd_io_device.h
    ("pa_inflater_create", ctypes.c_int, [c_int32, ctypes.POINTER(c_void_p)]),
    ("pa_inflater_destroy", None, [c_void_p]),
    ("pa_inflater_inflate", ctypes.c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int64, c_int32]),
    ("pa_inflater_last_kernel_ms", ctypes.c_int, [c_void_p, ctypes.POINTER(c_double)]),
    ("pa_realigner_last_timing", ctypes.c_int, [c_void_p, ctypes.POINTER(c_double), ctypes.POINTER(c_double),
                                                ctypes.POINTER(c_int64)]),
]

_lib = None


class PepperAmdError(RuntimeError):
    pass


def load():
    """Load libpepper_amd.so (built in-tree by pepper_amd.build).  Fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PepperAmdError(
            f"{LIB_PATH} is missing: run `python -m pepper_amd.build` (hipcc --offload-arch=gfx950). "
            "pepper_amd has no CPU fallback.")
    # torch bundles its own libamdhip64 (SONAME libamdhip64.so.7, same as /opt/rocm's).  Import
    # torch FIRST so our NEEDED libamdhip64.so.7 resolves to the runtime torch already loaded;
    # the other order puts two HIP runtimes in one process and the second one sees no device.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


# include/pepper_amd.h:20-24
PA_ERR_INVALID = 1
PA_ERR_HIP = 2
PA_ERR_NO_DEVICE = 3
PA_ERR_UNSUPPORTED = 4


BATCH_INVARIANT_ENV = "PEPPER_AMD_BATCH_INVARIANT"


def parse_batch_invariant(value):
    """A batch_invariant option or the value of PEPPER_AMD_BATCH_INVARIANT -> bool.  None / "" -> False; accepts bools,
    0 / 1 and the words true / false, yes / no, on / off (any case); anything else is a ValueError."""
    if value is None or isinstance(value, bool):
        return bool(value)
    if isinstance(value, int):
        if value in (0, 1):
            return bool(value)
        raise ValueError(f"batch_invariant must be 0 or 1, got {value!r}")
    v = str(value).strip().lower()
    if v in ("", "0", "false", "no", "off"):
        return False
    if v in ("1", "true", "yes", "on"):
        return True
    raise ValueError(f"batch_invariant: cannot read {value!r} as on / off")


def batch_invariant_default(value=None):
    """What a new handle uses: `value` when given (not None), else the process-wide PEPPER_AMD_BATCH_INVARIANT."""
    if value is not None:
        return parse_batch_invariant(value)
    return parse_batch_invariant(os.environ.get(BATCH_INVARIANT_ENV))


def reservoir_sample(seed, n, k):
    """pa_reservoir_sample (include/pepper_amd_io.h; exported by the I/O library, bound in pepper_amd/variant/bam.py): the
    slots of the reference's reservoir sample of n reads down to k, as the device draws it."""
    from pepper_amd.variant import bam
    return bam.reservoir_sample(seed, n, k)


DEVICE_SAMPLING_ENV = "PEPPER_AMD_DEVICE_SAMPLING"


def device_sampling():
    """PEPPER_AMD_DEVICE_SAMPLING=0: the image-generation drivers send sampled intervals through their host forms again."""
    return os.environ.get(DEVICE_SAMPLING_ENV, "1") != "0"


DEVICE_LONG_CIGARS_ENV = "PEPPER_AMD_DEVICE_LONG_CIGARS"


def device_long_cigars():
    """PEPPER_AMD_DEVICE_LONG_CIGARS=0: the image-generation drivers send a batch with a CIGAR kept in the CG tag through the
    host packer again."""
    return os.environ.get(DEVICE_LONG_CIGARS_ENV, "1") != "0"


DEVICE_CANDIDATES_ENV = "PEPPER_AMD_DEVICE_CANDIDATES"


def device_candidates():
    """PEPPER_AMD_DEVICE_CANDIDATES=1: the image-generation drivers have their encoders enumerate candidates on the device
    (pa_encoder_set_device_candidates).  Unset or any other value: on the host."""
    return os.environ.get(DEVICE_CANDIDATES_ENV, "0") == "1"


DEVICE_PACK_ENV = "PEPPER_AMD_DEVICE_PACK"


def device_pack():
    """PEPPER_AMD_DEVICE_PACK=1: the variant image-generation driver has its encoders build the packed read and pair tables
    on the device (pa_encoder_pack_records).  Unset or any other value: on the host."""
    return os.environ.get(DEVICE_PACK_ENV, "0") == "1"


DEVICE_INFLATE_ENV = "PEPPER_AMD_DEVICE_INFLATE"


def device_inflate():
    """PEPPER_AMD_DEVICE_INFLATE=0: the image-generation drivers have the host packer inflate the BGZF members again
    (PackedEncoder.fetch goes straight to pack)."""
    return os.environ.get(DEVICE_INFLATE_ENV, "1") != "0"


DEVICE_WALK_ENV = "PEPPER_AMD_DEVICE_WALK"


def device_walk():
    """PEPPER_AMD_DEVICE_WALK=0: PackedEncoder.pack_device walks a downloaded copy of every inflated span on the host again.
    Read per call."""
    return os.environ.get(DEVICE_WALK_ENV, "1") != "0"


DEVICE_STITCH_ENV = "PEPPER_AMD_DEVICE_STITCH"


def device_stitch():
    """PEPPER_AMD_DEVICE_STITCH=1: polish() merges the predictions on the device (pa_stitcher_*; pepper_amd/polish/DeviceStitch.py)
    instead of perform_stitch on the host.  Unset or any other value: on the host."""
    return os.environ.get(DEVICE_STITCH_ENV, "0") == "1"


DEVICE_SELECTION_ENV = "PEPPER_AMD_DEVICE_SELECTION"


def device_selection():
    """PEPPER_AMD_DEVICE_SELECTION=1: the fused call_variant selects its candidates on the device (pa_selector_*;
    pepper_amd/variant/DeviceSelect.py) behind the model, and hands the host only the rows that end up in a VCF.  Unset or any
    other value: on the host (FastCandidates.native_batch_arrays over every row).  Needs fused_inference."""
    return os.environ.get(DEVICE_SELECTION_ENV, "0") == "1"


POLISH_QUALITIES_ENV = "PEPPER_AMD_POLISH_QUALITIES"


def polish_qualities():
    """PEPPER_AMD_POLISH_QUALITIES=1: polish() writes <prefix>_pepper_polished.fastq beside the FASTA, every base with the phred of
    the prediction row that supplied it.  Unset or any other value: the FASTA alone."""
    return os.environ.get(POLISH_QUALITIES_ENV, "0") == "1"


POLISH_EDITS_ENV = "PEPPER_AMD_POLISH_EDITS"


def polish_edits():
    """PEPPER_AMD_POLISH_EDITS=1: polish() writes <prefix>_pepper_polished.edits.tsv beside the FASTA: what the consensus changed
    against the draft (pepper_amd/polish/Edits.py).  Unset or any other value: the FASTA alone."""
    return os.environ.get(POLISH_EDITS_ENV, "0") == "1"


POLISH_FILL_ENV = "PEPPER_AMD_POLISH_FILL"


def polish_fill():
    """PEPPER_AMD_POLISH_FILL=1: polish() writes a complete consensus -- every contig merged as one piece, the draft's own letters
    where no prediction covered a position, and without a region the contigs no read landed on.  Unset or any other value: the
    reference's stitch, which leaves such sequence out."""
    return os.environ.get(POLISH_FILL_ENV, "0") == "1"


POLISH_VCF_ENV = "PEPPER_AMD_POLISH_VCF"


def polish_vcf():
    """PEPPER_AMD_POLISH_VCF=1: polish() writes <prefix>_pepper_polished.vcf.gz and its .tbi beside the FASTA: what the filled
    consensus changed against the draft, trimmed and left-aligned (pepper_amd/polish/Variants.py); needs fill.  Unset or any other
    value: no VCF."""
    return os.environ.get(POLISH_VCF_ENV, "0") == "1"


POLISH_MIN_QUALITY_ENV = "PEPPER_AMD_POLISH_MIN_QUALITY"


def min_quality_value(min_quality):
    """What every stitch form makes of its min_quality argument: None or 0 -> None (off), an integer 1..255 -> itself, anything
    else ValueError."""
    if min_quality is None:
        return None
    if isinstance(min_quality, bool) or int(min_quality) != min_quality or not 0 <= min_quality <= 255:
        raise ValueError("min_quality is an integer from 1 to 255 (0 or None: off), not %r" % (min_quality,))
    return int(min_quality) or None


def polish_min_quality():
    """PEPPER_AMD_POLISH_MIN_QUALITY=Q (1..255): polish() applies only the edits against the draft whose winning prediction has
    phred >= Q and keeps the draft's letter elsewhere (pepper_amd/polish/Stitch.py gate_numpy; <prefix>_pepper_polished.withheld.tsv
    lists what it kept back).  Unset, empty or 0: every label the model emits is applied.  Anything else: ValueError."""
    text = os.environ.get(POLISH_MIN_QUALITY_ENV, "").strip()
    if not text:
        return None
    try:
        value = int(text)
    except ValueError:
        raise ValueError(POLISH_MIN_QUALITY_ENV + " is an integer from 1 to 255 (0 or unset: off), not %r" % text)
    return min_quality_value(value)


def check(rc):
    if rc != PA_OK:
        msg = load().pa_last_error()
        err = PepperAmdError(f"pepper_amd error {rc}: {msg.decode() if msg else '?'}")
        err.code = rc
        raise err


def _as_numpy_f32(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v), dtype=np.float32)


def marshal_state_dict(state_dict):
    """-> (names[], data[], numel[], n, keepalive) for pa_*_create."""
    items = [(k, _as_numpy_f32(v)) for k, v in state_dict.items()]
    n = len(items)
    names = (c_char_p * n)(*[k.encode() for k, _ in items])
    data = (c_void_p * n)(*[a.ctypes.data for _, a in items])
    numel = (c_int64 * n)(*[a.size for _, a in items])
    return names, data, numel, n, items


def profile_dict(handle):
    """{label: {"ms": total_ms, "launches": n, "flops": total_flops}} for a model handle."""
    lib = load()
    out = {}
    count = lib.pa_profile_count(handle)
    if count < 0:
        check(1)
    buf = ctypes.create_string_buffer(64)
    for i in range(count):
        ms, launches, flops = c_double(), c_int64(), c_double()
        check(lib.pa_profile_get(handle, i, buf, 64, ctypes.byref(ms), ctypes.byref(launches),
                                 ctypes.byref(flops)))
        out[buf.value.decode()] = {"ms": ms.value, "launches": launches.value, "flops": flops.value}
    return out
