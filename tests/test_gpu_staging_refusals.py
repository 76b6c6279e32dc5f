"""What the three staging entry points refuse, and how: pa_encoder_stage_batch (host-clipped form), pa_encoder_stage_packed
(packed form) and pa_polish_chain_run (the polish chain's front end) each answer an input that breaks one rule with PA_ERR_INVALID
and a message that names the rule.  A refused variant staging leaves no staged batch, and the base offsets of
pa_encoder_set_seq_offsets serve exactly one staging call, accepted or refused.  One region of 100 rows, at most one read of 20
bases in a 256-byte arena: nearly every case is refused before a kernel is launched."""
import ctypes

import numpy as np
import pytest

from pepper_amd import _lib
from pepper_amd.variant.bam import PACKED_READ
from pepper_amd.variant.PEPPER_VARIANT import _PackedRegion, _Params, _Pileup

pytestmark = pytest.mark.gpu

START, END = 1000, 1099                     # 100 rows
REF = b"ACGT" * 25
L_SEQ, ARENA = 20, 256
SLICE = 4 + (L_SEQ + 1) // 2 + L_SEQ        # one CIGAR word | 4-bit bases | qualities
BASES = SLICE - 4


@pytest.fixture(scope="module")
def enc():
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.pa_encoder_create(0, None, ctypes.byref(h)))
    yield lib, h
    lib.pa_encoder_destroy(h)


def _params(n=1, window=(32, 32), feature=26):
    return (_Params * n)(*[_Params(1.0, 1.0, 0.1, 0.15, 0.15, 3.0, 0.1, 0.12, 2.0, 0, START, END, window[r], feature) for r in range(n)])


def _refused(rc, text):
    assert rc == _lib.PA_ERR_INVALID
    assert text in _lib.load().pa_last_error().decode()


def _no_staged_batch(lib, h):
    counts = np.zeros(2, np.int64)
    _refused(lib.pa_encoder_run_staged(h, counts.ctypes.data), "no staged batch")


# ---- host-clipped form ------------------------------------------------------------------------------------------------------
def _flat(n_reads=1, seq_offset=(0, L_SEQ)):
    return dict(read_pos=np.array([1010], np.int64), read_reverse=np.zeros(1, np.uint8), read_mapq=np.array([60], np.int32),
                seq_offset=np.array(seq_offset, np.int64), seq=np.frombuffer(b"ACGTA" * 4 + b"\0", np.uint8),
                qual=np.full(L_SEQ + 1, 30, np.uint8), cigar_offset=np.array([0, 1], np.int64),
                cigar_op=np.array([0, 0], np.int32), cigar_len=np.array([L_SEQ, 0], np.int32), n_reads=n_reads)


def _piles(flat, n=1, end=END):
    f = flat
    return (_Pileup * n)(*[_Pileup(START, end, REF, len(REF), f["n_reads"], f["read_pos"].ctypes.data, f["read_reverse"].ctypes.data,
                                   f["read_mapq"].ctypes.data, f["seq_offset"].ctypes.data, f["seq"].ctypes.data, f["qual"].ctypes.data,
                                   f["cigar_offset"].ctypes.data, f["cigar_op"].ctypes.data, f["cigar_len"].ctypes.data)
                           for _ in range(n)])


HOST_CASES = {
    "region_end_before_start": (dict(end=START - 1), {}, {}, "bad region"),
    "feature_size_25": ({}, dict(feature=25), {}, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "window_1": ({}, dict(window=(1, 1)), {}, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "window_255": ({}, dict(window=(255, 255)), {}, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "two_window_sizes": (dict(n=2), dict(n=2, window=(32, 16)), {}, "one batch has one window size and one feature size"),
    "negative_n_reads": ({}, {}, dict(n_reads=-1), "negative count"),
    "descending_seq_offset": ({}, {}, dict(seq_offset=(L_SEQ, 0)), "offsets of read 0 are not ascending"),
}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_host_clipped_form_refuses(enc, case):
    lib, h = enc
    pile_kw, par_kw, flat_kw, text = HOST_CASES[case]
    good = _flat()
    _lib.check(lib.pa_encoder_stage_batch(h, 1, ctypes.cast(_piles(good), ctypes.c_void_p), ctypes.cast(_params(), ctypes.c_void_p)))
    flat = _flat(**flat_kw)
    piles, pars = _piles(flat, **pile_kw), _params(**par_kw)
    _refused(lib.pa_encoder_stage_batch(h, len(piles), ctypes.cast(piles, ctypes.c_void_p), ctypes.cast(pars, ctypes.c_void_p)), text)
    _no_staged_batch(lib, h)                # (the batch staged before the refusal is gone as well)


# ---- packed form and the polish chain: one read at `data_off` of the arena ----------------------------------------------------
def _arena():
    a = np.zeros(ARENA, np.uint8)
    a[0:4] = np.frombuffer(np.array([L_SEQ << 4], np.uint32).tobytes(), np.uint8)           # 20M
    a[4:4 + (L_SEQ + 1) // 2] = 0x12                                                      # A C A C ...
    a[4 + (L_SEQ + 1) // 2:SLICE] = 30
    return a


def _regions(n=1, end=END):
    return (_PackedRegion * n)(*[_PackedRegion(START, end, REF, len(REF)) for _ in range(n)])


def _tables(data_off=0, pair_read=(0,), region_pairs=(0, 1)):
    reads = np.zeros(1, PACKED_READ)
    reads[0] = (data_off, 1010, 1, L_SEQ, 60 << 16)
    return reads, np.array(pair_read, np.int32), np.array(region_pairs, np.int32)


def _stage_packed(lib, h, regs, pars, arena, reads, pair_read, region_pairs):
    return lib.pa_encoder_stage_packed(h, len(regs), ctypes.cast(regs, ctypes.c_void_p), ctypes.cast(pars, ctypes.c_void_p),
                                       arena.ctypes.data, ARENA, reads.ctypes.data, len(reads), pair_read.ctypes.data,
                                       region_pairs.ctypes.data)


# (regions, parameters, tables, base offsets set for the call, message)
PACKED_CASES = {
    "region_end_before_start": (dict(end=START - 1), {}, {}, None, "bad region"),
    "feature_size_25": ({}, dict(feature=25), {}, None, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "window_1": ({}, dict(window=(1, 1)), {}, None, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "window_255": ({}, dict(window=(255, 255)), {}, None, "feature_size must be >= 26 and 2 <= candidate_window_size <= 254"),
    "two_window_sizes": (dict(n=2), dict(n=2, window=(32, 16)), dict(region_pairs=(0, 1, 1)), None,
                         "one batch has one window size and one feature size"),
    "region_pairs_start": ({}, {}, dict(region_pairs=(1, 1)), None, "region_pairs must start at 0 and ascend"),
    "region_pairs_descend": ({}, {}, dict(region_pairs=(0, -1)), None, "region_pairs must start at 0 and ascend"),
    "region_pairs_descend_inside": (dict(n=2), dict(n=2), dict(region_pairs=(0, 1, 0)), None, "negative count"),
    "pair_read_out_of_range": ({}, {}, dict(pair_read=(1,)), None, "pair_read out of range"),
    "read_past_the_arena": ({}, {}, dict(data_off=ARENA - SLICE + 1), None, "packed read 0 lies outside the arena"),
    "bases_past_the_arena": ({}, {}, {}, [ARENA - BASES + 1], "packed read 0 lies outside the arena"),
    "offsets_not_one_per_read": ({}, {}, {}, [-1, -1], "the base offsets set for this call are not one per packed read"),
}


@pytest.mark.parametrize("case", sorted(PACKED_CASES))
def test_packed_form_refuses(enc, case):
    lib, h = enc
    reg_kw, par_kw, tab_kw, soff, text = PACKED_CASES[case]
    arena = _arena()
    good = _tables()
    _lib.check(_stage_packed(lib, h, _regions(), _params(), arena, *good))
    if soff is not None:
        table = np.array(soff, np.int64)
        _lib.check(lib.pa_encoder_set_seq_offsets(h, table.ctypes.data, len(table)))
    _refused(_stage_packed(lib, h, _regions(**reg_kw), _params(**par_kw), arena, *_tables(**tab_kw)), text)
    _no_staged_batch(lib, h)
    # the same valid batch with no offsets set: whatever table the refused call was given has been consumed by it
    _lib.check(_stage_packed(lib, h, _regions(), _params(), arena, *good))
    counts = np.zeros(1, np.int64)
    _lib.check(lib.pa_encoder_run_staged(h, counts.ctypes.data))
    live = np.zeros(1, np.int32)
    _lib.check(lib.pa_encoder_region_reads(h, live.ctypes.data, 1))
    assert live[0] == 1 and counts[0] == 0


POLISH_CASES = {
    "region_end_before_start": (dict(end=START - 1), {}, "bad region"),
    "region_pairs_descend": ({}, dict(region_pairs=(0, -1)), "region_pairs must start at 0 and ascend"),
    "region_pairs_descend_inside": (dict(n=2), dict(region_pairs=(0, 1, 0)), "region_pairs must ascend"),
    "pair_read_out_of_range": ({}, dict(pair_read=(1,)), "pair_read out of range"),
    "read_past_the_arena": ({}, dict(data_off=ARENA - SLICE + 1), "packed read 0 lies outside the arena"),
}


@pytest.mark.parametrize("case", sorted(POLISH_CASES))
def test_polish_chain_refuses(enc, case):
    lib, h = enc
    reg_kw, tab_kw, text = POLISH_CASES[case]
    arena = _arena()
    regs = _regions(**reg_kw)
    reads, pair_read, region_pairs = _tables(**tab_kw)
    n = len(regs)
    rows, live, chunks, total = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), ctypes.c_int64()
    rc = lib.pa_polish_chain_run(h, n, ctypes.cast(regs, ctypes.c_void_p), arena.ctypes.data, ARENA, reads.ctypes.data, len(reads),
                                 pair_read.ctypes.data, region_pairs.ctypes.data, 0, 1000, 50, rows.ctypes.data, live.ctypes.data,
                                 chunks.ctypes.data, ctypes.byref(total))
    _refused(rc, text)
