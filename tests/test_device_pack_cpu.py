"""The device pack's surface without a GPU: the PEPPER_AMD_DEVICE_PACK switch parses like its siblings, the new entry points
are declared, exported and bound, PackedEncoder.pack_device(device_pack=False) touches none of them, and the shared per-record
rules (pa_bam_pack_rule) equal a NumPy restatement on hand-built headers."""
import os
import re

import numpy as np

import test_pack_device_cpu as stub
from pepper_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pa_encoder_submit_walk", "pa_encoder_walk_headers", "pa_encoder_pack_records", "pa_encoder_stage_packed_device",
                "pa_encoder_packed_tables", "pa_encoder_pack_calls")


def test_the_switch_parses_like_its_siblings(monkeypatch):
    monkeypatch.delenv("PEPPER_AMD_DEVICE_PACK", raising=False)
    assert _lib.device_pack() is False
    for value, want in (("0", False), ("1", True), ("yes", False), ("", False), ("2", False)):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_PACK", value)
        assert _lib.device_pack() is want, value
    # (the sibling it is written like)
    monkeypatch.setenv("PEPPER_AMD_DEVICE_CANDIDATES", "junk")
    assert _lib.device_candidates() is False


def test_entry_points_declared_exported_and_bound():
    from pepper_amd import build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "pepper_amd_encoder.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound and hasattr(lib, name), name
    assert "pa_device_pack;" in code


def test_the_summary_struct_mirrors_the_header():
    import ctypes
    assert ctypes.sizeof(_lib.DevicePack) == 64
    assert _lib.DevicePack.slice_bytes.offset == 40 and _lib.DevicePack.n_headers.offset == 32


def test_switch_off_touches_no_new_entry_point(monkeypatch):
    """The stand-in library of tests/test_pack_device_cpu.py has none of the new entry points: a call with device_pack=False
    that reached for one would raise AttributeError instead of taking the stale-index way out."""
    monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", "1")
    enc = stub._encoder(_lib.PA_ERR_INVALID)
    assert not any(hasattr(enc.lib, name) for name in ENTRY_POINTS)
    got = enc.pack_device(stub._FakeBam(), "chr20", np.array([0]), np.array([1000]), False, 1, device_pack=False)
    assert got is None and enc.lib.calls == ["inflate", "walk"]


def test_the_host_walk_is_compiled_from_the_shared_rule():
    text = open(os.path.join(REPO, "pepper_amd", "csrc", "bamio.cpp")).read()
    kernels = open(os.path.join(REPO, "pepper_amd", "csrc", "encoder.hip")).read()
    for name in ("header_class", "record_dropped", "first_open_region", "region_range_end", "read_end", "slice_bytes"):
        assert "pa_pack::" + name in text and "pa_pack::" + name in kernels, name


def test_the_shared_rule_equals_its_restatement():
    """pa_bam_pack_rule (csrc/pack_rule.h compiled for the host: the functions the kernels call) on hand-built headers: the
    boundary rows with the values worked out by hand, then filters, walk ends and random tables against NumPy."""
    import ctypes
    import device_pack_cases as cases
    from pepper_amd.variant import bam

    def rule(hdr, starts, stops, supp, min_mapq):
        starts, stops = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(stops, np.int64)
        out = np.full((len(hdr), 4), -7, np.int32)
        assert bam._lib().pa_bam_pack_rule(hdr.ctypes.data, len(hdr), cases.TID, len(starts), starts.ctypes.data, stops.ctypes.data,
                                           supp, min_mapq, out.ctypes.data) == 0
        return out

    starts, stops = [1000, 2000, 3000, 4000], [2000, 3000, 4000, 5000]
    rows = [dict(pos=900, ref_len=2200),                                   # three regions
            dict(pos=1500, ref_len=500), dict(pos=1500, ref_len=501),      # end == start[1]: not its read; one more: its read
            dict(pos=1999, ref_len=1), dict(pos=2000, ref_len=1),          # pos == stop[0] - 1, pos == stop[0]
            dict(pos=2999, ref_len=0),                                     # ref_len 0 counts as 1
            dict(pos=500, ref_len=500), dict(pos=500, ref_len=501),        # in front of every region / reaching the first
            dict(pos=4999), dict(pos=5000), dict(ref_id=0, pos=10), dict(ref_id=2, pos=10), dict(ref_id=-1, pos=-1)]
    got = rule(cases.headers(rows), starts, stops, 0, 5)
    assert got[:8, 2:].tolist() == [[0, 3], [0, 1], [0, 2], [0, 1], [1, 2], [1, 2], [0, 0], [0, 1]]
    assert got[:, 0].tolist() == [2] * 9 + [1, 0, 1, 1] and not got[:, 1].any()
    assert rule(cases.headers([]), starts, stops, 0, 5).shape == (0, 4)

    rows = [dict(pos=10 * k, flag=flag) for k, flag in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0, 16))]
    rows += [dict(pos=500, mapq=5), dict(pos=510, mapq=4), dict(pos=520, l_seq=0), dict(pos=530, n_cigar=0)]
    assert rule(cases.headers(rows), starts, stops, 0, 5)[:, 1].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert rule(cases.headers(rows), starts, stops, 1, 4)[:, 1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1]

    rng = np.random.default_rng(9)
    for n_regions, kind in ((1, "abutting"), (2, "flank"), (17, "abutting"), (17, "flank"), (2, "gap"), (17, "gap")):
        starts, stops = cases.layouts(n_regions, kind)
        hdr = cases.random_headers(rng, 400, int(stops[-1]) + 800)
        hdr["ref_id"][::50] = [0, 2, -1, 1, 0, 2, -1, 1]
        for supp, min_mapq in ((0, 5), (1, 0)):
            got = rule(hdr, starts, stops, supp, min_mapq)
            ref_id, pos = hdr["ref_id"].astype(np.int64), hdr["pos"].astype(np.int64)
            flag, mapq = hdr["flags"] & 0xffff, (hdr["flags"] >> 16) & 0xff
            want_class = np.where(ref_id != cases.TID, np.where((ref_id > cases.TID) | (ref_id < 0), 1, 0), np.where(pos >= stops[-1], 1, 2))
            dropped = ((flag & 0x704) != 0) | ((supp == 0) & ((flag & 0x800) != 0)) | (mapq < min_mapq) | (hdr["l_seq"] == 0) | (hdr["n_cigar"] == 0)
            lo = np.searchsorted(stops, pos, side="right")
            hi = np.maximum(lo, np.searchsorted(starts, pos + np.maximum(1, hdr["ref_len"].astype(np.int64)), side="left"))
            assert np.array_equal(got[:, 0], want_class) and np.array_equal(got[:, 1], dropped)
            assert np.array_equal(got[:, 2], lo) and np.array_equal(got[:, 3], hi), (n_regions, kind)


def restated_device_pack(hdr, tid, starts, stops, final, supp, min_mapq, split):
    """The device pack's formulation in NumPy -- walk end as a first index, closed regions from the prefix maximum of the
    positions, a read's regions from two searches, snapshots at the header that closes a region -- without the arena test.
    -> (status, n_done, region_pairs, n_reads, n_pairs, slice_bytes, kept header indices, pair_read, seq_off)"""
    starts, stops = np.asarray(starts, np.int64), np.asarray(stops, np.int64)
    n_regions = len(starts)
    ref_id, pos = hdr["ref_id"].astype(np.int64), hdr["pos"].astype(np.int64)
    stop_here = (hdr["state"] == 2) | ((ref_id != tid) & ((ref_id > tid) | (ref_id < 0))) | ((ref_id == tid) & (pos >= stops[-1]))
    end = int(np.flatnonzero(stop_here)[0]) if stop_here.any() else len(hdr)
    if end < len(hdr) and hdr["state"][end] == 2:
        return (2,)
    h, pos = hdr[:end], pos[:end]
    active = h["ref_id"] == tid
    prefix_max = np.maximum.accumulate(np.where(active, pos, np.iinfo(np.int64).min)) if end else np.zeros(0, np.int64)
    lo = np.searchsorted(stops, prefix_max, side="right")            # first region with stop > the furthest position seen
    flag, mapq = h["flags"] & 0xffff, (h["flags"] >> 16) & 0xff
    kept = active & ((flag & 0x704) == 0) & ((supp != 0) | ((flag & 0x800) == 0)) & (mapq >= min_mapq) & (h["l_seq"] != 0) & (h["n_cigar"] != 0)
    read_end = pos + np.maximum(1, h["ref_len"].astype(np.int64))
    hi = np.maximum(lo, np.searchsorted(starts, read_end, side="left"))       # regions with start < end
    is_read = kept & (hi > lo)
    if (is_read & ((h["state"] == 1) | ((h["state"] == 3) & (not split)))).any():
        return (3,)
    bytes_ = np.where(is_read, 4 * h["n_cigar"].astype(np.int64) + (h["l_seq"].astype(np.int64) + 1) // 2 + h["l_seq"], 0)
    read_index = np.cumsum(is_read) - is_read
    cut = end == len(hdr) and not final
    n_closed = int(np.searchsorted(stops, prefix_max[-1] if end and active.any() else np.iinfo(np.int64).min, side="right")) if cut else n_regions
    if cut and n_closed == 0:
        return (4,)
    if cut:
        closer = int(np.flatnonzero(active & (prefix_max >= stops[n_closed - 1]))[0])     # the header that closed the last closed region
        n_reads, slice_bytes = int(read_index[closer]), int(bytes_[:closer].sum())
    else:
        n_reads, slice_bytes = int(is_read.sum()), int(bytes_.sum())
    region_pairs = np.zeros(n_regions + 1, np.int32)
    pair_read = []
    for r in range(n_regions):
        mine = np.flatnonzero(is_read & (lo <= r) & (r < hi)) if r < n_closed else np.zeros(0, np.int64)
        pair_read += read_index[mine].tolist()
        region_pairs[r + 1] = len(pair_read)
    which = np.flatnonzero(is_read)[:n_reads]
    seq_off = np.where(h["state"][which] == 3, h["data_off"][which] - h["block_size"][which], -1)
    return 0, n_closed, region_pairs, n_reads, len(pair_read), slice_bytes, which, np.array(pair_read, np.int32), seq_off


def test_the_formulation_the_kernels_use_equals_the_host_walk(tmp_path):
    """pa_bam_pack_headers against the NumPy restatement above on random and on unsorted tables, cut and final."""
    import bam_utils as bu
    import device_pack_cases as cases
    from pepper_amd.variant.bam import BAM_handler, BamError, PACKED_READ
    bam = str(tmp_path / "three_contigs.bam")
    bu.write_bam(bam, [("a", 1000), ("ctg", 60000), ("z", 1000)], {})
    handler = BAM_handler(bam)
    reads, pairs = np.zeros(8192, PACKED_READ), np.zeros(1 << 16, np.int32)
    rng = np.random.default_rng(31)
    checked = 0
    for trial in range(60):
        n_regions, kind = [(1, "abutting"), (2, "flank"), (17, "flank"), (17, "gap"), (5, "abutting")][trial % 5]
        starts, stops = cases.layouts(n_regions, kind)
        hdr = cases.random_headers(rng, int(rng.choice([0, 1, 40, 700])), int(stops[-1]) + (800 if trial % 3 else -2500))
        if trial % 4 == 3 and len(hdr) > 2:
            rng.shuffle(hdr)                                # an unsorted table: the furthest position seen closes regions
        if trial % 7 == 6 and len(hdr) > 2:
            hdr["ref_id"][:len(hdr) // 4] = 0
            hdr["ref_id"][-3:] = [2, 1, 1]
        if trial % 6 == 5 and len(hdr) > 9:
            hdr["state"][::9] = 3
            hdr["data_off"][::9] += 40000
            hdr["block_size"][::9] = 5000
        split = trial % 2 == 0
        for final in (1, 0):
            got = restated_device_pack(hdr, cases.TID, starts, stops, final, trial % 2, 5, split)
            try:
                n_done, rp, counts = handler.pack_headers(hdr if len(hdr) else cases.headers([dict()]), len(hdr), final, "ctg", starts, stops,
                                                          trial % 2, 5, reads, pairs, long_cigars=split)
            except BamError as err:
                assert got[0] in cases.STATUS_OF_RC[err.code], (trial, got[0], err.code)
                continue
            status, n_closed, region_pairs, n_reads, n_pairs, slice_bytes, which, pair_read, seq_off = got
            assert status == 0 and n_closed == n_done and np.array_equal(region_pairs, rp), trial
            assert (n_reads, n_pairs, slice_bytes) == counts, trial
            assert np.array_equal(hdr["pos"][which], reads["pos"][:n_reads]) and np.array_equal(hdr["data_off"][which], reads["data_off"][:n_reads])
            assert np.array_equal(pair_read, pairs[:n_pairs]), trial
            assert np.array_equal(seq_off, handler.split_offsets(n_reads)[0]), trial
            checked += 1
    assert checked > 60
