"""pa_encoder_pack_records against pa_bam_pack_headers on header tables built by hand: the same array goes to both, and
n_done, region_pairs, the counts, the read table, pair_read and the base offsets must agree byte for byte wherever the host
walk returns 0; where it fails the device reports the matching status.  The span behind the offsets is the inflated span of a
small BAM that one pack_device call leaves resident."""
import ctypes

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
from device_pack_cases import STATUS_OF_RC, TID, headers, layouts, random_headers
from pepper_amd import _lib

pytestmark = pytest.mark.gpu

BLOCK = 1024        # PACK_BLOCK of csrc/encoder.hip: headers (pack_scan_kernel) and reads (pack_fill_kernel) per scan step


@pytest.fixture(scope="module")
def rig(tmp_path_factory):
    from pepper_amd.variant.bam import BAM_handler, PACKED_READ
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    tmp = tmp_path_factory.mktemp("device_pack")
    rng = np.random.default_rng(77)
    ref = pu.random_reference(rng, 20000)
    reads = [r for r in pu.simulate_reads(rng, ref, 0, n_reads=120, read_len=(500, 2000)) if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "r%d" % i
    bam = str(tmp / "span.bam")
    bu.write_bam(bam, [("a", 1000), ("ctg", len(ref)), ("z", 1000)], {1: reads})
    handler = BAM_handler(bam)
    assert handler.contig_index("ctg") == TID and handler.contig_index("nope") == -1
    enc = PackedEncoder(0, arena_bytes=16 << 20, max_reads=4096, max_pairs=8192)
    got = enc.pack_device(handler, "ctg", [0], [20000], False, 0)
    assert got is not None
    span_bytes = got[2][2]
    assert span_bytes > 50000
    host_reads, host_pairs = np.zeros(4096, PACKED_READ), np.zeros(8192, np.int32)
    yield dict(enc=enc, handler=handler, span=span_bytes, reads=host_reads, pairs=host_pairs)
    enc.close()


def device(rig, hdr, starts, stops, final=1, supp=0, min_mapq=5, split=False, reads_cap=4096, pairs_cap=8192):
    enc = rig["enc"]
    _lib.check(enc.lib.pa_encoder_set_split_slices(enc.enc, 1 if split else 0))
    enc._split_walk = bool(split)
    starts, stops = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(stops, np.int64)
    n = len(starts)
    out, rp = _lib.DevicePack(), np.full(n + 1, -5, np.int32)
    table = hdr if len(hdr) else headers([dict()])      # (no entries: one header that is never looked at -- NULL would mean the handle's last walk)
    _lib.check(enc.lib.pa_encoder_pack_records(enc.enc, table.ctypes.data, len(hdr), final, TID, n, starts.ctypes.data,
                                               stops.ctypes.data, supp, min_mapq, reads_cap, pairs_cap, rp.ctypes.data,
                                               ctypes.byref(out)))
    return out, rp


def same(rig, hdr, starts, stops, final=1, supp=0, min_mapq=5, split=False):
    """Both packs on the same table -> the device's summary (after every comparison the host's verdict allows)."""
    from pepper_amd.variant.bam import BamError
    out, rp = device(rig, hdr, starts, stops, final, supp, min_mapq, split)
    handler = rig["handler"]
    try:
        n_done, want_rp, counts = handler.pack_headers(hdr if len(hdr) else headers([dict()]), len(hdr), final, "ctg", starts, stops,
                                                       supp, min_mapq, rig["reads"], rig["pairs"], long_cigars=split)
    except BamError as err:
        assert out.status in STATUS_OF_RC[err.code], (out.status, err.code)
        return out
    assert out.status == 0, out.status
    assert out.n_done == n_done and np.array_equal(rp, want_rp)
    assert (out.n_reads, out.n_pairs, out.slice_bytes) == counts
    reads, pair_read, seq_off = rig["enc"].packed_tables(out.n_reads, out.n_pairs)
    for field in ("data_off", "pos", "n_cigar", "l_seq", "flags"):
        assert np.array_equal(reads[field], rig["reads"][field][:out.n_reads]), field
    assert np.array_equal(pair_read, rig["pairs"][:out.n_pairs])
    want_off, n_split = handler.split_offsets(out.n_reads)
    assert np.array_equal(seq_off, want_off) and out.n_split == n_split
    return out


@pytest.mark.parametrize("n", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 452])
@pytest.mark.parametrize("n_regions,kind", [(1, "abutting"), (2, "flank"), (17, "abutting"), (17, "flank"), (2, "gap"), (17, "gap")])
def test_record_counts_and_region_layouts(rig, n, n_regions, kind):
    starts, stops = layouts(n_regions, kind)
    hdr = random_headers(np.random.default_rng(1000 + n + n_regions), n, int(stops[-1]) + 800)
    out = same(rig, hdr, starts, stops)
    assert out.n_done == n_regions and (n < BLOCK or out.n_pairs >= out.n_reads > 0)
    # the same table cut short: not final, so only the regions a position has closed are done
    cut = hdr[:max(0, n - n // 3)]
    same(rig, cut, starts, stops, final=0)


def test_region_boundaries(rig):
    starts, stops = [1000, 2000, 3000, 4000], [2000, 3000, 4000, 5000]
    rows = [dict(pos=900, ref_len=2200),                 # three regions
            dict(pos=1500, ref_len=500),                 # end == start[1]: not a read of region 1
            dict(pos=1500, ref_len=501),                 # end == start[1] + 1
            dict(pos=1999, ref_len=1), dict(pos=2000, ref_len=1),          # pos == stop[0] - 1, pos == stop[0]
            dict(pos=2999, ref_len=0), dict(pos=3999, ref_len=0),          # ref_len 0 counts as 1
            dict(pos=500, ref_len=500), dict(pos=500, ref_len=501)]
    rows.sort(key=lambda r: r["pos"])
    out = same(rig, headers(rows), starts, stops)
    assert out.n_done == 4 and out.n_reads == 8 and out.n_pairs == 11
    out = same(rig, headers(rows), [a - 100 for a in starts], [b + 100 for b in stops])
    assert out.n_pairs > 11


def test_filters(rig):
    starts, stops = [0, 1000], [1000, 2000]
    rows = [dict(pos=10 * k, flag=flag) for k, flag in enumerate((0x4, 0x100, 0x200, 0x400, 0x800, 0, 16))]
    rows += [dict(pos=500, mapq=5), dict(pos=510, mapq=4), dict(pos=520, l_seq=0), dict(pos=530, n_cigar=0)]
    assert same(rig, headers(rows), starts, stops, supp=0).n_reads == 3
    assert same(rig, headers(rows), starts, stops, supp=1).n_reads == 4
    assert same(rig, headers(rows), starts, stops, supp=1, min_mapq=4).n_reads == 5


def test_walk_start_and_end(rig):
    starts, stops = [0, 1000], [1000, 2000]
    lead = [dict(ref_id=0, pos=5), dict(ref_id=0, pos=900)]
    body = [dict(pos=100), dict(pos=950, ref_len=200), dict(pos=1500)]
    assert same(rig, headers(lead + body), starts, stops).n_reads == 3
    for stopper in (dict(ref_id=2, pos=0), dict(ref_id=-1, pos=-1), dict(pos=2000), dict(pos=5000)):
        out = same(rig, headers(lead + body[:2] + [stopper] + body[2:]), starts, stops, final=0)
        assert out.n_done == 2 and out.n_reads == 2          # what follows the stopping header does not count, cut or not


def test_cuts(rig):
    starts, stops = [0, 1000, 2000], [1000, 2000, 3000]
    rows = [dict(pos=100), dict(pos=900, ref_len=1500), dict(pos=1200), dict(pos=1900)]
    out = same(rig, headers(rows), starts, stops, final=0)
    assert out.n_done == 1 and out.n_reads == 2 and out.n_pairs == 2
    assert same(rig, headers(rows), starts, stops, final=1).n_done == 3
    out = same(rig, headers(rows[:2]), starts, stops, final=0)            # before the first stop: host rc -9
    assert out.status == 4
    assert same(rig, headers(rows[:2]), starts, stops, final=1).n_done == 3
    assert same(rig, headers([]), starts, stops, final=0).status == 4
    # an unsorted table: the furthest position seen is what closes regions
    rows = [dict(pos=100), dict(pos=1100), dict(pos=300, ref_len=900), dict(pos=1200)]
    assert same(rig, headers(rows), starts, stops, final=0).n_done == 1


def test_cg_records(rig):
    starts, stops = [0, 1000], [1000, 2000]
    cg = dict(pos=200, state=3, data_off=3000, block_size=1200, n_cigar=70, ref_len=900)
    rows = [dict(pos=100), cg, dict(pos=1500), dict(pos=1600, state=3, data_off=9000, block_size=4000)]
    out = same(rig, headers(rows), starts, stops, split=True)
    assert out.n_split == 2 and out.n_reads == 4
    assert same(rig, headers(rows), starts, stops, split=False).status == 3          # host rc -8
    placeholder = dict(pos=300, state=1)
    assert same(rig, headers(rows[:1] + [placeholder]), starts, stops, split=True).status == 3
    assert same(rig, headers(rows[:1] + [dict(pos=300, state=1, flag=0x4)]), starts, stops, split=True).status == 0
    # the bases in front of the span: host rc -6
    assert same(rig, headers([dict(pos=5, state=3, data_off=100, block_size=500)]), starts, stops, split=True).status == 5


def test_malformed_and_oversized_input(rig):
    starts, stops = [0, 1000], [1000, 2000]
    rows = [dict(pos=100), dict(pos=200, state=2), dict(pos=1500)]
    assert same(rig, headers(rows), starts, stops).status == 2               # host rc -6
    assert same(rig, headers(rows[:1] + [dict(pos=2500)] + rows[1:]), starts, stops).status == 0       # behind the walk's end
    rows = [dict(pos=100 * k, ref_len=1500) for k in range(10)]
    full, _ = device(rig, headers(rows), starts, stops)
    assert full.status == 0 and (full.n_reads, full.n_pairs) == (10, 20)
    assert device(rig, headers(rows), starts, stops, reads_cap=9)[0].status == 1
    assert device(rig, headers(rows), starts, stops, pairs_cap=19)[0].status == 1
    assert device(rig, headers(rows), starts, stops, reads_cap=10, pairs_cap=20)[0].status == 0
    # a slice that leaves the span: reported, nothing staged, no kernel run over it
    enc = rig["enc"]
    calls = enc.pack_calls()
    for bad in (dict(pos=300, data_off=rig["span"] - 40), dict(pos=300, data_off=1 << 40), dict(pos=300, data_off=-8),
                dict(pos=300, n_cigar=1 << 30), dict(pos=300, l_seq=-3)):
        out, rp = device(rig, headers(rows[:2] + [bad]), starts, stops)
        assert out.status == 5 and out.n_done == 0 and not rp.any(), bad
        assert enc.lib.pa_encoder_stage_packed_device(enc.enc, 0, None, None) != 0
        assert enc.lib.pa_encoder_packed_tables(enc.enc, None, None, None) != 0
    edge = dict(pos=300, data_off=rig["span"] - (12 + 25 + 50))              # the last byte of the span: inside
    assert device(rig, headers(rows[:2] + [edge]), starts, stops)[0].status == 0
    assert enc.pack_calls() == (calls[0] + 1, calls[1] + 5)


def test_back_to_back_calls_reuse_the_buffers(rig):
    starts, stops = layouts(17, "flank")
    big = random_headers(np.random.default_rng(5), 3 * BLOCK, int(stops[-1]))
    # no filter drops a record of the large table: every header that reaches the flanked regions (they cover everything from
    # 1 900 on, 96 % of the positions drawn) is a read, so the read table spans more than two scan blocks of the fill pass too
    big["flags"] = (big["flags"] & 16) | (60 << 16)
    small = random_headers(np.random.default_rng(6), 7, 4000)
    small["flags"] = (small["flags"] & 16) | (60 << 16)
    small["pos"] += 1900                               # (inside the first region, whatever they cover)
    a = same(rig, big, starts, stops)
    b = same(rig, small, starts[:2], stops[:2])
    assert a.n_pairs >= a.n_reads > 2 * BLOCK and b.n_reads == 7
    same(rig, big, starts, stops)
