"""Packed reads whose operations and bases lie apart (a CIGAR kept in the CG:B,I tag, SAM specification 4.2.2), host side:
pa_bam_set_split_slices makes pa_bam_pack_inflated / pa_bam_pack_headers keep such a record in place -- operations inside the
tag, bases and qualities in the core, the second offset in the table of pa_bam_split_offsets -- and what they keep decodes to
what pa_bam_pack_regions copies into its arena for the same BAM."""
import struct
import zlib

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
from record_walk_cases import split_headers          # (the restatement of the device's walk, tag walk included)
from pepper_amd.variant.bam import BAM_handler, BamError, PACKED_READ

AUX_EVERY_TYPE = (b"XAAq" + b"Xcc" + struct.pack("<b", -5) + b"XSS" + struct.pack("<H", 40000) + b"Xii" + struct.pack("<i", -70000) +
                  b"Xff" + struct.pack("<f", 1.5) + b"XBBc" + struct.pack("<I", 5) + bytes([1, 2, 3, 4, 5]) + b"XZZabc\0" +
                  b"MMZ" + b"C+m," * 175 + b"\0")


def _inflate_span(bam, contig, start, stop, lookahead=4):
    begin, first, end, final = bam.region_span(contig, start, stop, lookahead)
    buf = np.zeros(1 << 24, np.uint8)
    tables = (np.zeros(4096, np.int64), np.zeros(4096, np.int32), np.zeros(4096, np.int64), np.zeros(4096, np.int32))
    n, _comp_bytes, out_bytes, complete, at_eof = bam.read_span(begin, end, buf, tables, 1)
    assert complete
    data = np.zeros(out_bytes + 8, np.uint8)
    for k in range(n):
        o, l, at, m = int(tables[0][k]), int(tables[1][k]), int(tables[2][k]), int(tables[3][k])
        data[at:at + m] = np.frombuffer(zlib.decompress(buf[o:o + l].tobytes(), -15), np.uint8)
    return data, out_bytes, first, final or at_eof


def decode_split(arena, rd, seq_off):
    """bam_utils.unpack_packed_read with the second offset honoured: operations at data_off, `bases | qualities` at seq_off
    (-1: behind the operations)."""
    off, n_cig, l_seq = int(rd["data_off"]), int(rd["n_cigar"]), int(rd["l_seq"])
    words = np.frombuffer(arena[off:off + 4 * n_cig].tobytes(), "<u4")
    s0 = off + 4 * n_cig if seq_off < 0 else int(seq_off)
    packed = arena[s0:s0 + (l_seq + 1) // 2]
    codes = np.empty(2 * len(packed), np.uint8)
    codes[0::2] = packed >> 4
    codes[1::2] = packed & 15
    q0 = s0 + (l_seq + 1) // 2
    flags = int(rd["flags"])
    return dict(pos=int(rd["pos"]), cigar=[(int(w) & 15, int(w) >> 4) for w in words], seq="".join("=ACMGRSVTWYHKDBN"[c] for c in codes[:l_seq]),
                qual=arena[q0:q0 + l_seq].tolist(), flag=flags & 0xffff, mapq=(flags >> 16) & 0xff)


@pytest.fixture(scope="module")
def cg_bam(tmp_path_factory):
    """A few hundred reads over 60 kb, every fifth in CG form behind auxiliary fields of every type; flagged and mapq-0 records among both."""
    rng = np.random.default_rng(4221)
    ref = pu.random_reference(rng, 60000)
    reads = pu.simulate_reads(rng, ref, 0, n_reads=1000, read_len=(300, 5000), clip_rate=0.3, mapq_zero_rate=0.05)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "r%d" % i
        r["flag"] = (16 if r["reverse"] else 0) | int(rng.choice([0, 0x800, 0x100, 0x400], p=[.91, .03, .03, .03]))
        if i % 5 == 2:
            r["long_cigar"] = True
            r["aux"] = AUX_EVERY_TYPE if i % 2 else b""
    path = str(tmp_path_factory.mktemp("split") / "cg.bam")
    bu.write_bam(path, [("ctg", len(ref))], {0: reads}, flush_every=23)
    return path, reads


def _tables():
    return np.zeros(4000, PACKED_READ), np.zeros(8000, np.int32)


def test_split_slices_keep_what_the_host_packer_copies(cg_bam):
    path, reads = cg_bam
    bam = BAM_handler(path)
    edges = list(range(2000, 58001, 7000))
    starts, stops = [a - 100 for a in edges[:-1]], [b + 100 for b in edges[1:]]
    arena = np.zeros(1 << 24, np.uint8)
    t0, p0 = _tables()
    n0, rp0, c0 = bam.pack_regions("ctg", starts, stops, False, 1, arena, t0, p0)
    assert n0 == len(starts) and c0[0] > 100
    data, data_bytes, first, final = _inflate_span(bam, "ctg", starts[0], stops[-1])
    # a new handle refuses the record (-8); the switch is per handle and can be taken back
    t1, p1 = _tables()
    with pytest.raises(BamError) as e:
        bam.pack_inflated(data, data_bytes, first, final, "ctg", starts, stops, False, 1, t1, p1)
    assert e.value.code == -8
    n1, rp1, c1 = bam.pack_inflated(data, data_bytes, first, final, "ctg", starts, stops, False, 1, t1, p1, long_cigars=True)
    seq_off, n_split = bam.split_offsets(c1[0])
    assert (n1, c1[:2]) == (n0, c0[:2]) and rp1.tolist() == rp0.tolist() and p1[:c1[1]].tolist() == p0[:c0[1]].tolist()
    wanted_split = 0
    for k in range(c0[0]):
        want = bu.unpack_packed_read(arena, t0[k])
        assert decode_split(data, t1[k], int(seq_off[k])) == want, k
        wanted_split += int(seq_off[k]) >= 0
    by_pos = {}
    for r in reads:
        by_pos.setdefault(r["pos"], []).append(r)
    kept_cg = sum(1 for k in range(c0[0]) if any(r.get("long_cigar") and [tuple(c) for c in r["cigar"]] == bu.unpack_packed_read(arena, t0[k])["cigar"]
                                                  for r in by_pos[int(t0[k]["pos"])]))
    assert n_split == wanted_split == kept_cg > 10
    # the headers the device's walk reports for the same span give the same tables
    headers = split_headers(data, data_bytes, first)
    assert int((headers["state"] == 3).sum()) >= n_split
    t2, p2 = _tables()
    with pytest.raises(BamError) as e:
        bam.pack_headers(headers, len(headers), final, "ctg", starts, stops, False, 1, t2, p2)
    assert e.value.code == -8
    n2, rp2, c2 = bam.pack_headers(headers, len(headers), final, "ctg", starts, stops, False, 1, t2, p2, long_cigars=True)
    seq_off2, n_split2 = bam.split_offsets(c2[0])
    assert (n2, c2) == (n1, c1) and rp2.tolist() == rp1.tolist() and p2[:c2[1]].tolist() == p1[:c1[1]].tolist()
    assert t2[:c2[0]].tobytes() == t1[:c1[0]].tobytes() and seq_off2.tolist() == seq_off.tolist() and n_split2 == n_split
    with pytest.raises(BamError):
        bam.split_offsets(c2[0] + 1)
    bam.close()


def test_placeholder_without_a_usable_tag_keeps_its_core_cigar(tmp_path):
    """A placeholder record whose CG tag is missing, or holds fewer operations than the core field, is what the host reader
    makes of it: the core CIGAR <l_seq>S<ref_len>N, one slice."""
    rng = np.random.default_rng(4222)
    seq = "".join("ACGT"[k] for k in rng.integers(0, 4, 600))
    base = dict(flag=0, mapq=60, cigar=[(0, 300), (2, 3), (0, 300)], seq=seq, qual=list(rng.integers(5, 40, 600)), long_cigar=True, drop_cg=True)
    short_tag = b"XZZhello\0" + b"CGBI" + struct.pack("<I", 1) + struct.pack("<I", (600 << 4) | 0)
    recs = [dict(base, name="plain", pos=100, long_cigar=False), dict(base, name="none", pos=200),
            dict(base, name="short", pos=300, aux=short_tag), dict(base, name="real", pos=400, drop_cg=False, aux=AUX_EVERY_TYPE)]
    path = str(tmp_path / "p.bam")
    bu.write_bam(path, [("ctg", 5000)], {0: recs})
    bam = BAM_handler(path)
    arena = np.zeros(1 << 20, np.uint8)
    t0, p0 = _tables()
    n0, rp0, c0 = bam.pack_regions("ctg", [0], [2000], False, 0, arena, t0, p0)
    assert c0[0] == 4
    data, data_bytes, first, final = _inflate_span(bam, "ctg", 0, 2000)
    headers = split_headers(data, data_bytes, first)
    assert headers["state"].tolist() == [0, 0, 0, 3]
    for walk in ("inflated", "headers"):
        t1, p1 = _tables()
        if walk == "inflated":
            n1, rp1, c1 = bam.pack_inflated(data, data_bytes, first, final, "ctg", [0], [2000], False, 0, t1, p1, long_cigars=True)
        else:
            n1, rp1, c1 = bam.pack_headers(headers, len(headers), final, "ctg", [0], [2000], False, 0, t1, p1, long_cigars=True)
        seq_off, n_split = bam.split_offsets(c1[0])
        assert c1[:2] == c0[:2] and rp1.tolist() == rp0.tolist()
        assert (seq_off >= 0).tolist() == [False, False, False, True] and n_split == 1
        got = [decode_split(data, t1[k], int(seq_off[k])) for k in range(4)]
        assert got == [bu.unpack_packed_read(arena, t0[k]) for k in range(4)]
        assert got[1]["cigar"] == got[2]["cigar"] == [(4, 600), (3, 603)] and got[3]["cigar"] == [(0, 300), (2, 3), (0, 300)]
    bam.close()
