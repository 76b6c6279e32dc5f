"""Reads whose CIGAR travels in the CG:B,I tag (SAM specification 4.2.2) kept on the device image path: record_finish_kernel
finds the tag among the record's auxiliary fields, pa_bam_pack_headers / pa_bam_pack_inflated keep the record in place with a
second offset for its bases, unpack_clip_kernel reads operations and bases from the two places.  Everything is compared with
the host packer's form (pa_bam_pack_regions copies both parts into one slice), which tests/test_gpu_images_vs_ref.py holds to the
reference for such reads."""
import glob
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import test_split_slices_cpu as host_side          # (its restatement of the tag walk and its host inflate of a span)
from pepper_amd import h5

pytestmark = pytest.mark.gpu

# auxiliary fields of every type in front of the tag: A, c, S, i, f, a B,c array, a Z string of 3 bytes and one of 700
AUX_EVERY_TYPE = (b"XAAq" + b"Xcc" + struct.pack("<b", -5) + b"XSS" + struct.pack("<H", 40000) + b"Xii" + struct.pack("<i", -70000) +
                  b"Xff" + struct.pack("<f", 1.5) + b"XBBc" + struct.pack("<I", 5) + bytes([1, 2, 3, 4, 5]) + b"XZZabc\0" +
                  b"MMZ" + b"C+m," * 175 + b"\0")
PARAMS = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)


def _passes(r, min_mapq, lo, hi):
    """The packer's filters and its region test over the run of regions [lo, hi]."""
    flag = r.get("flag", 16 if r.get("reverse") else 0)
    return (not flag & 0xf04 and r.get("mapq", 60) >= min_mapq and r["pos"] < hi and r["pos"] + max(1, bu.ref_length(r["cigar"])) > lo)


def _same_outputs(got, want):
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for key in g:
            assert (g[key] == w[key]) if isinstance(g[key], list) else np.array_equal(g[key], w[key]), key


def _host_and_device(bam, contig, ref, edges, min_mapq, monkeypatch, expect_cg):
    """pack + encode against pack_device(long_cigars=True) + encode(resident=True), with the records read out on the device
    and with the span walked on the host."""
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    starts, stops = [a - 100 for a in edges[:-1]], [b + 100 for b in edges[1:]]
    regions = list(zip(starts, stops))
    refs = [ref[a:b + 1] for a, b in regions]
    cands = list(zip(edges[:-1], edges[1:]))
    enc = PackedEncoder(0, arena_bytes=64 << 20)
    handler = BAM_handler(bam)
    n_done, rp_h, counts_h = enc.pack(handler, contig, starts, stops, False, min_mapq)
    assert n_done == len(starts)
    want, live_h = enc.encode(regions, refs, rp_h, counts_h, PARAMS, cands)
    enc.close()
    for walk in ("1", "0"):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", walk)
        enc = PackedEncoder(0, arena_bytes=64 << 20)
        laps = {}
        on_device = enc.pack_device(handler, contig, starts, stops, False, min_mapq, laps=laps, long_cigars=True)
        assert on_device is not None and ("bam_walk_device" in laps) == (walk == "1")
        n_done, rp_d, counts_d = on_device
        assert n_done == len(starts) and counts_d[:2] == counts_h[:2] and rp_d.tolist() == rp_h.tolist()
        assert enc.long_cigar_reads == expect_cg
        # the tables came from the headers the device read out, not from the host walk pack_device falls back to ...
        assert enc.host_walk_spans == 0
        if walk == "1":
            # ... and those headers are the ones the host restatement of the tag walk derives from the same span, state 3 included
            data, data_bytes, first, _final = host_side._inflate_span(handler, contig, starts[0], stops[-1])
            derived = host_side.split_headers(data, data_bytes, first)
            assert int((derived["state"] == 3).sum()) >= expect_cg > 0
            assert enc.headers[:len(derived)].tobytes() == derived.tobytes()
        got, live_d = enc.encode(regions, refs, rp_d, counts_d, PARAMS, cands, resident=True)
        assert live_d.tolist() == live_h.tolist()
        _same_outputs(got, want)
        enc.close()
    return want


def test_cg_records_stay_on_the_device(tmp_path, monkeypatch):
    """CG records as the first and the last record of the span, cut by BGZF member boundaries (members of 19 records: one in
    three holds a CG record of several kb, and the 64 kb limit cuts inside them), reaching up to three regions, on both
    strands, every other one behind auxiliary fields of every type."""
    rng = np.random.default_rng(913)
    ref = pu.random_reference(rng, 60000)
    sites = {int(p): ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.5) for p in rng.choice(np.arange(300, 59000), 150, replace=False)}
    reads = pu.simulate_reads(rng, ref, 0, n_reads=1500, read_len=(500, 6000), snp_sites=sites,
                              indel_sites={20000: ("I", "ACGTACGTTTGACA", 0.5), 30000: ("D", 12, 0.5)}, clip_rate=0.3)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    assert 300 < len(reads) < 1000
    # two reads of 11 kb (simulated reads of that length rarely come without an N or P operation): four regions each, one per strand
    for pos, reverse in ((12000, False), (33050, True)):
        seq = ref[pos:pos + 4000] + "GT" + ref[pos + 4000:pos + 7000] + ref[pos + 7005:pos + 11005]
        reads.append(dict(pos=pos, reverse=reverse, mapq=60, cigar=[(0, 4000), (1, 2), (0, 3000), (2, 5), (0, 4000)], seq=seq,
                          qual=(np.arange(len(seq)) % 31 + 5).astype(np.uint8), wide=True))
    reads.sort(key=lambda r: r["pos"])
    n_cg = 0
    for i, r in enumerate(reads):
        r["name"] = "read_%05d" % i
        if i % 6 == 0 or i == len(reads) - 1 or r.get("wide"):
            r["long_cigar"] = True
            r["aux"] = AUX_EVERY_TYPE if n_cg % 2 == 0 else b""
            n_cg += 1
    reads[0]["mapq"] = 60
    bam = str(tmp_path / "in.bam")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=19)
    edges = list(range(5000, 56000, 5000))
    kept = [r for r in reads if r.get("long_cigar") and _passes(r, 1, edges[0] - 100, edges[-1] + 100)]
    assert len(kept) > 30 and any(r["reverse"] for r in kept) and any(not r["reverse"] for r in kept)
    assert any(sum(1 for a, b in zip(edges[:-1], edges[1:]) if r["pos"] < b + 100 and r["pos"] + bu.ref_length(r["cigar"]) > a - 100) >= 3 for r in kept)
    assert reads[0].get("long_cigar") and reads[-1].get("long_cigar")
    want = _host_and_device(bam, "ctg", ref, edges, 1, monkeypatch, len(kept))
    assert sum(len(g["candidates"]) for g in want) > 50


def test_a_count_above_16_bits_passes_through_the_tables(tmp_path, monkeypatch):
    """One read with 70 000 operations (1M 1I alternating: 35 000 reference bases, seven regions) among 50 ordinary reads."""
    rng = np.random.default_rng(914)
    ref = pu.random_reference(rng, 60000)
    reads = pu.simulate_reads(rng, ref, 0, n_reads=400, read_len=(800, 4000))
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])][::2][:50]
    assert len(reads) == 50
    pos = 8000
    seq = "".join(ref[pos + k] + "ACGT"[(k * 7) % 4] for k in range(35000))
    giant = dict(pos=pos, reverse=False, mapq=60, cigar=[(0, 1), (1, 1)] * 35000, seq=seq, qual=(np.arange(70000) % 37 + 3).astype(np.uint8),
                 long_cigar=True, aux=AUX_EVERY_TYPE)
    reads = sorted(reads + [giant], key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "g%d" % i
    bam = str(tmp_path / "giant.bam")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=7)
    _host_and_device(bam, "ctg", ref, list(range(5000, 56000, 5000)), 1, monkeypatch, 1)


def test_malformed_auxiliary_fields_fall_back_quietly(tmp_path, monkeypatch):
    """A Z string without its NUL, a B array longer than the record and an unknown type letter inside placeholder records:
    pack_device gives None or the host walk's tables, and raises nothing."""
    from pepper_amd.variant.bam import BAM_handler, PACKED_READ
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    rng = np.random.default_rng(915)
    ref = pu.random_reference(rng, 20000)
    reads = pu.simulate_reads(rng, ref, 0, n_reads=200, read_len=(300, 2000))
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])][::3][:40]
    for k, aux in ((5, b"XZZno terminator"), (15, b"XBBI" + struct.pack("<I", 100000) + b"\1\2\3\4"), (25, b"XXq\1\2\3\4")):
        reads[k]["long_cigar"], reads[k]["drop_cg"], reads[k]["aux"] = True, k != 25, aux
    for i, r in enumerate(reads):
        r["name"] = "m%d" % i
    bam = str(tmp_path / "bad.bam")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=11)
    for walk in ("1", "0"):
        monkeypatch.setenv("PEPPER_AMD_DEVICE_WALK", walk)
        enc = PackedEncoder(0, arena_bytes=16 << 20)
        handler = BAM_handler(bam)
        out = enc.pack_device(handler, "ctg", [0, 5000], [5100, 19000], False, 0, long_cigars=True)
        assert out is None or len(out) == 3
        # the rung that served the call: the device's walk marks the three records (state 2), pack_headers refuses them (-6)
        # and the host walks the span after all -- once; without the device's walk the host's walk is the first rung, not counted
        assert out is not None and enc.host_walk_spans == (1 if walk == "1" else 0)
        if walk == "1":
            assert int((enc.headers["state"] == 2).sum()) == 3
        # ... and its tables are pack_inflated's for the same span: the three records kept with their core CIGAR
        n_done, region_pairs, counts = out
        data, data_bytes, first, final = host_side._inflate_span(handler, "ctg", 0, 19000)
        reads, pairs = np.zeros(4000, PACKED_READ), np.zeros(8000, np.int32)
        want_done, want_rp, want_counts = handler.pack_inflated(data, data_bytes, first, final, "ctg", [0, 5000], [5100, 19000], False, 0,
                                                                reads, pairs, long_cigars=True)
        assert (n_done, counts[:2]) == (want_done, want_counts[:2]) and n_done == 2 and counts[0] > 25 and region_pairs.tolist() == want_rp.tolist()
        assert enc.reads[:counts[0]].tobytes() == reads[:counts[0]].tobytes()
        assert enc.pair_read[:counts[1]].tolist() == pairs[:counts[1]].tolist()
        assert enc.seq_off is None and handler.split_offsets(counts[0])[1] == 0
        enc.close()


def test_polish_chain_over_cg_records(tmp_path):
    """PolishChain over pack_device(long_cigars=True) against the same chain over the host packer's arena."""
    from pepper_amd.polish import PEPPER
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    from pepper_amd.variant.bam import BAM_handler
    rng = np.random.default_rng(916)
    draft = pu.random_reference(rng, 3300)
    reads = pu.simulate_reads(rng, draft, 0, n_reads=800, read_len=(300, 1500), ins_rate=0.03, del_rate=0.03)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "q%d" % i
        if i % 4 == 1:
            r["long_cigar"], r["aux"] = True, (AUX_EVERY_TYPE if i % 8 == 1 else b"")
    bam_path = str(tmp_path / "reads.bam")
    bu.write_bam(bam_path, [("ctg1", len(draft))], {0: reads}, flush_every=13)
    bounds = [(0, 1100), (900, 2100), (1900, 3100)]
    starts, stops = [a for a, _ in bounds], [b for _, b in bounds]
    windows = [draft[a:b + 20].encode() for a, b in bounds]
    expect = sum(1 for r in reads if r.get("long_cigar") and _passes(r, 0, 0, 3100))
    assert expect > 10
    for realign in (True, False):
        enc = PackedEncoder(0, 64 << 20, host_threads=1)
        chain = PEPPER.PolishChain(enc)
        bam = BAM_handler(bam_path)
        n_done, region_pairs, counts = enc.pack(bam, "ctg1", starts, stops, False, 0)
        assert n_done == 3
        _rows, live_h, chunks_h = chain.run(bounds, windows, region_pairs, counts, realign=realign)
        want = [a.copy() for a in chain.chunk_arrays()]
        on_device = enc.pack_device(bam, "ctg1", starts, stops, False, 0, long_cigars=True)
        assert on_device is not None and enc.long_cigar_reads == expect and enc.host_walk_spans == 0
        n_done, region_pairs, counts = on_device
        assert n_done == 3
        _rows, live_d, chunks_d = chain.run(bounds, windows, region_pairs, counts, realign=realign, resident=True)
        assert live_d.tolist() == live_h.tolist() and chunks_d.tolist() == chunks_h.tolist() and len(want[0]) > 3
        for g, w in zip(chain.chunk_arrays(), want):
            assert np.array_equal(g, w)
        enc.close()


def _variant_groups(directory):
    out = {}
    for fn in sorted(os.listdir(directory)):
        with h5.File(os.path.join(directory, fn)) as f:
            for name in (f.keys("summaries") if "summaries" in f else []):
                g = "summaries/" + name + "/"
                out[name] = dict(images=f[g + "images"], positions=f[g + "positions"], depths=f[g + "depths"],
                                 candidates=f[g + "candidates"].tolist(), freq=f[g + "candidate_frequency"], contigs=f[g + "contigs"].tolist())
    return out


def _polish_groups(directory):
    out = {}
    for path in glob.glob(os.path.join(directory, "*.hdf")):
        with h5.File(path) as f:
            for name in f.keys("summaries"):
                base = "summaries/" + name + "/"
                out[name] = {k: np.asarray(f[base + k]) for k in ("image", "label", "position", "index", "region_start", "region_end", "chunk_id")}
                out[name]["contig"] = f[base + "contig"]
    return out


def _assert_same_groups(got, want):
    assert sorted(got) == sorted(want) and len(want) > 3
    for name in want:
        for key, w in want[name].items():
            g = got[name][key]
            assert (g == w) if isinstance(w, (str, bytes, list)) else (g.dtype == w.dtype and np.array_equal(g, w)), (name, key)


def test_drivers_keep_cg_reads_on_the_device(tmp_path, monkeypatch):
    """generate_images and the polish make_images on BAMs with CG reads: the files of a run under
    PEPPER_AMD_DEVICE_LONG_CIGARS=0 (the groups with such a read through the host packer), and the counter of reads kept on the
    device above zero in the first run only."""
    from pepper_amd.polish.make_images import make_images
    from pepper_amd.variant.ImageGenerationUI import ImageGenerationUtils
    rng = np.random.default_rng(917)
    ref = pu.random_reference(rng, 16000)
    sites = {int(p): ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.5) for p in rng.choice(np.arange(300, 15000), 40, replace=False)}
    reads = pu.simulate_reads(rng, ref, 0, n_reads=500, read_len=(400, 2500), snp_sites=sites)
    reads = [r for r in reads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(reads):
        r["name"] = "r%d" % i
        if i % 9 == 4:
            r["long_cigar"], r["aux"] = True, (AUX_EVERY_TYPE if i % 2 else b"")
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "ref.fa")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=31)
    with open(fa, "w") as fh:
        fh.write(">ctg\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")

    def options(out, stats):
        return SimpleNamespace(
            bam=bam, fasta=fa, region=None, region_size=2000, threads=2, train_mode=False, use_hp_info=False,
            image_output_directory=out, include_supplementary=False, min_mapq=1, min_snp_baseq=1, min_indel_baseq=1,
            snp_frequency=0.10, insert_frequency=0.15, delete_frequency=0.15, min_coverage_threshold=3,
            snp_candidate_frequency_threshold=0.10, indel_candidate_frequency_threshold=0.12, candidate_support_threshold=2,
            skip_indels=False, downsample_rate=1.0, stage_seconds=stats)
    on, off = {}, {}
    ImageGenerationUtils.generate_images(options(str(tmp_path / "v_on"), on))
    monkeypatch.setenv("PEPPER_AMD_DEVICE_LONG_CIGARS", "0")
    ImageGenerationUtils.generate_images(options(str(tmp_path / "v_off"), off))
    monkeypatch.delenv("PEPPER_AMD_DEVICE_LONG_CIGARS")
    print("variant", {k: (on.get(k), off.get(k)) for k in ("long_cigar_reads_on_device", "bam_pack", "bam_inflate_device")})
    assert on["long_cigar_reads_on_device"] > 0 and off["long_cigar_reads_on_device"] == 0 and "bam_pack" in off
    _assert_same_groups(_variant_groups(str(tmp_path / "v_on")), _variant_groups(str(tmp_path / "v_off")))

    draft = pu.random_reference(rng, 4200)
    preads = pu.simulate_reads(rng, draft, 0, n_reads=600, read_len=(400, 2000), ins_rate=0.03, del_rate=0.03)
    preads = [r for r in preads if not any(op in (3, 6) for op, _ in r["cigar"])]
    for i, r in enumerate(preads):
        r["name"] = "q%d" % i
        if i % 7 == 3:
            r["long_cigar"], r["aux"] = True, (AUX_EVERY_TYPE if i % 2 else b"")
    pbam, pfa = str(tmp_path / "reads.bam"), str(tmp_path / "draft.fa")
    bu.write_bam(pbam, [("ctg1", len(draft))], {0: preads}, flush_every=17)
    with open(pfa, "w") as fh:
        fh.write(">ctg1\n" + draft + "\n")
    monkeypatch.setenv("PEPPER_AMD_POLISH_CHAIN", "1")
    on, off = {}, {}
    make_images(pbam, pfa, None, str(tmp_path / "p_on"), 2, stats=on)
    monkeypatch.setenv("PEPPER_AMD_DEVICE_LONG_CIGARS", "0")
    make_images(pbam, pfa, None, str(tmp_path / "p_off"), 2, stats=off)
    print("polish", {k: (on.get(k), off.get(k)) for k in ("long_cigar_reads_on_device", "bam_pack", "chain")})
    assert on["long_cigar_reads_on_device"] > 0 and off["long_cigar_reads_on_device"] == 0 and "chain" in on and "chain" in off
    _assert_same_groups(_polish_groups(str(tmp_path / "p_on")), _polish_groups(str(tmp_path / "p_off")))
