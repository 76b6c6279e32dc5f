"""One batch through the three forms of staging -- pa_encoder_stage_batch (reads clipped on the host), PackedEncoder.pack + encode
(pa_encoder_stage_packed over host tables) and PackedEncoder.pack_device(device_pack=True) + encode (pa_encoder_stage_packed_device
over tables built on the device) -- at the edges of the region pass: regions of 511, 512 and 513 rows (L + 1) straddle the
512-row tile and leave row_base at three different distances from its 16-row rounding; a fourth region has no read.  Every
form must give the same bytes, and each region the counts it has when encoded alone."""
import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu

pytestmark = pytest.mark.gpu

REGIONS = [(100, 609), (600, 1110), (1100, 1611), (1700, 1800)]          # L + 1 = 511, 512, 513 rows; nothing reaches the last one
PARAMS = (1, 1, 0.1, 0.15, 0.15, 3, 0.1, 0.12, 2, False)
LONG_INSERT = "ACGTACGTTTGACA"                                         # 14 bases: an allele of the pool
SEED = 3


def make_batch(seed=SEED):
    """-> (reference, reads): about 40 reads of 100 to 300 bases over 0 .. 1650, SNPs planted in every region, the long insert
    behind 800, and one read whose soft clip ends where the third region starts (1100, inside the second one too)."""
    rng = np.random.default_rng(seed)
    ref = pu.random_reference(rng, 2000)
    sites = {p: ("ACGT"[("ACGT".index(ref[p]) + 1) % 4], 0.8) for p in (180, 300, 450, 590, 605, 700, 950, 1090, 1105, 1250, 1400, 1580)}
    reads = pu.simulate_reads(rng, ref[:1650], 0, n_reads=46, read_len=(100, 300), snp_sites=sites, mapq_zero_rate=0.0,
                              indel_sites={800: ("I", LONG_INSERT, 0.7)})
    reads = [r for r in reads if not any(op in (pu.OP_N, pu.OP_P) for op, _ in r["cigar"])]      # (the simulator's skips carry read bases)
    clipped = dict(pos=1100, reverse=False, mapq=60, seq="ACGTACGTAC" + ref[1100:1220], qual=np.full(130, 30, np.uint8),
                   cigar=[(pu.OP_S, 10), (pu.OP_M, 120)])
    reads = sorted(reads + [clipped], key=lambda r: r["pos"])
    for i, r in enumerate(reads):
        r["name"] = "r%d" % i
        assert sum(n for op, n in r["cigar"] if op in (pu.OP_M, pu.OP_I, pu.OP_S, pu.OP_EQ, pu.OP_X)) == len(r["seq"])
    return ref, reads


def host_clipped_inputs(handler, ref):
    """-> (generators, flat reads) of the regions as the host-clipped form takes them."""
    from pepper_amd.variant.PEPPER_VARIANT import RegionalSummaryGenerator
    gens = [RegionalSummaryGenerator("ctg", a, b, ref[a:b + 1]) for a, b in REGIONS]
    flats = [handler.get_reads("ctg", a, b, False, 1, 1).as_pileup() for a, b in REGIONS]
    return gens, flats


def _same(got, want, tag):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        for key in ("positions", "depths", "candidate_frequency", "images", "images_int32"):
            assert g[key].dtype == w[key].dtype and np.array_equal(g[key], w[key]), (tag, r, key)
        assert g["candidates"] == w["candidates"] and g["candidates_blob"] == w["candidates_blob"], (tag, r)


def _layout(stats):
    return {k: stats[k] for k in ("rows", "tiles", "regions")}


def test_three_forms_of_one_batch_agree(tmp_path):
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder, StagedBatch
    ref, reads = make_batch()
    bam = str(tmp_path / "in.bam")
    bu.write_bam(bam, [("ctg", len(ref))], {0: reads}, flush_every=11)
    handler = BAM_handler(bam)
    gens, flats = host_clipped_inputs(handler, ref)
    assert flats[3]["n_reads"] == 0 and all(f["n_reads"] > 5 for f in flats[:3])
    # 1. clipped on the host
    batch = StagedBatch(gens, flats, PARAMS, REGIONS)
    counts = batch.run().tolist()
    want = batch.results(want_int32=True)
    assert all(c > 0 for c in counts[:3]) and counts[3] == 0
    assert any(c.startswith("2") and len(c) == 2 + len(LONG_INSERT) for c in want[1]["candidates"])       # the pool's allele
    stats = batch.stats()
    assert stats["tiles"] == 1 + 1 + 2 + 1 and stats["rows"] == 512 + 512 + 528 + 112 and stats["regions"] == 4
    # ... and every region by itself: the same counts (and bytes)
    for r in range(4):
        one = StagedBatch(gens[r:r + 1], flats[r:r + 1], PARAMS, REGIONS[r:r + 1])
        assert one.run().tolist() == counts[r:r + 1]
        _same(one.results(want_int32=True), want[r:r + 1], "alone %d" % r)
    # 2. packed on the host, 3. packed on the device
    starts, stops = [a for a, _ in REGIONS], [b for _, b in REGIONS]
    refs = [ref[a:b + 1] for a, b in REGIONS]
    enc = PackedEncoder(0, arena_bytes=16 << 20, max_reads=4096, max_pairs=8192)
    n_done, rp_h, counts_h = enc.pack(handler, "ctg", starts, stops, False, 1)
    assert n_done == 4 and counts_h[1] > counts_h[0] > 30                   # some reads span two regions
    got_h, live_h = enc.encode(REGIONS, refs, rp_h, counts_h, PARAMS, REGIONS, want_int32=True)
    _same(got_h, want, "packed")
    assert _layout(enc.last.stats()) == _layout(stats)
    assert live_h[3] == 0 and all(0 < n <= p for n, p in zip(live_h[:3].tolist(), np.diff(rp_h).tolist()))
    n_done, rp_d, counts_d = enc.pack_device(handler, "ctg", starts, stops, False, 1, device_pack=True)
    assert n_done == 4 and enc.device_packed and counts_d[:2] == counts_h[:2] and rp_d.tolist() == rp_h.tolist()
    got_d, live_d = enc.encode(REGIONS, refs, rp_d, counts_d, PARAMS, REGIONS, want_int32=True, resident=True)
    _same(got_d, want, "packed on the device")
    assert live_d.tolist() == live_h.tolist() and _layout(enc.last.stats()) == _layout(stats)
    assert enc.pack_calls() == (1, 0)
    enc.close()
