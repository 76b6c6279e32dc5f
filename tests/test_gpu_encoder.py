"""GPU parity of the variant summary encoder (HIP kernels + host allele bookkeeping, through the
C ABI) against the oracle restatement, the reference build where present, and the golden vectors.
Integer work: bit-exact."""
import os

import numpy as np
import pytest

import pileup_utils as pu
import variant_encoder_cases as vc
from test_encoder_oracle import CASES, PRESET_CASES, _case, preset_case

pytestmark = pytest.mark.gpu


class R(object):   # type_read-like view of a simulated read
    def __init__(self, d):
        from pepper_amd.variant.PEPPER_VARIANT import CigarOp, type_read_flags
        self.pos = d["pos"]
        self.flags = type_read_flags()
        self.flags.is_reverse = d["reverse"]
        self.mapping_quality = d["mapq"]
        self.sequence = d["seq"]
        self.base_qualities = list(d["qual"])
        self.cigar_tuples = [CigarOp(o, n) for o, n in d["cigar"]]


def _product(pile, params, reads=None):
    from pepper_amd.variant.PEPPER_VARIANT import RegionalSummaryGenerator
    gen = RegionalSummaryGenerator("chr20", pile.region_start, pile.region_end, pile.reference.decode())
    flat = dict(read_pos=pile.read_pos, read_reverse=pile.read_reverse, read_mapq=pile.read_mapq,
                seq_offset=pile.seq_offset, seq=pile.seq, qual=pile.qual, cigar_offset=pile.cigar_offset,
                cigar_op=pile.cigar_op, cigar_len=pile.cigar_len, n_reads=pile.n_reads)
    gen.generate_max_insert_summary(None)
    return gen.generate_summary_arrays(
        flat if reads is None else reads, params.min_snp_baseq, params.min_indel_baseq, params.snp_freq_threshold,
        params.insert_freq_threshold, params.delete_freq_threshold, params.min_coverage_threshold,
        params.snp_candidate_freq_threshold, params.indel_candidate_freq_threshold,
        params.candidate_support_threshold, bool(params.skip_indels), params.candidate_region_start,
        params.candidate_region_end, 32, 26, False, want_int32=True)


def _check(got, want):
    assert got["candidates"] == want["candidates"]
    assert np.array_equal(got["positions"], want["positions"])
    assert np.array_equal(got["depths"], want["depths"])
    assert np.array_equal(got["candidate_frequency"], want["candidate_frequency"])
    assert np.array_equal(got["images_int32"], want["images"])
    assert np.array_equal(got["images"], want["images"].astype(np.int64).astype(np.int8))   # int8 wrap


@pytest.mark.parametrize("name", sorted(CASES))
def test_encoder_matches_oracle_and_reference(name):
    oracle, ref = pu.load_restatement(), pu.load_reference_encoder()
    pile, params = _case(**CASES[name])
    got = _product(pile, params)
    assert len(got["candidates"]) > 0
    _check(got, pu.run_variant(oracle, pile, params))
    if ref is not None:
        _check(got, pu.run_variant(ref, pile, params, reference_impl=True))


def _both(pile, params):
    oracle, ref = pu.load_restatement(), pu.load_reference_encoder()
    want = pu.run_variant(oracle, pile, params)
    if ref is not None:
        other = pu.run_variant(ref, pile, params, reference_impl=True)
        assert other["candidates"] == want["candidates"] and np.array_equal(other["images"], want["images"])
    return want


def _gen_and_flat(pile):
    from pepper_amd.variant.PEPPER_VARIANT import RegionalSummaryGenerator
    gen = RegionalSummaryGenerator("chr20", pile.region_start, pile.region_end, pile.reference.decode())
    flat = dict(read_pos=pile.read_pos, read_reverse=pile.read_reverse, read_mapq=pile.read_mapq,
                seq_offset=pile.seq_offset, seq=pile.seq, qual=pile.qual, cigar_offset=pile.cigar_offset,
                cigar_op=pile.cigar_op, cigar_len=pile.cigar_len, n_reads=pile.n_reads)
    return gen, flat


def _tile_edge_case(seed, rows, **kw):
    """A region of exactly `rows` positions with SNPs, inserts and deletions planted on the rows either side of every
    256 rows (the tile is 512 rows: every other one is a tile boundary) (the anchor of an indel belongs to the tile before the operation's first row)."""
    rng = np.random.default_rng(seed)
    off = 40_000
    ref = pu.random_reference(rng, rows)
    snps, indels = {}, {}
    for row in range(20, min(rows, 250) - 10, 60):
        snps[off + row] = (rng.choice([c for c in "ACGT" if c != ref[row]]), 0.7)
    for b in range(256, rows - 70, 256):
        for row, what in ((b - 1, "I"), (b, "D"), (b - 2, "D"), (b + 1, "I")):
            indels[off + row] = ("I", "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 9)))), 0.8) if what == "I" \
                else ("D", int(rng.integers(1, 30)), 0.8)
        for row in (b - 3, b + 2):
            rb = ref[row]
            snps[off + row] = (rng.choice([c for c in "ACGT" if c != rb]), 0.7)
    reads = pu.simulate_reads(rng, ref, off, n_reads=int(45 * rows / 900), read_len=(300, 1500), snp_sites=snps,
                              indel_sites=indels, **kw)
    return pu.FlatPileup(off, off + rows - 1, ref, reads), pu.make_params(off, off + rows - 1)


@pytest.mark.parametrize("rows", [1023, 1024, 1025, 511, 512, 513, 256, 255, 700])
def test_tile_boundaries(rows):
    """Region lengths around a multiple of the 512-row tile (at L % 512 == 0 the all-zero row L has a tile of its own)
    and indels / SNPs on the boundary rows."""
    pile, params = _tile_edge_case(100 + rows, rows)
    want = _both(pile, params)
    assert len(want["candidates"]) > 0
    _check(_product(pile, params), want)


def _inner_region_case(seed, **kw):
    """Reads simulated over 9 kb, the generator built on an inner 6 kb of it: reads start before the region, end after
    it, cross it entirely; inserts and deletions up to 600 long (deletions spanning three tiles, inserts summed by the
    whole wave), reads of several kb (tens of tile records each)."""
    rng = np.random.default_rng(seed)
    off, total, lo, hi = 70_000, 9000, 1500, 7500
    ref = pu.random_reference(rng, total)
    snps = {}
    for p in rng.choice(np.arange(off + lo + 30, off + hi - 30), size=25, replace=False):
        rb = ref[p - off]
        snps[int(p)] = (rng.choice([c for c in "ACGT" if c != rb]), float(rng.choice([0.2, 0.6, 1.0])))
    reads = pu.simulate_reads(rng, ref, off, n_reads=140, read_len=(1500, 7000), snp_sites=snps, **kw)
    pile = pu.FlatPileup(off + lo, off + hi, ref[lo:hi + 1], reads)
    return pile, pu.make_params(off + lo + 100, off + hi - 100)


@pytest.mark.parametrize("kw", [dict(), dict(max_indel=600, ins_rate=0.004, del_rate=0.004), dict(skip_rate=0.003, eqx=True),
                                dict(long_indel_rate=0.3, low_q_rate=0.4)])
def test_reads_reaching_over_the_region_edges(kw):
    pile, params = _inner_region_case(7 + len(kw), **kw)
    assert (pile.read_pos < pile.region_start).any() and (pile.read_pos > pile.region_start + 256).any()
    want = _both(pile, params)
    assert len(want["candidates"]) > 0
    _check(_product(pile, params), want)


def test_batch_of_regions_equals_region_by_region():
    """Many regions per launch (pa_encoder_generate_summary_batch): regions of different lengths, depths and candidate
    ranges -- an empty pileup and a region shorter than a tile among them -- give, region by region, what the oracle
    gives for each alone; and a second batch on the same handle does not see the first."""
    from pepper_amd.variant.PEPPER_VARIANT import generate_summary_arrays_batch
    cases = [_case(**CASES["plain"]), _tile_edge_case(3, 1024), _case(**CASES["deep_over_125"]), _inner_region_case(5),
             _case(**CASES["ref_skip_pad_fallthrough"]), _tile_edge_case(4, 90), _case(**CASES["indel_heavy"])]
    rng = np.random.default_rng(9)
    ref = pu.random_reference(rng, 801)
    cases.insert(3, (pu.FlatPileup(5000, 5800, ref, []), pu.make_params(5000, 5800)))
    p0 = cases[0][1]
    for order in (list(range(len(cases))), [6, 2, 0]):
        gens, flats = zip(*[_gen_and_flat(cases[k][0]) for k in order])
        got = generate_summary_arrays_batch(
            list(gens), list(flats), p0.min_snp_baseq, p0.min_indel_baseq, p0.snp_freq_threshold, p0.insert_freq_threshold,
            p0.delete_freq_threshold, p0.min_coverage_threshold, p0.snp_candidate_freq_threshold,
            p0.indel_candidate_freq_threshold, p0.candidate_support_threshold, bool(p0.skip_indels),
            [(cases[k][1].candidate_region_start, cases[k][1].candidate_region_end) for k in order], 32, 26, False, want_int32=True)
        assert len(got) == len(order)
        for k, g in zip(order, got):
            want = pu.run_variant(pu.load_restatement(), *cases[k])
            assert len(want["candidates"]) > 0 or cases[k][0].n_reads < 10
            _check(g, want)


def test_more_tile_records_than_the_first_guess():
    """Reads of few bases that span many tiles (long deletions): the record buffer is sized from the base count, the
    kernels count what did not fit and the run is repeated with room -- same result as the oracle."""
    rng = np.random.default_rng(77)
    off, rows = 5000, 20000
    ref = pu.random_reference(rng, rows)
    reads = []
    for k in range(60):
        cigar, seq = [], []
        pos = int(rng.integers(0, 2000))
        at = pos
        while at < rows - 1200:
            n = int(rng.integers(6, 14))
            b = list(ref[at:at + n])
            if rng.random() < 0.5:
                b[n // 2] = "ACGT"[("ACGT".index(b[n // 2]) + 1) % 4]
            seq.extend(b)
            cigar.append((pu.OP_M, n))
            d = int(rng.integers(500, 1100))
            cigar.append((pu.OP_D, d))
            at += n + d
        seq.extend(ref[at:at + 8])
        cigar.append((pu.OP_M, 8))
        reads.append(dict(pos=off + pos, reverse=bool(k % 2), mapq=30, seq="".join(seq),
                          qual=np.full(len(seq), 20, np.uint8), cigar=cigar))
    reads.sort(key=lambda r: r["pos"])
    pile = pu.FlatPileup(off, off + rows - 1, ref, reads)
    params = pu.make_params(off, off + rows - 1, min_coverage_threshold=1)
    assert pile.seq_offset[-1] // 256 + 2 * len(reads) + 1024 < sum(len(r["cigar"]) // 2 for r in reads) * 3
    want = _both(pile, params)
    _check(_product(pile, params), want)


def test_cigar_past_the_sequence_is_an_error():
    from pepper_amd import _lib
    pile, params = _case(**CASES["plain"])
    r = next(k for k in range(pile.n_reads) if pile.read_mapq[k] > 0 and pile.cigar_op[int(pile.cigar_offset[k])] in (0, 7, 8)
             and pile.read_pos[k] >= pile.region_start)
    pile.cigar_len[int(pile.cigar_offset[r])] += 100000          # a match run of read r now outruns its bases
    with pytest.raises(_lib.PepperAmdError, match="runs past its sequence"):
        _product(pile, params)


@pytest.mark.parametrize("preset", sorted(pu.PRESET_PARAMS))
@pytest.mark.parametrize("name", sorted(PRESET_CASES))
def test_encoder_under_reference_presets(preset, name):
    """BASELINE configs[3] (--hifi) and the CLR / R10 presets through the HIP encoder: min base quality 10 / 0,
    their frequency and coverage thresholds (SetParameters.py:122-256), on pileups where a fifth to a half of the bases
    sit below the cut-off so the quality branches of region_summary.cpp:366-454 decide coverage, votes and inserts."""
    oracle, ref = pu.load_restatement(), pu.load_reference_encoder()
    pile, params = preset_case(preset, name)
    got = _product(pile, params)
    assert len(got["candidates"]) > 0
    _check(got, pu.run_variant(oracle, pile, params))
    if ref is not None:
        _check(got, pu.run_variant(ref, pile, params, reference_impl=True))


def test_encoder_golden_vectors(golden_dir):
    for name in sorted(CASES)[:4]:
        g = np.load(os.path.join(golden_dir, f"encoder_variant_{name}.npz"))
        pile, params = _case(**CASES[name])
        got = _product(pile, params)
        assert got["candidates"] == [s for s in str(g["candidates"]).split("\n") if s]
        assert np.array_equal(got["images_int32"].astype(np.int16), g["images"])
        assert np.array_equal(got["positions"], g["positions"])


def test_encoder_object_interface_and_edges():
    """pybind-shaped interface: type_read-like objects in, CandidateImageSummary objects out; rare
    alphabet (N / lower-case read bases -> exact allele keys); empty pileup; region-edge windows."""
    from pepper_amd.variant.PEPPER_VARIANT import RegionalSummaryGenerator
    oracle = pu.load_restatement()
    rng = np.random.default_rng(5)
    ref = pu.random_reference(rng, 801)
    reads = pu.simulate_reads(rng, ref, 5000, 120, read_len=(150, 400), snp_sites={5300: ("G" if ref[300] != "G" else "T", 0.6)})
    for r in reads[::7]:          # sprinkle N and lower-case bases into some reads
        s = list(r["seq"])
        for k in range(0, len(s), 11):
            s[k] = "N" if k % 2 else s[k].lower()
        r["seq"] = "".join(s)
    pile = pu.FlatPileup(5000, 5800, ref, reads)
    params = pu.make_params(5000, 5800)
    want = pu.run_variant(oracle, pile, params)
    assert any(len(c) == 2 and c[1] not in "ACGT" for c in want["candidates"])   # rare-alphabet alleles present
    gen = RegionalSummaryGenerator("chr20", 5000, 5800, ref)
    objs = gen.generate_summary([R(d) for d in reads], 1, 1, 0.10, 0.15, 0.15, 3, 0.10, 0.12, 2, False, 5000, 5800,
                                32, 26, False)
    assert [o.candidates[0] for o in objs] == want["candidates"]
    assert [o.position for o in objs] == want["positions"].tolist()
    assert np.array_equal(np.array([o.image_matrix for o in objs]), want["images"])
    assert objs[0].contig == "chr20" and objs[0].candidate_frequency == [int(want["candidate_frequency"][0])]
    # windows of candidates within 16 rows of the region edges are zero padded: tests/variant_encoder_cases.py region_edges / snp
    # has a SNP candidate on rows 0, 1, 15, 16, 17, L - 18, L - 17, L - 16, L - 2 and L - 1 of a region of L = 100 rows.  Window
    # row w of a candidate on row r shows row r - 16 + w; every row inside the region holds its reference code, row L is all zero
    case = vc.region_edges()["snp"]
    n_rows = case[1] - case[0] + 1
    edge = _product(vc.pileup(case), vc.params(case))
    _check(edge, pu.run_variant(oracle, vc.pileup(case), vc.params(case)))
    rows = (edge["positions"] - case[0]).tolist()
    assert rows == list(vc.EDGE_SITES) and min(rows) == 0 and max(rows) == n_rows - 1
    for r, img in zip(rows, edge["images_int32"]):
        if r < 16:
            assert not img[:16 - r].any() and img[16 - r].any(), r             # rows 0 .. 15 - r lie in front of the region
        else:
            assert img[0].any(), r
        if r >= n_rows - 16:
            assert img[n_rows - 1 - r + 16].any() and not img[n_rows - r + 16:].any(), r    # row L and everything behind it
        else:
            assert img[32].any(), r
    # empty pileup
    empty = pu.FlatPileup(5000, 5800, ref, [])
    assert _product(empty, params)["candidates"] == []


def test_insert_in_front_of_the_first_aligned_base_on_a_tile_boundary():
    """S I M reads that start exactly on row 512 / 1024: the insert is anchored on the last row of the previous tile, a tile
    the read does not otherwise touch."""
    rng = np.random.default_rng(91)
    off, rows = 30_000, 1600
    ref = pu.random_reference(rng, rows)
    reads = pu.simulate_reads(rng, ref, off, n_reads=70, read_len=(300, 900))
    for k in range(24):
        row0 = 512 * (1 + k % 2)
        n = 200 + 7 * k
        ins = "ACGTTG"[:1 + k % 4]
        reads.append(dict(pos=off + row0, reverse=bool(k % 2), mapq=30, seq="TT" + ins + ref[row0:row0 + n],
                          qual=np.full(2 + len(ins) + n, 25, np.uint8), cigar=[(pu.OP_S, 2), (pu.OP_I, len(ins)), (pu.OP_M, n)]))
    reads.sort(key=lambda r: r["pos"])
    pile = pu.FlatPileup(off, off + rows - 1, ref, reads)
    params = pu.make_params(off, off + rows - 1)
    want = _both(pile, params)
    assert any(c[0] == "2" for c, p in zip(want["candidates"], want["positions"]) if p - off in (511, 1023))
    _check(_product(pile, params), want)
    # the polish encoder counts the same inserts into the insert slots of rows 511 / 1023
    from pepper_amd.polish.PEPPER import SummaryGenerator
    want_img, want_pos = pu.run_polish_oracle(pu.load_restatement(), pile, off, off + rows - 1)
    gen = SummaryGenerator(ref, "contig_1", off, off + rows - 1)
    gen.generate_summary([R(d) for d in reads], off, off + rows - 1)
    assert ((want_pos[:, 0] == off + 511) & (want_pos[:, 1] > 0)).any()
    assert np.array_equal(gen.positions_array, want_pos) and np.array_equal(gen.image, want_img)


def _polish_cases():
    cases = []
    for seed, kw in ((21, {}), (22, dict(ins_rate=0.04, del_rate=0.04)), (23, dict(skip_rate=0.01, eqx=True))):
        rng = np.random.default_rng(seed)
        ref = pu.random_reference(rng, 1201)
        indels = {7300: ("I", "ACGTAC", 0.5), 7600: ("D", 9, 0.6), 7900: ("I", "T", 0.9), 7511: ("I", "GG", 0.7), 7512: ("D", 3, 0.7)}
        reads = pu.simulate_reads(rng, ref, 7000, 90, read_len=(200, 700), indel_sites=indels, **kw)
        cases.append((pu.FlatPileup(7000, 8200, ref, reads), reads, ref, 7000, 8200, 7000, 8200))
    # reads simulated over 4 kb, the generator built on an inner 2.5 kb, summarised over a span that is wider on one side and
    # narrower on the other: reads crossing both edges, deletions of hundreds of bases, rows outside the region (all zero)
    rng = np.random.default_rng(24)
    ref = pu.random_reference(rng, 4000)
    reads = pu.simulate_reads(rng, ref, 50_000, 80, read_len=(800, 3500), max_indel=300, ins_rate=0.004, del_rate=0.004)
    cases.append((pu.FlatPileup(50_700, 53_199, ref[700:3200], reads), reads, ref[700:3200], 50_700, 53_199, 50_650, 53_100))
    return cases


def test_polish_encoder_device_walk_and_batches():
    """The polish walk on the device (tile records, insert slots by prefix sums) against the oracle restatement: single regions,
    a span that differs from the generator's region, and all of them as one batch."""
    from pepper_amd.polish.PEPPER import SummaryGenerator, generate_summaries
    oracle = pu.load_restatement()
    cases = _polish_cases()
    wants = [pu.run_polish_oracle(oracle, c[0], c[5], c[6]) for c in cases]
    for c, (want_img, want_pos) in zip(cases, wants):
        gen = SummaryGenerator(c[2], "contig_1", c[3], c[4])
        gen.generate_summary([R(d) for d in c[1]], c[5], c[6])
        assert np.array_equal(gen.positions_array, want_pos)
        assert np.array_equal(gen.image, want_img)
    gens = [SummaryGenerator(c[2], "contig_1", c[3], c[4]) for c in cases]
    generate_summaries(gens, [[R(d) for d in c[1]] for c in cases], [(c[5], c[6]) for c in cases])
    for g, (want_img, want_pos) in zip(gens, wants):
        assert np.array_equal(g.positions_array, want_pos) and np.array_equal(g.image, want_img)
    assert wants[3][0].shape[0] > 53_100 - 50_650 + 1 and (wants[3][1][:50, 0] < 50_700).all()


def test_polish_encoder_matches_oracle():
    """Polish summary encoder against the oracle restatement (itself pinned to the reference build by
    tests/test_encoder_oracle.py):
    insert columns, deletion-coverage quirk, REF_SKIP/PAD as gaps, 254 scaling truncation."""
    from pepper_amd.polish.PEPPER import SummaryGenerator
    oracle = pu.load_restatement()
    for seed, kw in ((21, {}), (22, dict(ins_rate=0.04, del_rate=0.04)), (23, dict(skip_rate=0.01, eqx=True))):
        rng = np.random.default_rng(seed)
        ref = pu.random_reference(rng, 1201)
        indels = {7300: ("I", "ACGTAC", 0.5), 7600: ("D", 9, 0.6), 7900: ("I", "T", 0.9)}
        reads = pu.simulate_reads(rng, ref, 7000, 90, read_len=(200, 700), indel_sites=indels, **kw)
        pile = pu.FlatPileup(7000, 8200, ref, reads)
        want_img, want_pos = pu.run_polish_oracle(oracle, pile, 7000, 8200)
        gen = SummaryGenerator(ref, "contig_1", 7000, 8200)
        gen.generate_summary([R(d) for d in reads], 7000, 8200)
        assert gen.image.shape == want_img.shape and len(gen.image) > 1201       # insert rows present
        assert np.array_equal(gen.positions_array, want_pos)
        assert np.array_equal(gen.image, want_img)
        assert gen.genomic_pos[0] == (7000, 0)


def test_polish_chunker():
    from pepper_amd.polish.AlignmentSummarizer import AlignmentSummarizer

    class S(object):
        pass
    s = S()
    rows = 2300
    s.image = (np.arange(rows * 10) % 251).astype(np.uint8).reshape(rows, 10)
    s.genomic_pos = [(100 + i, 0) for i in range(rows)]
    images, labels, positions, ids = AlignmentSummarizer.chunk_images(s, 1000, 50)
    # chunk starts: 0, 950, 1900 ; last chunk holds rows 1900..2299 then padding
    assert ids == [0, 1, 2] and all(im.shape == (1000, 10) for im in images)
    assert np.array_equal(images[1][0], s.image[950]) and np.array_equal(images[2][399], s.image[2299])
    assert (images[2][400:] == 0).all() and tuple(positions[2][400]) == (-1, -1) and tuple(positions[2][399]) == (2399, 0)
    s.image, s.genomic_pos = s.image[:1000], s.genomic_pos[:1000]
    images, _, _, ids = AlignmentSummarizer.chunk_images(s, 1000, 50)
    assert ids == [0]


def test_polish_encoder_against_the_reference_build_and_the_goldens(golden_dir):
    """The HIP polish encoder compared DIRECTLY with the reference's own SummaryGenerator (oracle/_ref/libref_polish_encoder.so,
    built from summary_generator.cpp as it lies; it travels with the snapshot) on the six pileup families of
    tests/test_encoder_oracle.py, and with the committed golden vectors written by that build (tests/golden/
    encoder_polish_*.npz) -- one hop, not two; single calls and all six as one batch (the device-side sizing of the outputs:
    the "deep" and "long_inserts" families need several times the rows of the others)."""
    from test_encoder_oracle import POLISH_CASES, _polish_case
    from pepper_amd.polish.PEPPER import SummaryGenerator, generate_summaries
    ref_lib = pu.load_reference_polish_encoder()

    def flat_of(pile):
        return dict(read_pos=pile.read_pos, read_reverse=pile.read_reverse, read_mapq=pile.read_mapq, seq_offset=pile.seq_offset,
                    seq=pile.seq, qual=pile.qual, cigar_offset=pile.cigar_offset, cigar_op=pile.cigar_op, cigar_len=pile.cigar_len,
                    n_reads=pile.n_reads)
    gens, reads_list, spans, wants = [], [], [], []
    for name in sorted(POLISH_CASES):
        pile, start, end = _polish_case(**POLISH_CASES[name])
        want = pu.run_polish_reference(ref_lib, pile, start, end) if ref_lib is not None else None
        golden = os.path.join(golden_dir, f"encoder_polish_{name}.npz")
        if os.path.exists(golden):
            g = np.load(golden, allow_pickle=False)
            if want is not None:
                assert np.array_equal(want[0], g["image"]) and np.array_equal(want[1], g["positions"])
            want = (g["image"], g["positions"])
        if want is None:
            continue
        gen = SummaryGenerator(pile.reference, "contig_1", start, end)
        gen.generate_summary(flat_of(pile), start, end)
        assert np.array_equal(gen.positions_array, want[1]) and np.array_equal(gen.image, want[0]), name
        gens.append(SummaryGenerator(pile.reference, "contig_1", start, end))
        reads_list.append(flat_of(pile))
        spans.append((start, end))
        wants.append(want)
    assert len(wants) >= 3                         # the goldens at least; all six where oracle/_ref travelled
    generate_summaries(gens, reads_list, spans)
    for g, (img, pos) in zip(gens, wants):
        assert np.array_equal(g.positions_array, pos) and np.array_equal(g.image, img)
